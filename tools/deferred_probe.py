"""Deferred shading against the colour render (srz_frameset_shade_visibility) of BASELINE configs 1-5, in one process, alternating.

    python tools/deferred_probe.py [steps] [--configs 1,2,3,4,5] [--out FILE]

Per config: one frameset of bench.py's batch size (tools/vis_probe.py's sets).  After warm-up (the clear grid's measurement included)
five calls alternate, each timed with device events on its own: the colour render, the visibility render, a shade of the visibility
buffer into a separate buffer with and without SRZ_FUSED_CLEAR, and a shade in place (on a copy of the visibility buffer, made outside
the timed interval).  Prints one JSON line per config (median / p10 / p90 ms per call, each call's share of the colour render) and writes
them to --out.  Nothing is asserted."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import srz  # noqa: E402
from srz import abi  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402


def main():
    args = sys.argv[1:]
    steps = int(args[0]) if args and args[0].isdigit() else 20
    pick = {1, 2, 3, 4, 5}
    out_path = None
    if "--configs" in args:
        pick = {int(c) for c in args[args.index("--configs") + 1].split(",")}
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    rows = []
    for cfg, wl_name, n in CONFIGS:
        if cfg not in pick:
            continue
        fs = ctx.frameset(frames_of(cfg, wl_name, n, ctx))
        col, vis, out, tmp = (torch.empty(fs.out_shape, dtype=torch.float32, device="cuda") for _ in range(4))
        sp, nb, F = s.cuda_stream, fs.out_bytes, abi.FUSED_CLEAR
        calls = {"colour": lambda: fs.render(col.data_ptr(), nb, F, sp),
                 "visibility": lambda: fs.render_visibility(vis.data_ptr(), nb, F, sp),
                 "shade_fused": lambda: fs.shade_visibility(vis.data_ptr(), out.data_ptr(), nb, F, sp),
                 "shade_not_fused": lambda: fs.shade_visibility(vis.data_ptr(), out.data_ptr(), nb, 0, sp),
                 "shade_in_place": lambda: fs.shade_visibility(tmp.data_ptr(), tmp.data_ptr(), nb, F, sp)}
        for _ in range(30):  # warm-up: clock ramp, the colour render's clear-grid measurement
            calls["colour"]()
        calls["visibility"]()
        for k in ("shade_fused", "shade_not_fused"):
            calls[k]()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(steps):
            for k, fn in calls.items():
                if k == "shade_in_place":
                    tmp.copy_(vis)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn()
                e1.record(s)
                times[k].append((e0, e1))
        torch.cuda.synchronize()
        row = {"config": cfg, "workload": wl_name or "config1_256", "frames": n, "steps": steps}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90)}
        for k in calls:
            row[k]["over_colour"] = row[k]["ms_median"] / row["colour"]["ms_median"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del col, vis, out, tmp
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
