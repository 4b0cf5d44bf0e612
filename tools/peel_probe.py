"""Depth peeling (srz_frameset_peel_visibility) beside the visibility render of BASELINE configs 2 and 4, in one process, alternating.

    python tools/peel_probe.py [steps] [--configs 2,4] [--out FILE]

Per config: one frameset of bench.py's batch size and three buffers; after warm-up the visibility render (layer 1), the peel of
layer 1 (layer 2) and the peel of layer 2 (layer 3) alternate, each timed with device events on its own.  Prints one JSON line per
config (medians and p10 / p90 in ms per call, each peel's share of the visibility render, the pixels every layer owns) and writes
them to --out.  Nothing is asserted."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import srz  # noqa: E402
from srz import abi, scenes  # noqa: E402

# (config, workload, frames per step): bench.py's batch sizes (tools/vis_probe.py)
CONFIGS = [(2, "spot_texture_1024", 256), (4, "spot_x16_texture_2048", 128)]


def frames_of(wl_name, n, ctx):
    wl = scenes.WORKLOADS[wl_name]()
    uniq = [wl.frame(i) for i in range(min(n, 36))]
    wl.upload_textures(ctx)  # (after the frames: they load the textures)
    return [uniq[i % len(uniq)] for i in range(n)]


def pct(xs, q):
    return float(np.percentile(np.asarray(xs), q))


def main():
    args = sys.argv[1:]
    steps = int(args[0]) if args and args[0].isdigit() else 20
    pick = {2, 4}
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
        fs = ctx.frameset(frames_of(wl_name, n, ctx))
        l1, l2, l3 = (torch.empty(fs.out_shape, dtype=torch.float32, device="cuda") for _ in range(3))
        sp = s.cuda_stream
        calls = {"visibility": lambda: fs.render_visibility(l1.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, sp),
                 "peel_2": lambda: fs.peel_visibility(l1.data_ptr(), l2.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, sp),
                 "peel_3": lambda: fs.peel_visibility(l2.data_ptr(), l3.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, sp)}
        for _ in range(8):  # warm-up: clock ramp, the pool's growth
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(steps):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn()
                e1.record(s)
                times[k].append((e0, e1))
        torch.cuda.synchronize()
        row = {"config": cfg, "workload": wl_name, "frames": n, "steps": steps, "slow_tiles": fs.debug_counters()["slow_tiles"]}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90)}
        for k in ("peel_2", "peel_3"):
            row[k + "_over_visibility"] = row[k]["ms_median"] / row["visibility"]["ms_median"]
        row["owned_pixels"] = [int((t.view(torch.int32)[:, 1, :fs.height] != 0).sum()) for t in (l1, l2, l3)]
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del l1, l2, l3
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
