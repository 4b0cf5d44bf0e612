"""The G-buffer pass (srz_frameset_gbuffer) beside the shade of a visibility buffer, BASELINE configs 1-5, in one process, alternating.

    python tools/gbuffer_probe.py [steps] [--configs 1,2,3,4,5] [--out FILE]

Per config: one frameset of bench.py's batch size (tools/vis_probe.py's sets) and one visibility buffer of it.  After warm-up three calls
alternate, each timed with device events on its own: shade_visibility with SRZ_FUSED_CLEAR, gbuffer with NORMAL | UV | BATCH, gbuffer
with all four groups.  Beside each G-buffer time stands the pass's memory floor, derived from include/srz.h's layout — 4 bytes of id
per pixel, 8 of alpha and beta + 62 of gather (60 of normals and texture coordinates, a 2-byte batch id) per owned pixel, 4 written per
requested plane and pixel — and the fraction of the measured copy rate (COPY_RATE) the run reached on those bytes.  Prints one JSON line
per config and writes them to --out.  Nothing is asserted."""
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
from srz.visibility import gbuffer_planes  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s: the device-to-device copy rate measured on MI355X
MASKS = {"gbuffer_nub": abi.GB_NORMAL | abi.GB_UV | abi.GB_BATCH, "gbuffer_all": abi.GB_ALL}


def floor_bytes(pixels, owned, what):
    return 4 * pixels + (8 + 62) * owned + 4 * len(gbuffer_planes(what)) * pixels


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
        vis, out = (torch.empty(fs.out_shape, dtype=torch.float32, device="cuda") for _ in range(2))
        gb = torch.empty(fs.gbuffer_shape(abi.GB_ALL), dtype=torch.float32, device="cuda")
        sp, nb, F = s.cuda_stream, fs.out_bytes, abi.FUSED_CLEAR
        fs.render_visibility(vis.data_ptr(), nb, F, sp)
        calls = {"shade_fused": lambda: fs.shade_visibility(vis.data_ptr(), out.data_ptr(), nb, F, sp)}
        for name, what in MASKS.items():
            calls[name] = lambda what=what: fs.gbuffer(vis.data_ptr(), gb.data_ptr(), fs.gbuffer_bytes(what), what, F, sp)
        for _ in range(10):  # warm-up: clock ramp, first launches
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
        pixels = n * fs.local_rows * fs.width
        owned = int((vis.view(torch.int32)[:, 1] != 0).sum())
        row = {"config": cfg, "workload": wl_name or "config1_256", "frames": n, "steps": steps, "pixels": pixels, "owned_pixels": owned}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90)}
        for k, what in MASKS.items():
            fb = floor_bytes(pixels, owned, what)
            row[k]["floor_bytes"] = fb
            row[k]["floor_ms"] = fb / COPY_RATE * 1e3
            row[k]["fraction_of_copy_rate"] = fb / (row[k]["ms_median"] * 1e-3) / COPY_RATE
            row[k]["over_shade"] = row[k]["ms_median"] / row["shade_fused"]["ms_median"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del vis, out, gb
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
