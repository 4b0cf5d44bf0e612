"""The motion pass (srz_frameset_motion) beside the G-buffer pass, BASELINE configs 1-5, in one process, alternating.

    python tools/motion_probe.py [steps] [--configs 1,2,3,4,5] [--out FILE]

Per config: one frameset of bench.py's batch size (tools/vis_probe.py's sets: poses of one mesh, so every frame has one triangle
count) and one visibility buffer of it.  After warm-up three calls alternate, each timed with device events on its own: gbuffer with
NORMAL | UV | BATCH (the yardstick: the same walk over the same buffer), motion with FLOW | DEPTH and motion with all groups, both at
delta = 1.  Beside each time stands the pass's memory floor, derived from include/srz.h's layouts — motion: 4 bytes of id per pixel;
8 of alpha and beta, 36 of gather and, with TARGET, 8 more per owned pixel of a frame that has a target; 4 written per requested
plane and pixel — and the fraction of the measured copy rate (COPY_RATE) the run reached on those bytes.  Prints one JSON line per
config and writes them to --out.  Nothing is asserted."""
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
from srz.visibility import gbuffer_planes, motion_planes  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s: the device-to-device copy rate measured on MI355X
GB_NUB = abi.GB_NORMAL | abi.GB_UV | abi.GB_BATCH
MASKS = {"motion_fd": abi.MV_FLOW | abi.MV_DEPTH, "motion_all": abi.MV_ALL}
DELTA = 1


def motion_floor_bytes(pixels, owned_with_target, what):
    per_owned = 8 + 36 + (8 if what & abi.MV_TARGET else 0)
    return 4 * pixels + per_owned * owned_with_target + 4 * len(motion_planes(what)) * pixels


def gbuffer_floor_bytes(pixels, owned, what):
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
        vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
        gb = torch.empty(fs.gbuffer_shape(GB_NUB), dtype=torch.float32, device="cuda")
        mv = torch.empty(fs.motion_shape(abi.MV_ALL), dtype=torch.float32, device="cuda")
        sp, F = s.cuda_stream, abi.FUSED_CLEAR
        fs.render_visibility(vis.data_ptr(), fs.out_bytes, F, sp)
        calls = {"gbuffer_nub": lambda: fs.gbuffer(vis.data_ptr(), gb.data_ptr(), fs.gbuffer_bytes(GB_NUB), GB_NUB, F, sp)}
        for name, what in MASKS.items():
            calls[name] = lambda what=what: fs.motion(vis.data_ptr(), mv.data_ptr(), fs.motion_bytes(what), what, DELTA, F, sp)
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
        ids = vis.view(torch.int32)[:, 1]
        owned = int((ids != 0).sum())
        owned_t = int((ids[:n - DELTA] != 0).sum())  # (the last DELTA frames have no target: their ids are not even read)
        row = {"config": cfg, "workload": wl_name or "config1_256", "frames": n, "steps": steps, "delta": DELTA, "pixels": pixels,
               "owned_pixels": owned, "owned_pixels_with_target": owned_t}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90), "ms_series": [round(x, 4) for x in ms]}
        floors = {"gbuffer_nub": gbuffer_floor_bytes(pixels, owned, GB_NUB)}
        floors.update({k: motion_floor_bytes(pixels, owned_t, what) for k, what in MASKS.items()})
        for k, fb in floors.items():
            row[k]["floor_bytes"] = fb
            row[k]["floor_ms"] = fb / COPY_RATE * 1e3
            row[k]["fraction_of_copy_rate"] = fb / (row[k]["ms_median"] * 1e-3) / COPY_RATE
        for k in MASKS:
            row[k]["over_gbuffer_nub"] = row[k]["ms_median"] / row["gbuffer_nub"]["ms_median"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del vis, gb, mv
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
