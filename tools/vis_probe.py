"""Colour render against visibility render (srz_frameset_render_visibility) of BASELINE configs 1-5, in one process, alternating.

    python tools/vis_probe.py [steps] [--configs 1,2,3,4,5] [--out FILE]

Per config: one frameset of bench.py's batch size, two output buffers; after warm-up (the clear grid's measurement included) the two
renders alternate, each timed with device events on its own.  Prints one JSON line per config (medians and p10 / p90 in ms per
render, frames per second, the visibility render's share of the colour render) and writes them to --out.  Nothing is asserted."""
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

# (config, workload, frames per step): bench.py's EXTRA_CASES batch sizes, its headline's 256 frames for config 2
CONFIGS = [(1, None, 256), (2, "spot_texture_1024", 256), (3, "spot_bunny_phong_1080p", 128), (4, "spot_x16_texture_2048", 128),
           (5, "spot_x8_overdraw_4096", 64)]


def frames_of(cfg, wl_name, n, ctx):
    if wl_name is None:  # config 1: the 256x256 plumbing frame (three flat triangles)
        import scenes as test_scenes
        return [test_scenes.config1() for _ in range(n)]
    wl = scenes.WORKLOADS[wl_name]()
    uniq = [wl.frame(i) for i in range(min(n, 36))]
    wl.upload_textures(ctx)  # (after the frames: they load the textures)
    return [uniq[i % len(uniq)] for i in range(n)]


def pct(xs, q):
    return float(np.percentile(np.asarray(xs), q))


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
        col = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
        vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
        sp = s.cuda_stream
        renders = {"colour": lambda: fs.render(col.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, sp),
                   "visibility": lambda: fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, sp)}
        for _ in range(30):  # warm-up: clock ramp, the colour render's clear-grid measurement (18 renders after 3 skipped)
            renders["colour"]()
        for _ in range(4):
            renders["visibility"]()
        torch.cuda.synchronize()
        times = {k: [] for k in renders}
        for _ in range(steps):
            for k, fn in renders.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn()
                e1.record(s)
                times[k].append((e0, e1))
        torch.cuda.synchronize()
        row = {"config": cfg, "workload": wl_name or "config1_256", "frames": n, "steps": steps}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90),
                      "frames_per_s": n / (float(np.median(ms)) * 1e-3)}
        row["vis_over_colour"] = row["visibility"]["ms_median"] / row["colour"]["ms_median"]
        # the visibility buffer's floor: 12 bytes written per pixel of an owned tile (planes 1..3) — owned tiles counted on the buffer
        v = vis.view(n, 4, fs.local_rows, fs.width)[:, 1].view(torch.int32)
        H, W = fs.local_rows, fs.width
        Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
        pad = torch.zeros((n, Hp, Wp), dtype=torch.int32, device="cuda")
        pad[:, :H, :W] = v
        owned_tiles = int((pad.view(n, Hp // 32, 32, Wp // 32, 32) != 0).any(dim=4).any(dim=2).sum())
        row["owned_tiles"] = owned_tiles
        row["floor_bytes"] = owned_tiles * 1024 * 12
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del col, vis
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
