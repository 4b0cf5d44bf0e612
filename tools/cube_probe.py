"""The cube lookup over a visibility buffer (srz_frameset_texture_cube / _texture_cube_grad), BASELINE configs 1-5, in one process,
alternating.

    python tools/cube_probe.py [rounds] [--configs 1,2,3,4,5] [--out FILE]

Per config: one frameset of bench.py's batch size (tools/vis_probe.py's sets: poses of one mesh), one visibility buffer of it and the
direction planes interpolate writes for the frames' own per-vertex normals ([n, T, 3, 3] attributes).  The cube is 6 x 256^2 at C = 3,
shared by every frame: a linear function of the unit direction per channel (cube_dirs).  After 10 warm-up rounds the calls alternate,
each timed with device events on its own; the median of the rounds (default 20) is reported with p10 and p90: the forward pass, the
backward with gtex only, with gdir only and with both, and srz_frameset_texture's forward at C = 3 over the spot texture and the
set's uv planes (the yardstick: the same planes written, two coordinate planes read where the cube pass reads three, the same 12
floats gathered per sampled pixel).  Counted from the buffers: the owned pixels and those whose direction is finite and not zero.
Prints one JSON line per config and writes them to --out.  Nothing is asserted."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import scenes as test_scenes  # noqa: E402
import srz  # noqa: E402
from srz import abi  # noqa: E402
from srz.visibility import cube_dirs  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s: device-to-device copies
C, N = 3, 256
WARMUP = 10


def normals_of(frames):
    """[n, T, 3, 3] float32 on the device: the per-vertex normals of every frame's triangle stream (a set's frames repeat: each
    distinct frame is laid out once)"""
    T = max(sum(len(t) for t in f.tris) for f in frames)
    a = torch.zeros((len(frames), T, 3, 3), dtype=torch.float32, device="cuda")
    seen = {}
    for i, f in enumerate(frames):
        if id(f) not in seen:
            nrm = np.concatenate([t["nrm"] for t in f.tris]) if T else np.zeros((0, 3, 3), np.float32)
            seen[id(f)] = torch.as_tensor(np.ascontiguousarray(nrm, np.float32)).cuda()
        a[i, :seen[id(f)].shape[0]] = seen[id(f)]
    return a, T


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    pick = {1, 2, 3, 4, 5}
    out_path = None
    if "--configs" in args:
        pick = {int(c) for c in args[args.index("--configs") + 1].split(",")}
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    sp, F = s.cuda_stream, abi.FUSED_CLEAR
    tex = torch.as_tensor(np.ascontiguousarray(test_scenes.spot_texture(), np.float32)).cuda()
    th, tw = tex.shape[0], tex.shape[1]
    coef = torch.tensor([[0.3, -0.5, 0.8], [-0.6, 0.2, 0.4], [0.5, 0.7, -0.1]], device="cuda")
    cube = (cube_dirs(N, "cuda") @ coef.T).contiguous()  # [6, N, N, 3]
    rows = []
    for cfg, wl_name, n in CONFIGS:
        if cfg not in pick:
            continue
        frames = frames_of(cfg, wl_name, n, ctx)
        fs = ctx.frameset(frames)
        attr, T = normals_of(frames)
        vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
        uv = torch.empty(fs.gbuffer_shape(abi.GB_UV), dtype=torch.float32, device="cuda")
        dirs = torch.empty(fs.interpolate_shape(3), dtype=torch.float32, device="cuda")
        nb = fs.interpolate_bytes(C)
        fs.render_visibility(vis.data_ptr(), fs.out_bytes, F, sp)
        fs.gbuffer(vis.data_ptr(), uv.data_ptr(), fs.gbuffer_bytes(abi.GB_UV), abi.GB_UV, F, sp)
        fs.interpolate(vis.data_ptr(), attr.data_ptr(), 3, n, T, dirs.data_ptr(), fs.interpolate_bytes(3), F, sp)
        torch.cuda.synchronize()
        H, W = fs.local_rows, fs.width
        pixels = n * H * W
        ids = vis.view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
        own = (ids > 0) & (ids <= T)
        n_own = int(own.sum())
        n_sampled = int((own & torch.isfinite(dirs).all(1) & (dirs != 0).any(1)).sum())
        del ids, own
        out = torch.empty(fs.interpolate_shape(C), dtype=torch.float32, device="cuda")
        gout = torch.randn(fs.interpolate_shape(C), device="cuda")
        gtex, gdir = torch.zeros_like(cube), torch.empty_like(dirs)

        def bwd(want_tex, want_dir):
            return lambda: fs.texture_cube_grad(vis.data_ptr(), dirs.data_ptr(), gout.data_ptr(), cube.data_ptr(), N, C, 1,
                                                gtex.data_ptr() if want_tex else None, gdir.data_ptr() if want_dir else None, F, sp)
        calls = {"forward": lambda: fs.texture_cube(vis.data_ptr(), dirs.data_ptr(), cube.data_ptr(), N, C, 1, out.data_ptr(), nb, F, sp),
                 "backward_gtex": bwd(True, False), "backward_gdir": bwd(False, True), "backward_both": bwd(True, True),
                 "texture_c3": lambda: fs.texture(vis.data_ptr(), uv.data_ptr(), tex.data_ptr(), tw, th, C, 1, abi.TEX_CLAMP, out.data_ptr(), nb, F, sp)}
        for _ in range(WARMUP):  # clock ramp, first launches
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(rounds):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn()
                e1.record(s)
                times[k].append((e0, e1))
        torch.cuda.synchronize()
        row = {"config": cfg, "workload": wl_name or "config1_256", "frames": n, "rounds": rounds, "channels": C, "cube": N,
               "pixels": pixels, "owned_pixels": n_own, "sampled_pixels": n_sampled,
               "forward_floor_ms": (4 * pixels + (12 + 16 * C) * n_sampled + 4 * C * pixels) / COPY_RATE * 1e3,
               "backward_floor_ms": (4 * pixels + 12 * n_sampled + 4 * C * n_sampled) / COPY_RATE * 1e3}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90), "ms_series": [round(x, 4) for x in ms]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del vis, uv, dirs, out, gout, gdir, attr
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
