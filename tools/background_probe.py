"""The background pass over a visibility buffer (srz_frameset_background / _background_grad) beside the cube lookup
(srz_frameset_texture_cube / _texture_cube_grad), BASELINE configs 1-5, in one process, alternating.

    python tools/background_probe.py [rounds] [--configs 2] [--out FILE]

tools/cube_probe.py's sets, visibility buffers, direction planes and cube (6 x 256^2 at C = 3, shared by every frame).  The ray block
is view_rays of the reference's camera for the set's frame size, shared by every frame.  After 10 warm-up rounds the calls alternate,
each timed with device events on its own; the median of the rounds (default 20) is reported with p10 and p90: the background's
forward at nobody's pixels and at all pixels, its backward with gtex only (the build without partials), with gray only and with both,
and texture_cube's forward, gtex-only and gdir-only backward.  Counted from the buffers: the owned pixels and nobody's.  Prints one JSON
line per config and writes them to --out.  Nothing is asserted."""
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
from cube_probe import normals_of  # noqa: E402
from srz import abi  # noqa: E402
from srz.visibility import cube_dirs, view_rays  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

C, N = 3, 256
WARMUP = 10


def camera(w, h):
    """screen <- world of the reference's camera (eye (0, 0, 0.9) at the origin, lookAtLH, perspectiveLH_NO with 45 handed to a radians
    api) in binary64, mathematical layout"""
    t = np.tan(45.0 / 2)
    view = np.array([[-1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0.9], [0, 0, 0, 1]])
    proj = np.array([[1 / (w / h * t), 0, 0, 0], [0, 1 / t, 0, 0], [0, 0, 100.1 / 99.9, -20.0 / 99.9], [0, 0, 1, 0]])
    scr = np.array([[w / 2 * (w / h), 0, 0, w / 2], [0, h / 2, 0, h / 2], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    return scr @ proj @ view


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    pick = {2}
    out_path = None
    if "--configs" in args:
        pick = {int(c) for c in args[args.index("--configs") + 1].split(",")}
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    sp, F = s.cuda_stream, abi.FUSED_CLEAR
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
        dirs = torch.empty(fs.interpolate_shape(3), dtype=torch.float32, device="cuda")
        nb = fs.interpolate_bytes(C)
        fs.render_visibility(vis.data_ptr(), fs.out_bytes, F, sp)
        fs.interpolate(vis.data_ptr(), attr.data_ptr(), 3, n, T, dirs.data_ptr(), fs.interpolate_bytes(3), F, sp)
        torch.cuda.synchronize()
        H, W = fs.local_rows, fs.width
        ray = view_rays(torch.as_tensor(camera(W, H))).cuda()
        ids = vis.view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
        n_own = int(((ids > 0) & (ids <= T)).sum())
        del ids
        out = torch.empty(fs.interpolate_shape(C), dtype=torch.float32, device="cuda")
        gout = torch.randn(fs.interpolate_shape(C), device="cuda")
        gtex, gdir, gray = torch.zeros_like(cube), torch.empty_like(dirs), torch.empty_like(ray)
        wb = fs.background_work_bytes()
        work = torch.empty(wb // 4, dtype=torch.float32, device="cuda")
        v, r, t, g = vis.data_ptr(), ray.data_ptr(), cube.data_ptr(), gout.data_ptr()

        def bg_bwd(where, want_tex, want_ray):
            return lambda: fs.background_grad(v, r, 1, g, t, N, C, 1, where, gtex.data_ptr() if want_tex else None,
                                              gray.data_ptr() if want_ray else None, work.data_ptr() if want_ray else None, wb if want_ray else 0, F, sp)

        def cube_bwd(want_tex, want_dir):
            return lambda: fs.texture_cube_grad(v, dirs.data_ptr(), g, t, N, C, 1, gtex.data_ptr() if want_tex else None,
                                                gdir.data_ptr() if want_dir else None, F, sp)
        calls = {"background_nobody": lambda: fs.background(v, r, 1, t, N, C, 1, abi.BG_NOBODY, out.data_ptr(), nb, F, sp),
                 "background_all": lambda: fs.background(None, r, 1, t, N, C, 1, abi.BG_ALL, out.data_ptr(), nb, F, sp),
                 "background_grad_gtex": bg_bwd(abi.BG_NOBODY, True, False), "background_grad_gray": bg_bwd(abi.BG_NOBODY, False, True),
                 "background_grad_both": bg_bwd(abi.BG_NOBODY, True, True), "background_all_grad_both": bg_bwd(abi.BG_ALL, True, True),
                 "texture_cube": lambda: fs.texture_cube(v, dirs.data_ptr(), t, N, C, 1, out.data_ptr(), nb, F, sp),
                 "texture_cube_grad_gtex": cube_bwd(True, False), "texture_cube_grad_gdir": cube_bwd(False, True)}
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
               "pixels": n * H * W, "owned_pixels": n_own, "nobodys_pixels": n * H * W - n_own}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del vis, dirs, out, gout, gdir, attr
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
