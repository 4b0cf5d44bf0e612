"""SH9 lighting timed beside the all-pairs path it replaces, in one process, alternating.

    python tools/sh_probe.py [rounds] [--frames N] [--env 64] [--out FILE]

tools/ibl_probe.py's set (poses of BASELINE config 2's mesh; --frames, default 8, of 1024^2), one visibility buffer of it, the normal
planes interpolate writes for the frames' own per-vertex normals, an environment cube of --env x --env faces (default 64), C = 3.
Legs, each through srz.visibility (the torch.autograd.Functions, so scratch allocation and autograd's bookkeeping are inside the
timing on both sides alike):
  sh            sh_light(cube_sh(env), nrm)                           forward, and forward + backward to env
  cube          texture_cube(cube_irradiance(env, 8), nrm)            forward, and forward + backward to env
  sh_param      sh_light(sh, nrm) with sh a [9, 3] leaf               forward, and forward + backward to sh: the learned-probe loop
and the plain calls on their own: FrameSet.sh, FrameSet.sh_grad (planes only; with d_gsh), Context.cube_sh, Context.cube_sh_grad.
After 5 warm-up rounds the legs alternate, each timed with device events on its own; the median of the rounds (default 20) is
reported with p10 and p90.  Prints one JSON line and writes it to --out.  Nothing is asserted: timing is recorded."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

import srz  # noqa: E402
from cube_probe import normals_of  # noqa: E402
from light_probe import timed  # noqa: E402
from srz import abi  # noqa: E402
from srz import visibility as V  # noqa: E402
from vis_probe import CONFIGS, frames_of  # noqa: E402

C = 3


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    n_frames, n_env, out_path = 8, 64, None
    if "--frames" in args:
        n_frames = int(args[args.index("--frames") + 1])
    if "--env" in args:
        n_env = int(args[args.index("--env") + 1])
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    sp, F = s.cuda_stream, abi.FUSED_CLEAR
    cfg, wl_name, _ = next(c for c in CONFIGS if c[0] == 2)
    frames = frames_of(cfg, wl_name, n_frames, ctx)
    fs = ctx.frameset(frames)
    attr, T = normals_of(frames)
    vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
    nrm = torch.empty(fs.interpolate_shape(3), dtype=torch.float32, device="cuda")
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, F, sp)
    fs.interpolate(vis.data_ptr(), attr.data_ptr(), 3, n_frames, T, nrm.data_ptr(), fs.interpolate_bytes(3), F, sp)
    del attr
    env = (torch.rand((6, n_env, n_env, C), device="cuda") * 2.0).requires_grad_(True)
    coef = torch.randn((9, C), device="cuda").requires_grad_(True)
    g = torch.randn(fs.interpolate_shape(C), device="cuda")
    ids = vis.view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
    n_own = int(((ids > 0) & (ids <= T)).sum())
    del ids

    def leg(make, leaf, backward):
        def run():
            with torch.set_grad_enabled(backward):
                out = make()
                if backward:
                    torch.autograd.grad(out, leaf, g)
        return run
    by_sh = lambda: V.sh_light(fs, vis, V.cube_sh(ctx, env), nrm)  # noqa: E731
    by_cube = lambda: V.texture_cube(fs, vis, V.cube_irradiance(ctx, env, 8), nrm)  # noqa: E731
    by_param = lambda: V.sh_light(fs, vis, coef, nrm)  # noqa: E731
    out, gn = torch.empty(fs.interpolate_shape(C), device="cuda"), torch.empty_like(nrm)
    shd, gsh, den = coef.detach().clone(), torch.empty((9, C), device="cuda"), torch.empty(1, device="cuda")
    wb, cb = fs.sh_work_bytes(C), ctx.cube_sh_work_bytes(n_env, C, 1)
    work, cwork = torch.empty(wb // 4, device="cuda"), torch.empty(cb // 4, device="cuda")
    envd, genv = env.detach(), torch.empty((6, n_env, n_env, C), device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    calls = {
        "sh_forward": leg(by_sh, env, False), "sh_forward_backward": leg(by_sh, env, True),
        "cube_forward": leg(by_cube, env, False), "cube_forward_backward": leg(by_cube, env, True),
        "sh_param_forward": leg(by_param, coef, False), "sh_param_forward_backward": leg(by_param, coef, True),
        "FrameSet.sh": lambda: fs.sh(p(vis), p(nrm), p(shd), C, 1, abi.SH_IRRADIANCE, p(out), fs.interpolate_bytes(C), F, sp),
        "FrameSet.sh_grad planes": lambda: fs.sh_grad(p(vis), p(nrm), p(shd), C, 1, abi.SH_IRRADIANCE, p(g), p(gn), None, None, 0, F, sp),
        "FrameSet.sh_grad gsh": lambda: fs.sh_grad(p(vis), p(nrm), p(shd), C, 1, abi.SH_IRRADIANCE, p(g), None, p(gsh), p(work), wb, F, sp),
        "Context.cube_sh": lambda: ctx.cube_sh(p(envd), n_env, C, 1, p(gsh), p(den), p(cwork), cb, sp),
        "Context.cube_sh_grad": lambda: ctx.cube_sh_grad(p(shd), p(den), n_env, C, 1, p(genv), p(cwork), cb, sp),
    }
    row = {"rounds": rounds, "frames": n_frames, "width": fs.width, "height": fs.local_rows, "env": n_env, "channels": C, "owned_pixels": n_own}
    row.update(timed(s, calls, rounds))
    for k in ("forward", "forward_backward"):
        row["cube_over_sh_" + k] = row["cube_" + k]["ms_median"] / row["sh_" + k]["ms_median"]
    # the pixel pass against its floor: 4 bytes of id per pixel, 12 of normal read and 4 C written per owned pixel
    moved = 4 * n_frames * fs.width * fs.local_rows + (12 + 4 * C) * n_own
    row["FrameSet.sh"]["gb_per_s"] = moved / row["FrameSet.sh"]["ms_median"] / 1e6
    for v in row.values():
        if isinstance(v, dict):
            v.pop("ms_series", None)
    print(json.dumps(row), flush=True)
    fs.close(), ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
