"""The mipmapped cube lookup (srz_frameset_texture_cube_mip / _texture_cube_mip_grad) beside the flat pair it extends
(srz_frameset_texture_cube / _texture_cube_grad) on the same directions, 256 frames of 1024^2 (BASELINE config 2), in one process,
alternating.

    python tools/cube_mip_probe.py [rounds] [--frames N] [--out FILE]

One frameset of tools/vis_probe.py's config 2, one visibility buffer of it and the direction planes interpolate writes for the
frames' own per-vertex normals.  The cube is 6 x 256^2 at C = 3, shared by every frame (cube_probe.py's), with the box-filtered
pyramid srz_cube_mip_build makes of it (9 levels).  The level plane is a constant: 0 and 2 (ALL-INTEGER: f == 0 everywhere, one level
read, the second level's gathers skipped) and 0.5 and 2.5 (ALL-FRACTIONAL: two levels blended at every sampled pixel).  Per level
plane: the forward; the backward with gtex + gmip and gdir (what the flat pair's backward_both computes, over two levels); the same
with glam on top (which reads level l0 + 1 at an integer level too).  Beside them the flat forward and its backward with gtex and
gdir.  After 10 warm-up rounds the calls alternate, each timed with device events on its own; the median of the rounds (default 20)
is reported with p10 and p90, and the ratio of each mipmapped median to its flat counterpart.  Counted from the buffers: the owned and
the sampled pixels.  Prints one JSON line and writes it to --out.  Nothing is asserted: no threshold exists to hold these to."""
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
from srz.visibility import cube_dirs, cube_mip_build  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

C, N = 3, 256
WARMUP = 10
LEVELS = {"lam_0": 0.0, "lam_2": 2.0, "lam_0.5": 0.5, "lam_2.5": 2.5}


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    cfg, wl_name, n = CONFIGS[1]
    out_path = None
    if "--frames" in args:
        n = int(args[args.index("--frames") + 1])
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    sp, F = s.cuda_stream, abi.FUSED_CLEAR
    coef = torch.tensor([[0.3, -0.5, 0.8], [-0.6, 0.2, 0.4], [0.5, 0.7, -0.1]], device="cuda")
    cube = (cube_dirs(N, "cuda") @ coef.T).contiguous()  # [6, N, N, 3]
    L = srz.cube_mip_levels(N)
    mip = cube_mip_build(ctx, cube)
    frames = frames_of(cfg, wl_name, n, ctx)
    fs = ctx.frameset(frames)
    attr, T = normals_of(frames)
    vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
    dirs = torch.empty(fs.interpolate_shape(3), dtype=torch.float32, device="cuda")
    nb = fs.interpolate_bytes(C)
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, F, sp)
    fs.interpolate(vis.data_ptr(), attr.data_ptr(), 3, n, T, dirs.data_ptr(), fs.interpolate_bytes(3), F, sp)
    torch.cuda.synchronize()
    ids = vis.view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
    own = (ids > 0) & (ids <= T)
    n_own = int(own.sum())
    n_sampled = int((own & torch.isfinite(dirs).all(1) & (dirs != 0).any(1)).sum())
    del ids, own
    out = torch.empty(fs.interpolate_shape(C), dtype=torch.float32, device="cuda")
    gout = torch.randn(fs.interpolate_shape(C), device="cuda")
    gtex, gmip, gdir = torch.zeros_like(cube), torch.zeros_like(mip), torch.empty_like(dirs)
    glam = torch.empty(fs.interpolate_shape(1), dtype=torch.float32, device="cuda")
    lams = {k: torch.full(fs.interpolate_shape(1), v, dtype=torch.float32, device="cuda") for k, v in LEVELS.items()}
    v, d, g, t, m = vis.data_ptr(), dirs.data_ptr(), gout.data_ptr(), cube.data_ptr(), mip.data_ptr()
    calls = {"flat_forward": lambda: fs.texture_cube(v, d, t, N, C, 1, out.data_ptr(), nb, F, sp),
             "flat_backward": lambda: fs.texture_cube_grad(v, d, g, t, N, C, 1, gtex.data_ptr(), gdir.data_ptr(), F, sp)}
    for k, lam in lams.items():
        lp = lam.data_ptr()
        calls[k + "_forward"] = lambda lp=lp: fs.texture_cube_mip(v, d, lp, t, N, C, 1, m, L, out.data_ptr(), nb, F, sp)
        calls[k + "_backward"] = lambda lp=lp: fs.texture_cube_mip_grad(v, d, lp, g, t, m, N, C, 1, L, gtex.data_ptr(), gmip.data_ptr(),
                                                                        gdir.data_ptr(), None, F, sp)
        calls[k + "_backward_glam"] = lambda lp=lp: fs.texture_cube_mip_grad(v, d, lp, g, t, m, N, C, 1, L, gtex.data_ptr(), gmip.data_ptr(),
                                                                             gdir.data_ptr(), glam.data_ptr(), F, sp)
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
    row = {"config": cfg, "workload": wl_name, "frames": n, "rounds": rounds, "channels": C, "cube": N, "levels": L,
           "pixels": n * fs.local_rows * fs.width, "owned_pixels": n_own, "sampled_pixels": n_sampled}
    for k, evs in times.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90), "ms_series": [round(x, 4) for x in ms]}
    for k in lams:
        row[k + "_forward"]["over_flat"] = row[k + "_forward"]["ms_median"] / row["flat_forward"]["ms_median"]
        for b in ("_backward", "_backward_glam"):
            row[k + b]["over_flat"] = row[k + b]["ms_median"] / row["flat_backward"]["ms_median"]
    print(json.dumps(row), flush=True)
    fs.close()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
