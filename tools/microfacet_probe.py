"""The Cook-Torrance pass over a visibility buffer (srz_frameset_microfacet / _microfacet_grad) beside the Blinn-Phong pass
(srz_frameset_light / _light_grad) on the same set, in one process, alternating.

    python tools/microfacet_probe.py [rounds] [--frames N] [--lights 3] [--out FILE]

tools/light_probe.py's set (poses of BASELINE config 2's mesh; --frames, default 8, of 1024^2), one visibility buffer of it, the normal
planes interpolate writes for the frames' own per-vertex normals, position planes from a linear ramp over the frame, base colour
planes of uniform noise, roughness and metallic planes uniform over [-0.1, 1.1], one parameter frame shared by every frame (light: p =
5).  After 5 warm-up rounds the calls alternate, each timed with device events on its own; the median of the rounds (default 20) is
reported with p10 and p90: the two forwards, the two backwards with the planes only, and with the planes and gpar.  Beside them the
bytes each pass moves per owned pixel, and their ratio.  Prints one JSON line per light count and writes them to --out.  Nothing is
asserted: timing is recorded."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

import lightref  # noqa: E402
import microfacetref  # noqa: E402
import srz  # noqa: E402
from cube_probe import normals_of  # noqa: E402
from light_probe import P, timed  # noqa: E402
from srz import abi  # noqa: E402
from vis_probe import CONFIGS, frames_of  # noqa: E402

# 4-byte words per owned pixel beside the id plane every pixel reads — light: nrm, pos, kd in, out; backward: + gout in, three
# gradients out.  microfacet: + two material planes in; backward: + two material gradient planes out
WORDS = {"light": 9 + 3, "light_grad": 12 + 9, "microfacet": 11 + 3, "microfacet_grad": 14 + 11}


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    n_frames, lights, out_path = 8, (3,), None
    if "--frames" in args:
        n_frames = int(args[args.index("--frames") + 1])
    if "--lights" in args:
        lights = tuple(int(c) for c in args[args.index("--lights") + 1].split(","))
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
    H, W = fs.local_rows, fs.width
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda") * (2.0 / H) - 1, torch.arange(W, device="cuda") * (2.0 / W) - 1, indexing="ij")
    pos = torch.stack([xs, ys, 0.1 * xs - 0.2 * ys]).expand(n_frames, 3, H, W).contiguous()
    base = torch.rand(fs.interpolate_shape(3), device="cuda") * 0.9 + 0.1
    mat = torch.rand(fs.interpolate_shape(2), device="cuda") * 1.2 - 0.1
    gout = torch.randn(fs.interpolate_shape(3), device="cuda")
    out, gn, gp, gb = (torch.empty_like(nrm) for _ in range(4))
    gm = torch.empty_like(mat)
    ids = vis.view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
    n_own = int(((ids > 0) & (ids <= T)).sum())
    del ids
    torch.cuda.synchronize()
    pixels, nb, rows = n_frames * H * W, fs.interpolate_bytes(3), []
    for L in lights:
        lpar = torch.as_tensor(lightref.make_params(7, L)).cuda().reshape(1, -1).contiguous()
        mpar = torch.as_tensor(microfacetref.make_params(7, L)).cuda().reshape(1, -1).contiguous()
        lgpar, mgpar = torch.empty_like(lpar), torch.empty_like(mpar)
        lwb, mwb = fs.light_work_bytes(L), fs.microfacet_work_bytes(L)
        work = torch.empty(max(lwb, mwb) // 4, dtype=torch.float32, device="cuda")

        def light_bwd(with_par):
            return lambda: fs.light_grad(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), base.data_ptr(), lpar.data_ptr(), L, 1, P,
                                         gout.data_ptr(), gn.data_ptr(), gp.data_ptr(), gb.data_ptr(), lgpar.data_ptr() if with_par else None,
                                         work.data_ptr() if with_par else None, lwb if with_par else 0, F, sp)

        def mf_bwd(with_par):
            return lambda: fs.microfacet_grad(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), base.data_ptr(), mat.data_ptr(), mpar.data_ptr(),
                                              L, 1, gout.data_ptr(), gn.data_ptr(), gp.data_ptr(), gb.data_ptr(), gm.data_ptr(),
                                              mgpar.data_ptr() if with_par else None, work.data_ptr() if with_par else None,
                                              mwb if with_par else 0, F, sp)
        calls = {"light": lambda: fs.light(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), base.data_ptr(), lpar.data_ptr(), L, 1, P,
                                           out.data_ptr(), nb, F, sp),
                 "microfacet": lambda: fs.microfacet(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), base.data_ptr(), mat.data_ptr(),
                                                     mpar.data_ptr(), L, 1, out.data_ptr(), nb, F, sp),
                 "light_grad_planes": light_bwd(False), "microfacet_grad_planes": mf_bwd(False),
                 "light_grad_planes_gpar": light_bwd(True), "microfacet_grad_planes_gpar": mf_bwd(True)}
        nbytes = {k: 4 * pixels + 4 * w * n_own for k, w in WORDS.items()}
        row = {"config": cfg, "frames": n_frames, "rounds": rounds, "lights": L, "pixels": pixels, "owned_pixels": n_own, "bytes": nbytes,
               "byte_ratio_forward": nbytes["microfacet"] / nbytes["light"],
               "byte_ratio_backward": nbytes["microfacet_grad"] / nbytes["light_grad"]}
        row.update(timed(s, calls, rounds))
        for a, b in (("microfacet", "light"), ("microfacet_grad_planes", "light_grad_planes"),
                     ("microfacet_grad_planes_gpar", "light_grad_planes_gpar")):
            row["time_ratio_" + a] = row[a]["ms_median"] / row[b]["ms_median"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    fs.close()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
