"""The image-based-lighting passes over a visibility buffer (srz_frameset_reflect / _reflect_grad, srz_frameset_ibl / _ibl_grad,
srz_brdf_table) beside the Cook-Torrance pass with one light (srz_frameset_microfacet / _microfacet_grad: the sibling of the same
shape) and beside the same rules as float32 torch ops on the device (what a caller wrote before these passes existed), in one
process, alternating.

    python tools/ibl_probe.py [rounds] [--frames N] [--table 32] [--out FILE]

tools/microfacet_probe.py's set (poses of BASELINE config 2's mesh; --frames, default 8, of 1024^2), one visibility buffer of it, the
normal planes interpolate writes for the frames' own per-vertex normals, position planes from a linear ramp over the frame, base
colour, irradiance and specular planes of uniform noise, roughness and metallic planes uniform over [-0.1, 1.1], nv reflect's own
plane 3, one eye shared by every frame, the table brdf_table(--table, 64).  After 5 warm-up rounds the calls alternate, each timed
with device events on its own; the median of the rounds (default 20) is reported with p10 and p90: the forwards, the backwards with
the planes only, ibl_grad with the table's gradient too, the torch legs (forward, and forward + backward through autograd), and
brdf_table once.  Beside them the bytes each pass moves per owned pixel, and their ratio to microfacet's.  Prints one JSON line and
writes it to --out.  Nothing is asserted: timing is recorded."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

import iblref  # noqa: E402
import microfacetref  # noqa: E402
import srz  # noqa: E402
from cube_probe import normals_of  # noqa: E402
from light_probe import timed  # noqa: E402
from srz import abi  # noqa: E402
from vis_probe import CONFIGS, frames_of  # noqa: E402

# 4-byte words per owned pixel beside the id plane every pixel reads — reflect: nrm, pos in, four planes out; backward: + gout in, two
# gradients out.  ibl: base, mat, nv, irr, spec in (the table's words come from cache), out; backward: + gout in, five gradients out.
# microfacet with one light: microfacet_probe's
WORDS = {"reflect": 6 + 4, "reflect_grad": 6 + 4 + 6, "ibl": 12 + 3, "ibl_grad": 12 + 3 + 12, "microfacet": 11 + 3, "microfacet_grad": 14 + 11}


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    n_frames, t, out_path = 8, 32, None
    if "--frames" in args:
        n_frames = int(args[args.index("--frames") + 1])
    if "--table" in args:
        t = int(args[args.index("--table") + 1])
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
    base, irr, spec = (torch.rand(fs.interpolate_shape(3), device="cuda") * 0.9 + 0.1 for _ in range(3))
    mat = torch.rand(fs.interpolate_shape(2), device="cuda") * 1.2 - 0.1
    g3, g4 = torch.randn(fs.interpolate_shape(3), device="cuda"), torch.randn(fs.interpolate_shape(4), device="cuda")
    par = torch.as_tensor(microfacetref.make_params(7, 1)).cuda().reshape(1, -1).contiguous()
    eye = par[0, :3].contiguous()
    rf = torch.empty(fs.interpolate_shape(4), dtype=torch.float32, device="cuda")
    fs.reflect(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), eye.data_ptr(), 1, rf.data_ptr(), fs.interpolate_bytes(4), F, sp)
    nv = rf[:, 3:].contiguous()
    tab = torch.empty((t, t, 2), dtype=torch.float32, device="cuda")
    ctx.brdf_table(tab.data_ptr(), tab.numel() * 4, t, 64, sp)
    gtab = torch.zeros_like(tab)
    out, gn, gp, gb, gi, gs = (torch.empty_like(nrm) for _ in range(6))
    gm, gnv = torch.empty_like(mat), torch.empty_like(nv)
    ids = vis.view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
    n_own = int(((ids > 0) & (ids <= T)).sum())
    del ids
    torch.cuda.synchronize()
    pixels, nb = n_frames * H * W, fs.interpolate_bytes(3)

    def ibl_bwd(with_tab):
        return lambda: fs.ibl_grad(vis.data_ptr(), base.data_ptr(), mat.data_ptr(), nv.data_ptr(), irr.data_ptr(), spec.data_ptr(), tab.data_ptr(), t,
                                   g3.data_ptr(), gb.data_ptr(), gm.data_ptr(), gnv.data_ptr(), gi.data_ptr(), gs.data_ptr(),
                                   gtab.data_ptr() if with_tab else None, F, sp)

    def torch_reflect(backward):
        def run():
            with torch.set_grad_enabled(backward):
                n_, p_ = (nrm.requires_grad_(backward), pos.requires_grad_(backward))
                o = iblref.torch_reflect(n_, p_, eye)
                if backward:
                    torch.autograd.grad(o, (n_, p_), g4)
        return run

    def torch_ibl(backward):
        def run():
            with torch.set_grad_enabled(backward):
                ins = [x.requires_grad_(backward) for x in (base, mat, nv, irr, spec)]
                o = iblref.torch_ibl(*ins, tab)
                if backward:
                    torch.autograd.grad(o, ins, g3)
        return run
    calls = {"reflect": lambda: fs.reflect(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), eye.data_ptr(), 1, rf.data_ptr(),
                                           fs.interpolate_bytes(4), F, sp),
             "ibl": lambda: fs.ibl(vis.data_ptr(), base.data_ptr(), mat.data_ptr(), nv.data_ptr(), irr.data_ptr(), spec.data_ptr(), tab.data_ptr(), t,
                                   out.data_ptr(), nb, F, sp),
             "microfacet": lambda: fs.microfacet(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), base.data_ptr(), mat.data_ptr(), par.data_ptr(), 1, 1,
                                                 out.data_ptr(), nb, F, sp),
             "reflect_grad": lambda: fs.reflect_grad(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), eye.data_ptr(), 1, g4.data_ptr(), gn.data_ptr(),
                                                     gp.data_ptr(), F, sp),
             "ibl_grad": ibl_bwd(False), "ibl_grad_gtab": ibl_bwd(True),
             "microfacet_grad": lambda: fs.microfacet_grad(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), base.data_ptr(), mat.data_ptr(),
                                                           par.data_ptr(), 1, 1, g3.data_ptr(), gn.data_ptr(), gp.data_ptr(), gb.data_ptr(),
                                                           gm.data_ptr(), None, None, 0, F, sp),
             "torch_reflect": torch_reflect(False), "torch_reflect_and_grad": torch_reflect(True),
             "torch_ibl": torch_ibl(False), "torch_ibl_and_grad": torch_ibl(True)}
    nbytes = {k: 4 * pixels + 4 * w * n_own for k, w in WORDS.items()}
    row = {"config": cfg, "frames": n_frames, "rounds": rounds, "table": t, "pixels": pixels, "owned_pixels": n_own, "bytes": nbytes,
           "byte_ratio": {k: nbytes[k] / nbytes["microfacet_grad" if k.endswith("grad") else "microfacet"] for k in WORDS}}
    row.update(timed(s, calls, rounds))
    for k in ("reflect", "ibl", "reflect_grad", "ibl_grad", "ibl_grad_gtab"):
        row["time_ratio_" + k] = row[k]["ms_median"] / row["microfacet_grad" if "grad" in k else "microfacet"]["ms_median"]
    for k, tk in (("reflect", "torch_reflect"), ("ibl", "torch_ibl")):
        row["torch_over_" + k] = row[tk]["ms_median"] / row[k]["ms_median"]
        row["torch_over_" + k + "_and_grad"] = row[tk + "_and_grad"]["ms_median"] / (row[k]["ms_median"] + row[k + "_grad"]["ms_median"])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    big = torch.empty((32, 32, 2), dtype=torch.float32, device="cuda")
    e0.record(s)
    ctx.brdf_table(big.data_ptr(), big.numel() * 4, 32, 64, sp)
    e1.record(s)
    torch.cuda.synchronize()
    row["brdf_table_32_64_ms"] = e0.elapsed_time(e1)
    for v in row.values():
        if isinstance(v, dict):
            v.pop("ms_series", None)
    print(json.dumps(row), flush=True)
    fs.close()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
