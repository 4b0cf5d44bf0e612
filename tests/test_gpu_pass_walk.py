"""-m gpu: the tile walk of the passes over a visibility buffer, beyond the grid's cap.  tile_grid (csrc/srz_kernels.hip) launches at
most 16,384 workgroups, so a set of more tiles sends workgroups round the walk's loop a second time — with whatever they carry from
one tile to the next (the LDS tables of the gradient kernels, k_pos_grad's alternating slot counter, k_tex_mip_grad's rotating level
word).  Only tests/test_gpu_pass_walk_lit.py has that many tiles too: the newer passes, on the same sets (tests/walkkit.py).  Two
shapes, every pass on both:
  many   6,144 frames of 36 x 33: four tiles per frame — a full tile, a 4-pixel column, a 1-row band and a corner —, 24,576 tiles,
         1.5 x the cap, through the walk's branch for eight frames and more; a handful of triangles per frame, different in every
         frame, so that a tile written from the wrong frame shows up;
  large  7 frames of 1568 x 1568: 49 x 49 tiles each, 16,807 tiles, through the branch for fewer than eight frames, which has a
         second iteration only above the cap; a dozen large triangles per frame.
The visibility buffer is the GPU's own render_visibility, uv and uvd the GPU's own interpolate and interpolate_deriv; the expected
values are the references' of the passes' own tests (tests/*ref.py) on those buffers, with the bounds of those tests: the
deterministic planes bit for bit (a NaN on one side must be a NaN on the other), the float-atomic sums within gamma_n * sum |term|,
gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing terms — bit for bit where n = 1, exactly 0 where n = 0;
shade_visibility against the set's own colour render, bit for bit.  Every output starts from a sentinel; every pass that has the flag
also runs without SRZ_FUSED_CLEAR (the frames do not clear either), where nobody's pixels must keep the sentinel."""
import numpy as np
import pytest
import torch

import antialiasref
import gbufref
import interpref
import mipref
import motionref
import posgradref
import texref
import walkkit
from srz import abi
from support import SENTINEL, ctx, filled, frame_positions, stream, words  # noqa: F401
from walkkit import F, SHAPES, TEX_H, TEX_W, check_nobody, check_sum, dev, pre, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worlds(ctx):
    yield from walkkit.make_worlds(ctx)


# ------------------------------------------------------------------------------------------------------ the passes
def run_shade_visibility(tmp, w, fused):
    """against the set's own colour render into the same prefill: z +inf (the frames do not clear: a render tests against it),
    the colour planes the sentinel"""
    fs, flags = w.fs, F if fused else 0
    col = filled(fs.out_shape).view(torch.float32)
    col[:, 0] = float("inf")
    out = col.clone()
    fs.render(col.data_ptr(), fs.out_bytes, flags, stream())
    fs.shade_visibility(w.vis.data_ptr(), out.data_ptr(), fs.out_bytes, flags, stream())
    torch.cuda.synchronize()
    assert torch.equal(col.view(torch.int32), out.view(torch.int32))
    got = words(out)
    check_nobody(w, got[:, 1:], fused, "shade_visibility")


def run_gbuffer(tmp, w, fused):
    fs, what = w.fs, abi.GB_ALL
    out = filled(fs.gbuffer_shape(what))
    fs.gbuffer(w.vis.data_ptr(), out.data_ptr(), fs.gbuffer_bytes(what), what, F if fused else 0, stream())
    torch.cuda.synchronize()
    got = words(out)
    same(got, np.stack([gbufref.expected(tmp, f, {}, w.v[i], fused, pre(w, 9)) for i, f in enumerate(w.frames)]), "gbuffer")
    check_nobody(w, got, fused, "gbuffer")


def run_motion(tmp, w, fused):
    fs, what = w.fs, abi.MV_ALL
    out = filled(fs.motion_shape(what))
    fs.motion(w.vis.data_ptr(), out.data_ptr(), fs.motion_bytes(what), what, 1, F if fused else 0, stream())
    torch.cuda.synchronize()
    want = [motionref.expected(tmp, frame_positions(w.frames[i + 1]), w.v[i], w.v[i + 1], fused, pre(w, 5)) for i in range(w.n - 1)]
    want.append(motionref.nobody(w.v.shape[2:], fused, SENTINEL))  # (the last frame has no target frame)
    got = words(out)
    same(got, np.stack(want), "motion")
    check_nobody(w, got[:-1], fused, "motion")


def run_interpolate(tmp, w, fused):
    fs, C = w.fs, w.C
    a, out = dev(w.attr), filled(w.shape(C))
    fs.interpolate(w.vis.data_ptr(), a.data_ptr(), C, w.n, w.T, out.data_ptr(), fs.interpolate_bytes(C), F if fused else 0, stream())
    torch.cuda.synchronize()
    got = words(out)
    same(got, np.stack([interpref.forward(tmp, w.attr[i], w.n_tris[i], w.v[i], fused, pre(w, C)) for i in range(w.n)]), "interpolate")
    check_nobody(w, got, fused, "interpolate")


def run_interpolate_grad(tmp, w, fused):
    fs, C = w.fs, w.C
    (gout, g), a = w.gout, dev(w.attr)
    ga, gb = torch.zeros_like(a), filled(w.shape(2))
    fs.interpolate_grad(w.vis.data_ptr(), g.data_ptr(), a.data_ptr(), C, w.n, w.T, ga.data_ptr(), gb.data_ptr(), F if fused else 0, stream())
    torch.cuda.synchronize()
    accs = [interpref.Grad(w.attr.shape[1:]) for _ in range(w.n)]
    want = [interpref.grad(tmp, w.attr[i], w.n_tris[i], w.v[i], gout[i], accs[i], True, fused, pre(w, 2)) for i in range(w.n)]
    got = words(gb)
    same(got, np.stack(want), "gbary")
    check_nobody(w, got, fused, "gbary")
    check_sum(ga.cpu().numpy(), np.stack([x.gattr for x in accs]), np.stack([x.gabs for x in accs]),
              np.stack([x.count for x in accs])[:, :, None, None], "gattr")


def run_position_grad(tmp, w, fused):
    fs = w.fs
    gout, g = w.gout
    gb, gz = g[:, :2].contiguous(), g[:, :1].contiguous()
    gp, gx = torch.zeros((w.n, w.T, 3, 3), dtype=torch.float32, device="cuda"), filled(w.shape(2))
    fs.position_grad(w.vis.data_ptr(), gb.data_ptr(), gz.data_ptr(), w.T, gp.data_ptr(), gx.data_ptr(), F if fused else 0, stream())
    torch.cuda.synchronize()
    accs = [posgradref.Grad(w.T) for _ in range(w.n)]
    want = [posgradref.grad(tmp, w.pos[i], w.n_tris[i], w.v[i], gout[i, :2], gout[i, :1], accs[i], True, fused, pre(w, 2)) for i in range(w.n)]
    got = words(gx)
    same(got, np.stack(want), "gpix")
    check_nobody(w, got, fused, "gpix")
    check_sum(gp.cpu().numpy(), np.stack([x.gpos for x in accs]), np.stack([x.gabs for x in accs]),
              np.stack([x.count for x in accs])[:, :, None, None], "gpos")


def run_antialias(tmp, w, fused):
    fs, C = w.fs, w.C
    c, d = w.planes
    out = filled(d.shape)
    fs.antialias(w.vis.data_ptr(), d.data_ptr(), C, out.data_ptr(), fs.interpolate_bytes(C), F, stream())
    torch.cuda.synchronize()
    want = np.stack([antialiasref.forward(tmp, w.pos[i], w.n_tris[i], w.v[i], c[i]) for i in range(w.n)])
    assert (want.view(np.uint32) != c.view(np.uint32)).reshape(w.n, -1).any(1).mean() >= 0.9  # the frames blend somewhere
    same(words(out), want, "antialias")


def run_antialias_grad(tmp, w, fused):
    fs, C = w.fs, w.C
    (c, d), g = w.planes, np.nan_to_num(w.gout[0], nan=0.5)
    dg, gin, gp = dev(g), filled(d.shape), torch.zeros((w.n, w.T, 3, 3), dtype=torch.float32, device="cuda")
    fs.antialias_grad(w.vis.data_ptr(), d.data_ptr(), dg.data_ptr(), C, gin.data_ptr(), w.T, gp.data_ptr(), F, stream())
    torch.cuda.synchronize()
    accs = [antialiasref.Grad(w.T) for _ in range(w.n)]
    want = [antialiasref.backward(tmp, w.pos[i], w.n_tris[i], w.v[i], c[i], g[i], accs[i]) for i in range(w.n)]
    same(words(gin), np.stack(want), "gin")
    got = gp.cpu().numpy()
    check_sum(got, np.stack([x.gpos for x in accs]), np.stack([x.gabs for x in accs]), np.stack([x.count for x in accs]), "antialias gpos")
    assert (got[..., 2] == 0).all()


def run_texture(tmp, w, fused, mode=texref.CLAMP):
    fs, C = w.fs, w.C
    (uv, _, uvw, _), (t, t_dev, _, _) = w.uv, w.tex
    out = filled(w.shape(C))
    fs.texture(w.vis.data_ptr(), uv.data_ptr(), t_dev.data_ptr(), TEX_W, TEX_H, C, 1, mode, out.data_ptr(), fs.interpolate_bytes(C),
               F if fused else 0, stream())
    torch.cuda.synchronize()
    got = words(out)
    same(got, np.stack([texref.forward(tmp, t, mode, w.n_tris[i], w.v[i, 1], uvw[i], fused, pre(w, C)) for i in range(w.n)]), "texture")
    check_nobody(w, got, fused, "texture")


def run_texture_grad(tmp, w, fused, mode=texref.WRAP):  # (CLAMP would add every uv beyond 1 into one texel)
    fs, C = w.fs, w.C
    (uv, _, uvw, _), (t, t_dev, _, _), (gout, g) = w.uv, w.tex, w.gout
    gt, gu = torch.zeros_like(t_dev), filled(w.shape(2))
    fs.texture_grad(w.vis.data_ptr(), uv.data_ptr(), g.data_ptr(), t_dev.data_ptr(), TEX_W, TEX_H, C, 1, mode, gt.data_ptr(), gu.data_ptr(),
                    F if fused else 0, stream())
    torch.cuda.synchronize()
    acc = texref.Grad(t.shape)
    want = [texref.grad(tmp, t, mode, w.n_tris[i], w.v[i, 1], uvw[i], gout[i], acc, True, fused, pre(w, 2)) for i in range(w.n)]
    got = words(gu)
    same(got, np.stack(want), "guv")
    check_nobody(w, got, fused, "guv")
    check_sum(gt.cpu().numpy(), acc.gtex, acc.gabs, acc.count[:, :, None], "gtex")


def run_interpolate_deriv(tmp, w, fused):
    fs, C = w.fs, w.C
    a, out = dev(w.attr), filled(w.shape(2 * C))
    fs.interpolate_deriv(w.vis.data_ptr(), a.data_ptr(), C, w.n, w.T, out.data_ptr(), fs.interpolate_bytes(2 * C), F if fused else 0, stream())
    torch.cuda.synchronize()
    got = words(out)
    same(got, np.stack([mipref.deriv(tmp, w.attr[i], w.pos[i], w.n_tris[i], w.v[i, 1], fused, pre(w, 2 * C)) for i in range(w.n)]), "deriv")
    check_nobody(w, got, fused, "deriv")


def run_texture_mip(tmp, w, fused, mode=mipref.CLAMP):
    fs, C = w.fs, w.C
    (uv, uvd, uvw, uvdw), (t, t_dev, L, mip) = w.uv, w.tex
    out = filled(w.shape(C))
    fs.texture_mip(w.vis.data_ptr(), uv.data_ptr(), uvd.data_ptr(), t_dev.data_ptr(), TEX_W, TEX_H, C, 1, mode, mip.data_ptr(), L, out.data_ptr(),
                   fs.interpolate_bytes(C), F if fused else 0, stream())
    torch.cuda.synchronize()
    ref_mip = mipref.build(tmp, t, L)
    l0, _ = mipref.lod(tmp, (TEX_H, TEX_W), L, np.moveaxis(uvdw, 1, 0)[:, w.own])
    assert (l0 == 0).any() and (l0 > 0).any()  # magnified and minified pixels
    got = words(out)
    same(got, np.stack([mipref.forward(tmp, t, ref_mip, mode, L, w.n_tris[i], w.v[i, 1], uvw[i], uvdw[i], fused, pre(w, C)) for i in range(w.n)]),
         "texture_mip")
    check_nobody(w, got, fused, "texture_mip")


def run_texture_mip_grad(tmp, w, fused, mode=mipref.WRAP):
    import srz
    fs, C = w.fs, w.C
    (uv, uvd, uvw, uvdw), (t, t_dev, L, mip), (gout, g) = w.uv, w.tex, w.gout
    gt, gu = torch.zeros_like(t_dev), filled(w.shape(2))
    gm = torch.zeros((srz.mip_bytes(TEX_W, TEX_H, C, 1, L) // 4,), dtype=torch.float32, device="cuda")
    fs.texture_mip_grad(w.vis.data_ptr(), uv.data_ptr(), uvd.data_ptr(), g.data_ptr(), t_dev.data_ptr(), mip.data_ptr(), TEX_W, TEX_H, C, 1, mode, L,
                        gt.data_ptr(), gm.data_ptr(), gu.data_ptr(), F if fused else 0, stream())
    torch.cuda.synchronize()
    ref_mip, acc = mipref.build(tmp, t, L), mipref.Grad(tmp, t.shape, L)
    want = [mipref.grad(tmp, t, ref_mip, mode, L, w.n_tris[i], w.v[i, 1], uvw[i], uvdw[i], gout[i], acc, True, fused, pre(w, 2)) for i in range(w.n)]
    got = words(gu)
    same(got, np.stack(want), "mip guv")
    check_nobody(w, got, fused, "mip guv")
    levels = [gt.cpu().numpy()] + mipref.views(tmp, gm.cpu().numpy(), t.shape, L)
    for l in range(L):
        ref, mag, cnt = acc.level(l)
        if cnt.any():
            check_sum(levels[l], ref, mag, cnt[:, :, None], f"gtex level {l}")
        else:
            assert (levels[l] == 0).all()
    assert acc.level(0)[2].any() and acc.level(1)[2].any()


# pass → (its run, whether it has SRZ_FUSED_CLEAR's two behaviours)
PASSES = {"shade_visibility": (run_shade_visibility, True), "gbuffer": (run_gbuffer, True), "motion": (run_motion, True),
          "interpolate": (run_interpolate, True), "interpolate_grad": (run_interpolate_grad, True), "position_grad": (run_position_grad, True),
          "antialias": (run_antialias, False), "antialias_grad": (run_antialias_grad, False), "texture": (run_texture, True),
          "texture_grad": (run_texture_grad, True), "interpolate_deriv": (run_interpolate_deriv, True), "texture_mip": (run_texture_mip, True),
          "texture_mip_grad": (run_texture_mip_grad, True)}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", list(PASSES))
def test_more_tiles_than_workgroups(worlds, tmp_path, name, shape):
    """(many: with and without the fused clear; large: without it, the stricter of the two — nobody's words must survive)"""
    run, has_fused = PASSES[name]
    w = worlds(shape)
    for fused in ((False, True) if has_fused and shape == "many" else (False,)):
        run(tmp_path, w, fused)
