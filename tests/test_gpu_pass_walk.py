"""-m gpu: the tile walk of the passes over a visibility buffer, beyond the grid's cap.  tile_grid (csrc/srz_kernels.hip) launches at
most 16,384 workgroups, so a set of more tiles sends workgroups round the walk's loop a second time — with whatever they carry from
one tile to the next (the LDS tables of the gradient kernels, k_pos_grad's alternating slot counter, k_tex_mip_grad's rotating level
word).  No other test has that many tiles.  Two shapes, every pass on both:
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
import functools

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
from srz import abi
from support import SENTINEL, ccw, ctx, filled, frame, frame_positions, padded_positions, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
CAP = 16384  # tile_grid's cap on the workgroups of a pass
ZS = np.float32([1, 2, 3, 4])
U = 2.0 ** -24
BACK_UV = ((0.1, 0.2), (0.9, 0.3), (0.4, 0.95))
TEX_W, TEX_H = 16, 16
SHAPES = ("many", "large")
CHANNELS = {"many": 5, "large": 2}  # (many: a full register chunk of channels and a tail)
UV_SCALE = {"many": 3.0, "large": 60.0}  # (both reach the levels above 0 of a 16 x 16 texture)


def many_frames():
    """a soup of five small triangles in front of a triangle that covers the lower right of the frame (the partial column, the
    partial band and the corner tile) and leaves the upper left to the soup and to nobody; soup and shift differ from frame to frame"""
    out = []
    for i in range(6144):
        back = ccw((44, 41), (-16, 41), (44, -19), z=80.0, uv=BACK_UV)
        back["pos"][:, :, :2] += np.float32([i % 7 - 3, i // 7 % 5 - 2])
        out.append(frame(np.concatenate([soup(i, 5, 36, 33, ZS), back]), 36, 33, flags=0))
    return out


def large_frames():
    """a soup of ten triangles some hundred pixels across in front of a triangle that covers the frame but its upper left corner"""
    out = []
    for i in range(7):
        t = soup(i, 10, 98, 98, ZS, big=True)
        t["pos"][:, :, :2] *= np.float32(16)
        back = ccw((1576, 1576), (-424 + 16 * i, 1576), (1576, -424 - 16 * i), z=80.0, uv=BACK_UV)
        out.append(frame(np.concatenate([t, back]), 1568, 1568, flags=0))
    return out


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


class World:
    """one shape's set with everything the passes read, each thing made once on first use"""

    def __init__(self, ctx, name):
        self.ctx, self.name, self.C = ctx, name, CHANNELS[name]
        self.frames = many_frames() if name == "many" else large_frames()
        self.n = len(self.frames)
        self.fs = ctx.frameset(self.frames)
        w, h = self.fs.width, self.fs.height
        tiles = self.n * ((w + 31) // 32) * ((h + 31) // 32)
        assert tiles > CAP and (name != "many" or tiles >= 1.25 * CAP), tiles
        self.vis = visibility(self.fs)
        self.v = words(self.vis)
        self.n_tris = [f.n_tris for f in self.frames]
        self.T = max(self.n_tris)
        self.own = ((self.v[:, 1] & np.uint32(0x7fffffff)) - np.uint32(1)) < np.uint32(self.n_tris)[:, None, None]
        # owners and nobody's pixels exist in (nearly) every frame; many: in each of the four kinds of tile
        per = lambda m: m.reshape(self.n, -1).any(1)  # noqa: E731
        parts = [self.own, ~self.own]
        if name == "many":
            parts += [self.own[:, :32, :32], self.own[:, :32, 32:], self.own[:, 32:, :32], self.own[:, 32:, 32:]]
        assert all(per(m).mean() >= 0.9 for m in parts), [per(m).mean() for m in parts]
        some = range(0, self.n, max(1, self.n // 64))
        assert len({self.v[i, 1].tobytes() for i in some}) >= 0.9 * len(some)  # the frames differ (a culled soup leaves the shift alone)

    def rng(self, salt):
        return np.random.default_rng([salt, self.n])

    def shape(self, n_ch):
        return self.fs.interpolate_shape(n_ch)

    @functools.cached_property
    def pos(self):
        return padded_positions(self.frames, self.T)

    @functools.cached_property
    def attr(self):
        return self.rng(1).normal(0, 3, (self.n, self.T, 3, self.C)).astype(np.float32)

    @functools.cached_property
    def gout(self):
        """[n, C, rows, W] float32, NaN at nobody's pixels (their words may hold anything), and its copy on the device"""
        g = self.rng(2).normal(0, 2, self.shape(self.C)).astype(np.float32)
        g[np.broadcast_to(~self.own[:, None], g.shape)] = np.nan
        return g, dev(g)

    @functools.cached_property
    def planes(self):
        """antialias's input planes [n, C, rows, W] float32 and their copy on the device"""
        c = self.rng(3).normal(0, 1, self.shape(self.C)).astype(np.float32)
        return c, dev(c)

    @functools.cached_property
    def uv(self):
        """the GPU's interpolate and interpolate_deriv of the frames' own uv, scaled → (uv [n, 2, rows, W], uvd [n, 4, rows, W]) on
        the device and as float32 arrays"""
        a = np.zeros((self.n, self.T, 3, 2), np.float32)
        for i, f in enumerate(self.frames):
            a[i, :f.n_tris] = texref.frame_uv(f) * np.float32(UV_SCALE[self.name])
        a_dev, fs = dev(a), self.fs
        uv, uvd = torch.zeros(self.shape(2), dtype=torch.float32, device="cuda"), torch.zeros(self.shape(4), dtype=torch.float32, device="cuda")
        fs.interpolate(self.vis.data_ptr(), a_dev.data_ptr(), 2, self.n, self.T, uv.data_ptr(), fs.interpolate_bytes(2), F, stream())
        fs.interpolate_deriv(self.vis.data_ptr(), a_dev.data_ptr(), 2, self.n, self.T, uvd.data_ptr(), fs.interpolate_bytes(4), F, stream())
        torch.cuda.synchronize()
        return uv, uvd, uv.cpu().numpy(), uvd.cpu().numpy()

    @functools.cached_property
    def tex(self):
        """one texture for every frame [h, w, C], its copy on the device, the level count and the GPU's pyramid"""
        import srz
        t = texref.make_tex(3, TEX_W, TEX_H, self.C)
        L = srz.mip_levels(TEX_W, TEX_H)
        nbytes = srz.mip_bytes(TEX_W, TEX_H, self.C, 1, L)
        t_dev, mip = dev(t), torch.zeros((nbytes // 4,), dtype=torch.float32, device="cuda")
        self.ctx.mip_build(t_dev.data_ptr(), TEX_W, TEX_H, self.C, 1, L, mip.data_ptr(), nbytes, stream())
        torch.cuda.synchronize()
        assert L > 1
        return t, t_dev, L, mip


@pytest.fixture(scope="module")
def worlds(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = World(ctx, name)
        return made[name]
    yield get
    for w in made.values():
        w.fs.close()


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def check_sum(got, ref, mag, cnt, what):
    """a float-atomic sum against the reference's double: ref the sums, mag the sums of |term|, cnt the terms per element"""
    got, cnt = got.reshape(ref.shape), np.broadcast_to(cnt, ref.shape).astype(np.float64)
    assert np.isfinite(ref).all() and (cnt > 1).any(), what
    nu = cnt * U
    assert nu.max() < 1.0, (what, cnt.max())  # (the bound's domain)
    bound = nu / (1.0 - nu) * mag
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{what}: max err {err.max():.3e}, max err / bound {np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0:.3f}, "
          f"max n {int(cnt.max())}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    one = cnt == 1
    same((got + np.float32(0))[one], (ref.astype(np.float32) + np.float32(0))[one], what + " (n = 1)")
    assert (got[cnt == 0] == 0).all(), what


def check_nobody(w, got, fused, what):
    """nobody's words: zeros with the fused clear, else the sentinel the buffer started from"""
    nobody = np.broadcast_to(~w.own[:len(got), None], got.shape)
    assert (got[nobody] == (0 if fused else SENTINEL)).all() and (got[~nobody] != SENTINEL).any(), what


def pre(w, n_planes):
    return np.full((n_planes,) + w.v.shape[2:], SENTINEL, np.uint32)


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
