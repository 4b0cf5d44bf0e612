"""-m gpu: the passes over a visibility buffer on band shards, held to their whole-frame words.  include/srz.h promises of every pass
that it works on a shard: a rank holds the 32-row bands THE BAND MAP (srz_set_shard) gives it, band band_of(lb, rank, world) at local
band lb.  The passes' own shard tests run four full bands on two ranks, or one band on one rank; here every pass runs on
tests/shardkit.py's two frame sizes — 72 x 197 (16-byte quads) and 70 x 197 (W % 4 == 2: scalar accesses), seven bands, the last one
five rows — under three layouts: world 3 (rotation 5: a rank's second band is not band 3 + rank; rank 1 has the ragged band at local
band 2, ranks 0 and 2 are a local band short), world 5 (rotation 1; the ragged band at local band 1 of rank 2) and ranks 6 and 7 of
world 8 (the ragged band alone; no band at all).  One process plays every rank, each with a context of its own.

Per pass and geometry (shardkit.hold_pass): the unsharded call is held to the pass's own reference (tests/*ref.py on the device's
visibility words, as the pass's own test calls it) — the planes word for word (a NaN for a NaN), the float-atomic sums within
gamma_n * sum |term|, gamma_n = n u / (1 - n u), u = 2^-24, bit for bit at n = 1 and exactly 0 at n = 0.  Then every rank is given
its rows of the whole-frame inputs — NaN in every float plane outside its bands, the sentinel in the id plane there and in every
output — and its planes must be the whole frame's rows word for word, every word outside its bands untouched, with and without
SRZ_FUSED_CLEAR.  A rank's sums are held to the reference run on the whole frame with the other ranks' rows written to nobody — its
own counts, its own bound —, and the float64 sum of the ranks of worlds 3 and 5 to the whole frame's reference within the whole
frame's bound.  Before any sum is checked the reference alone shows that a band matters: on 90 % of the touched elements the
smallest share a band has in the element is above four times its bound (walkkit.teeth over the bands).  Textures are 8 x 8 and the
cubes' faces 4 x 4, so that rows of different bands land on common texels.  Inputs with a shape of their own (attributes, q, textures,
cubes, maps) are whole and the same on every rank.  gbuffer runs every one of its fifteen masks (one to nine planes: the frame stride of
the output differs), perspective with and without the flag it ignores.  On the rank without a band the float-atomic outputs start from
shardkit.ACC_FILL, not from zeros, and must hold exactly that afterwards."""
import numpy as np
import pytest
import torch

import cubemipref
import cuberef
import gbufref
import interpref
import mipref
import motionref
import perspref
import posgradref
import shadowref
import shardkit
import texref
from shardkit import GEOMETRIES, hold_pass, owner_pass
from srz import abi
from support import SENTINEL, ctx, filled, frame_positions, stream, words  # noqa: F401
from walkkit import dev

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
C = 5  # interpolate, its gradient and the textures: a full register chunk of channels and a tail; the derivatives take 3, shadow 1
TEX = 8
CUBE_N = 4
MAP = 8
BIAS, WIDTH = 0.375, 5.0  # tests/test_gpu_shadow.py's
UV_SCALE = 12.0  # the frame repeats the texture a dozen times: every band reaches every texel, and levels 0 .. 3 are met
INF = 0x7f800000


@pytest.fixture(scope="module")
def geos(ctx):
    yield from shardkit.make_geos(ctx)


def fl(fused):
    return F if fused else 0


def pre(g, k):
    return np.full((k, g.H, g.W), SENTINEL, np.uint32)


def done(**outs):
    torch.cuda.synchronize()
    return {k: words(t) for k, t in outs.items()}


# ------------------------------------------------------------------------------------------------------ inputs, once per geometry
def attr_of(g):
    return g.memo("attr", lambda g: g.rng(1).normal(0, 3, (g.n, g.T, 3, C)).astype(np.float32))


def gout_of(g):
    """[n, C, H, W], NaN at nobody's pixels: their words may hold anything"""
    return g.memo("gout", lambda g: g.planes(2, C, 2.0, nan=~g.own))


def q_of(g):
    def make(g):
        rng = g.rng(13)
        return (rng.uniform(0.25, 4.0, (g.n, g.T, 3)) * 2.0 ** rng.integers(-3, 4, (g.n, g.T, 1))).astype(np.float32)
    return g.memo("q", make)


def interpolated(g, a, deriv=False):
    """the GPU's own interpolate (deriv: interpolate_deriv) of the attributes a [n, T, 3, k] over the whole frame, NaN at nobody's"""
    k, fs = a.shape[-1], g.fs
    planes = 2 * k if deriv else k
    a_dev, out = dev(a), torch.zeros(fs.interpolate_shape(planes), dtype=torch.float32, device="cuda")
    (fs.interpolate_deriv if deriv else fs.interpolate)(g.vis.data_ptr(), a_dev.data_ptr(), k, g.n, g.T, out.data_ptr(),
                                                       fs.interpolate_bytes(planes), F, stream())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    o[np.broadcast_to(~g.own[:, None], o.shape)] = np.nan
    return o


def uv_of(g):
    """(uv [n, 2, H, W], uvd [n, 4, H, W]): the frames' own uv, scaled so that the levels above 0 of an 8 x 8 texture are reached"""
    def make(g):
        a = np.zeros((g.n, g.T, 3, 2), np.float32)
        for i, f in enumerate(g.frames):
            a[i, :f.n_tris] = texref.frame_uv(f) * np.float32(UV_SCALE)
        return interpolated(g, a), interpolated(g, a, deriv=True)
    return g.memo("uv", make)


def tex_of(g):
    """(one 8 x 8 texture of C channels for every frame, its copy on the device, the level count, the GPU's pyramid)"""
    def make(g):
        import srz
        t = texref.make_tex(3, TEX, TEX, C)
        L = srz.mip_levels(TEX, TEX)
        nbytes = srz.mip_bytes(TEX, TEX, C, 1, L)
        t_dev, mip = dev(t), torch.zeros((nbytes // 4,), dtype=torch.float32, device="cuda")
        g.whole.ctx.mip_build(t_dev.data_ptr(), TEX, TEX, C, 1, L, mip.data_ptr(), nbytes, stream())
        torch.cuda.synchronize()
        assert L > 1
        return t, t_dev, L, mip
    return g.memo("tex", make)


def dirs_of(g):
    """(dirs [n, 3, H, W], dird [n, 6, H, W]) from seeded attributes"""
    def make(g):
        a = g.rng(11).normal(0, 1, (g.n, g.T, 3, 3)).astype(np.float32)
        return interpolated(g, a), interpolated(g, a, deriv=True)
    return g.memo("dirs", make)


def cube_of(g):
    """one 4 x 4 cube of C channels per frame → (levels, the cube on the device, the levels above 0 on the device)"""
    def make(g):
        cube = cuberef.make_cube(21, CUBE_N, C, frames=g.n)
        levels = cubemipref.build(cube)
        assert len(levels) > 1
        return levels, dev(cube), dev(cubemipref.flat(levels, 1))
    return g.memo("cube", make)


def lam_of(g):
    def make(g):
        L = len(cube_of(g)[0])
        lam = g.rng(12).uniform(-0.5, L - 0.5, (g.n, 1, g.H, g.W)).astype(np.float32)
        lam[np.broadcast_to(~g.own[:, None], lam.shape)] = np.nan
        return lam
    return g.memo("lam", make)


def shadow_of(g):
    """(one 8 x 8 map per frame, its copy on the device, sc [n, 3, H, W])"""
    def make(g):
        depth = shadowref.make_map(31, MAP, MAP, frames=g.n)
        sc = np.ascontiguousarray(shadowref.make_coords(32, (g.n, g.H, g.W), MAP, MAP).transpose(1, 0, 2, 3), np.float32)
        sc[np.broadcast_to(~g.own[:, None], sc.shape)] = np.nan
        return depth, dev(depth), sc
    return g.memo("shadow", make)


# ------------------------------------------------------------------------------------------------------ the passes
# run_*(tmp, g, S, fused) → (planes, sums) of the call on the Shard S; ref_*(tmp, g, v, fused) → the reference's on the words v
def run_shade_visibility(tmp, g, S, fused):
    """into z +inf (the frames do not clear: a render tests against it) and the sentinel in the colour planes"""
    out = filled((g.n, 4, S.local_rows, g.W)).view(torch.float32)
    out[:, 0] = float("inf")
    S.fs.shade_visibility(S.vis_in.data_ptr(), out.data_ptr(), S.fs.out_bytes, fl(fused), stream())
    w = done(out=out)["out"]
    return {"z": (w[:, :1], INF), "colour": w[:, 1:]}, {}


def ref_shade_visibility(tmp, g, v, fused):
    """the set's own colour render into the same prefill (pinned to the oracle by tests/test_gpu_shade_visibility.py)"""
    col = filled(g.fs.out_shape).view(torch.float32)
    col[:, 0] = float("inf")
    g.fs.render(col.data_ptr(), g.fs.out_bytes, fl(fused), stream())
    torch.cuda.synchronize()
    w = words(col)
    nobody = np.broadcast_to(~g.own[:, None], w[:, 1:].shape)
    assert (w[:, 1:][nobody] == (0 if fused else SENTINEL)).all()
    return {"z": w[:, :1], "colour": w[:, 1:]}, {}


GB_MASKS = tuple(range(1, abi.GB_ALL + 1))  # every mask, as tests/test_gpu_gbuffer.py walks them: 1 .. 9 planes, each its own frame stride


def run_gbuffer(tmp, g, S, fused):
    outs = {}
    for what in GB_MASKS:
        k = S.fs.gbuffer_shape(what)[1]
        outs[f"mask {what}"] = S.out(k)
        assert tuple(S.fs.gbuffer_shape(what)) == (g.n, k, S.local_rows, g.W)
        S.fs.gbuffer(S.vis_in.data_ptr(), outs[f"mask {what}"].data_ptr(), S.fs.gbuffer_bytes(what), what, fl(fused), stream())
    return done(**outs), {}


def ref_gbuffer(tmp, g, v, fused):
    full = np.stack([gbufref.expected(tmp, f, {}, v[i], fused, pre(g, 9)) for i, f in enumerate(g.frames)])
    return {f"mask {what}": full[:, gbufref.planes_of(what)] for what in GB_MASKS}, {}


MV = abi.MV_FLOW | abi.MV_DEPTH


def run_motion(tmp, g, S, fused):
    out = S.out(3)
    S.fs.motion(S.vis_in.data_ptr(), out.data_ptr(), S.fs.motion_bytes(MV), MV, 1, fl(fused), stream())
    return done(flow_depth=out), {}


def ref_motion(tmp, g, v, fused):
    want = [motionref.expected(tmp, frame_positions(g.frames[i + 1]), v[i], v[i + 1], fused, pre(g, 5)) for i in range(g.n - 1)]
    want.append(motionref.nobody((g.H, g.W), fused, SENTINEL))  # (the last frame has no target frame)
    return {"flow_depth": np.stack(want)[:, motionref.planes_of(MV)]}, {}


def run_interpolate(tmp, g, S, fused):
    a, out = dev(attr_of(g)), S.out(C)
    S.fs.interpolate(S.vis_in.data_ptr(), a.data_ptr(), C, g.n, g.T, out.data_ptr(), S.fs.interpolate_bytes(C), fl(fused), stream())
    return done(out=out), {}


def ref_interpolate(tmp, g, v, fused):
    a = attr_of(g)
    return {"out": np.stack([interpref.forward(tmp, a[i], g.n_tris[i], v[i], fused, pre(g, C)) for i in range(g.n)])}, {}


def run_interpolate_grad(tmp, g, S, fused):
    a, go = dev(attr_of(g)), S.dev(gout_of(g))
    ga, gb = S.acc(a.shape), S.out(2)
    S.fs.interpolate_grad(S.vis_in.data_ptr(), go.data_ptr(), a.data_ptr(), C, g.n, g.T, ga.data_ptr(), gb.data_ptr(), fl(fused), stream())
    return done(gbary=gb), {"gattr": ga.cpu().numpy()}


def ref_interpolate_grad(tmp, g, v, fused):
    a, go = attr_of(g), gout_of(g)
    accs = [interpref.Grad(a.shape[1:]) for _ in range(g.n)]
    gb = [interpref.grad(tmp, a[i], g.n_tris[i], v[i], go[i], accs[i], True, fused, pre(g, 2)) for i in range(g.n)]
    return {"gbary": np.stack(gb)}, {"gattr": (np.stack([x.gattr for x in accs]), np.stack([x.gabs for x in accs]),
                                               np.stack([x.count for x in accs])[:, :, None, None], 0)}


def run_interpolate_deriv(tmp, g, S, fused):
    a, out = dev(attr_of(g)[..., :3]), S.out(6)
    S.fs.interpolate_deriv(S.vis_in.data_ptr(), a.data_ptr(), 3, g.n, g.T, out.data_ptr(), S.fs.interpolate_bytes(6), fl(fused), stream())
    return done(deriv=out), {}


def ref_interpolate_deriv(tmp, g, v, fused):
    a = np.ascontiguousarray(attr_of(g)[..., :3])
    return {"deriv": np.stack([mipref.deriv(tmp, a[i], g.pos[i], g.n_tris[i], v[i, 1], fused, pre(g, 6)) for i in range(g.n)])}, {}


def run_position_grad(tmp, g, S, fused):
    go = gout_of(g)
    gb, gz = S.dev(go[:, :2]), S.dev(go[:, 2:3])
    gp, gx = S.acc((g.n, g.T, 3, 3)), S.out(2)
    S.fs.position_grad(S.vis_in.data_ptr(), gb.data_ptr(), gz.data_ptr(), g.T, gp.data_ptr(), gx.data_ptr(), fl(fused), stream())
    return done(gpix=gx), {"gpos": gp.cpu().numpy()}


def ref_position_grad(tmp, g, v, fused):
    go = gout_of(g)
    accs = [posgradref.Grad(g.T) for _ in range(g.n)]
    gx = [posgradref.grad(tmp, g.pos[i], g.n_tris[i], v[i], go[i, :2], go[i, 2:3], accs[i], True, fused, pre(g, 2)) for i in range(g.n)]
    return {"gpix": np.stack(gx)}, {"gpos": (np.stack([x.gpos for x in accs]), np.stack([x.gabs for x in accs]),
                                             np.stack([x.count for x in accs])[:, :, None, None], 0)}


def run_perspective(tmp, g, S, fused):
    qd, out = dev(q_of(g)), S.out(4)
    S.fs.perspective(S.vis_in.data_ptr(), qd.data_ptr(), g.n, g.T, out.data_ptr(), S.fs.out_bytes, fl(fused), stream())
    return done(out=out), {}


def ref_perspective(tmp, g, v, fused):
    q = q_of(g)
    return {"out": np.stack([perspref.forward(tmp, q[i], g.n_tris[i], v[i]) for i in range(g.n)])}, {}  # (every word is written)


def run_perspective_grad(tmp, g, S, fused):
    qd, gbp = dev(q_of(g)), S.dev(gout_of(g)[:, :2])
    gq, gb = S.acc(qd.shape), S.out(2)
    S.fs.perspective_grad(S.vis_in.data_ptr(), qd.data_ptr(), g.n, g.T, gbp.data_ptr(), gb.data_ptr(), gq.data_ptr(), fl(fused), stream())
    return done(gbary=gb), {"gq": gq.cpu().numpy()}


def ref_perspective_grad(tmp, g, v, fused):
    q, go = q_of(g), gout_of(g)
    accs = [perspref.Grad(q.shape[1:]) for _ in range(g.n)]
    gb = [perspref.grad(tmp, q[i], g.n_tris[i], v[i], go[i, :2], accs[i], True, fused, pre(g, 2)) for i in range(g.n)]
    return {"gbary": np.stack(gb)}, {"gq": (np.stack([x.gq for x in accs]), np.stack([x.gabs for x in accs]),
                                            np.stack([x.count for x in accs])[:, :, None], 0)}


def run_interpolate_deriv_persp(tmp, g, S, fused):
    qd, a, out = dev(q_of(g)), dev(attr_of(g)[..., :3]), S.out(6)
    S.fs.interpolate_deriv_persp(S.vis_in.data_ptr(), qd.data_ptr(), g.n, g.T, a.data_ptr(), 3, g.n, g.T, out.data_ptr(),
                                 S.fs.interpolate_bytes(6), fl(fused), stream())
    return done(deriv=out), {}


def ref_interpolate_deriv_persp(tmp, g, v, fused):
    q, a = q_of(g), np.ascontiguousarray(attr_of(g)[..., :3])
    return {"deriv": np.stack([perspref.deriv(tmp, q[i], g.pos[i], a[i], g.n_tris[i], v[i], fused, pre(g, 6)) for i in range(g.n)])}, {}


def run_texture(tmp, g, S, fused, mode=texref.CLAMP):
    uv, (_, t_dev, _, _), out = S.dev(uv_of(g)[0]), tex_of(g), S.out(C)
    S.fs.texture(S.vis_in.data_ptr(), uv.data_ptr(), t_dev.data_ptr(), TEX, TEX, C, 1, mode, out.data_ptr(), S.fs.interpolate_bytes(C), fl(fused),
                 stream())
    return done(out=out), {}


def ref_texture(tmp, g, v, fused, mode=texref.CLAMP):
    uv, t = uv_of(g)[0], tex_of(g)[0]
    return {"out": np.stack([texref.forward(tmp, t, mode, g.n_tris[i], v[i, 1], uv[i], fused, pre(g, C)) for i in range(g.n)])}, {}


def run_texture_grad(tmp, g, S, fused, mode=texref.WRAP):  # (CLAMP would add every uv beyond 1 into one texel)
    uv, (_, t_dev, _, _), go = S.dev(uv_of(g)[0]), tex_of(g), S.dev(gout_of(g))
    gt, gu = S.acc(t_dev.shape), S.out(2)
    S.fs.texture_grad(S.vis_in.data_ptr(), uv.data_ptr(), go.data_ptr(), t_dev.data_ptr(), TEX, TEX, C, 1, mode, gt.data_ptr(), gu.data_ptr(),
                      fl(fused), stream())
    return done(guv=gu), {"gtex": gt.cpu().numpy()}


def ref_texture_grad(tmp, g, v, fused, mode=texref.WRAP):
    uv, t, go = uv_of(g)[0], tex_of(g)[0], gout_of(g)
    acc = texref.Grad(t.shape)
    gu = [texref.grad(tmp, t, mode, g.n_tris[i], v[i, 1], uv[i], go[i], acc, True, fused, pre(g, 2)) for i in range(g.n)]
    return {"guv": np.stack(gu)}, {"gtex": (acc.gtex, acc.gabs, acc.count[:, :, None], 0)}


def run_texture_mip(tmp, g, S, fused, mode=mipref.CLAMP):
    (uvw, uvdw), (_, t_dev, L, mip), out = uv_of(g), tex_of(g), S.out(C)
    uv, uvd = S.dev(uvw), S.dev(uvdw)
    S.fs.texture_mip(S.vis_in.data_ptr(), uv.data_ptr(), uvd.data_ptr(), t_dev.data_ptr(), TEX, TEX, C, 1, mode, mip.data_ptr(), L, out.data_ptr(),
                     S.fs.interpolate_bytes(C), fl(fused), stream())
    return done(out=out), {}


def ref_texture_mip(tmp, g, v, fused, mode=mipref.CLAMP):
    (uv, uvd), (t, _, L, _) = uv_of(g), tex_of(g)
    ref_mip = mipref.build(tmp, t, L)
    l0, _ = mipref.lod(tmp, (TEX, TEX), L, np.moveaxis(uvd, 1, 0)[:, g.own])
    assert (l0 == 0).any() and (l0 > 0).any()  # magnified and minified pixels
    return {"out": np.stack([mipref.forward(tmp, t, ref_mip, mode, L, g.n_tris[i], v[i, 1], uv[i], uvd[i], fused, pre(g, C))
                             for i in range(g.n)])}, {}


def run_texture_mip_grad(tmp, g, S, fused, mode=mipref.WRAP):
    import srz
    (uvw, uvdw), (t, t_dev, L, mip), go = uv_of(g), tex_of(g), S.dev(gout_of(g))
    uv, uvd = S.dev(uvw), S.dev(uvdw)
    gt, gu = S.acc(t_dev.shape), S.out(2)
    gm = S.acc((srz.mip_bytes(TEX, TEX, C, 1, L) // 4,))
    S.fs.texture_mip_grad(S.vis_in.data_ptr(), uv.data_ptr(), uvd.data_ptr(), go.data_ptr(), t_dev.data_ptr(), mip.data_ptr(), TEX, TEX, C, 1, mode, L,
                          gt.data_ptr(), gm.data_ptr(), gu.data_ptr(), fl(fused), stream())
    planes = done(guv=gu)
    levels = [gt.cpu().numpy()] + mipref.views(tmp, gm.cpu().numpy(), t.shape, L)
    return planes, {f"gtex level {l}": np.ascontiguousarray(levels[l]) for l in range(L)}


def ref_texture_mip_grad(tmp, g, v, fused, mode=mipref.WRAP):
    (uv, uvd), (t, _, L, _), go = uv_of(g), tex_of(g), gout_of(g)
    ref_mip, acc = mipref.build(tmp, t, L), mipref.Grad(tmp, t.shape, L)
    gu = [mipref.grad(tmp, t, ref_mip, mode, L, g.n_tris[i], v[i, 1], uv[i], uvd[i], go[i], acc, True, fused, pre(g, 2)) for i in range(g.n)]
    sums = {}
    for l in range(L):
        r, mag, cnt = acc.level(l)
        sums[f"gtex level {l}"] = (r, mag, cnt[:, :, None], 0)
    return {"guv": np.stack(gu)}, sums


def run_texture_cube(tmp, g, S, fused):
    d, (_, t, _), out = S.dev(dirs_of(g)[0]), cube_of(g), S.out(C)
    S.fs.texture_cube(S.vis_in.data_ptr(), d.data_ptr(), t.data_ptr(), CUBE_N, C, g.n, out.data_ptr(), S.fs.interpolate_bytes(C), fl(fused), stream())
    return done(out=out), {}


def ref_texture_cube(tmp, g, v, fused):
    d, cube = dirs_of(g)[0], cube_of(g)[0][0]
    return {"out": np.stack([cuberef.forward(tmp, cube[i], g.n_tris[i], v[i, 1], d[i], fused, pre(g, C)) for i in range(g.n)])}, {}


def run_texture_cube_grad(tmp, g, S, fused):
    d, (_, t, _), go = S.dev(dirs_of(g)[0]), cube_of(g), S.dev(gout_of(g))
    gt, gd = S.acc(t.shape), S.out(3)
    S.fs.texture_cube_grad(S.vis_in.data_ptr(), d.data_ptr(), go.data_ptr(), t.data_ptr(), CUBE_N, C, g.n, gt.data_ptr(), gd.data_ptr(), fl(fused),
                           stream())
    return done(gdir=gd), {"gtex": gt.cpu().numpy()}


def ref_texture_cube_grad(tmp, g, v, fused):
    d, cube, go = dirs_of(g)[0], cube_of(g)[0][0], gout_of(g)
    accs = [cuberef.Grad(cube.shape[-4:]) for _ in range(g.n)]
    gd = [cuberef.grad(tmp, cube[i], g.n_tris[i], v[i, 1], d[i], go[i], accs[i], True, fused, pre(g, 3)) for i in range(g.n)]
    return {"gdir": np.stack(gd)}, {"gtex": (np.stack([a.gtex for a in accs]), np.stack([a.gabs for a in accs]),
                                             np.stack([a.count for a in accs])[..., None], 0)}


def run_cube_level(tmp, g, S, fused):
    (dw, ddw), L, out = dirs_of(g), len(cube_of(g)[0]), S.out(1)
    d, dd = S.dev(dw), S.dev(ddw)
    S.fs.cube_level(S.vis_in.data_ptr(), d.data_ptr(), dd.data_ptr(), CUBE_N, L, out.data_ptr(), S.fs.interpolate_bytes(1), fl(fused), stream())
    return done(lam=out), {}


def ref_cube_level(tmp, g, v, fused):
    (d, dd), L = dirs_of(g), len(cube_of(g)[0])
    return {"lam": np.stack([cubemipref.level(tmp, CUBE_N, L, g.n_tris[i], v[i, 1], d[i], dd[i], fused, SENTINEL)[None] for i in range(g.n)])}, {}


def run_texture_cube_mip(tmp, g, S, fused):
    d, lam, (levels, t, mip), out = S.dev(dirs_of(g)[0]), S.dev(lam_of(g)), cube_of(g), S.out(C)
    S.fs.texture_cube_mip(S.vis_in.data_ptr(), d.data_ptr(), lam.data_ptr(), t.data_ptr(), CUBE_N, C, g.n, mip.data_ptr(), len(levels), out.data_ptr(),
                          S.fs.interpolate_bytes(C), fl(fused), stream())
    return done(out=out), {}


def ref_texture_cube_mip(tmp, g, v, fused):
    d, lam, levels = dirs_of(g)[0], lam_of(g), cube_of(g)[0]
    return {"out": np.stack([cubemipref.forward(tmp, [l[i] for l in levels], g.n_tris[i], v[i, 1], d[i], lam[i, 0], fused, pre(g, C))
                             for i in range(g.n)])}, {}


def run_texture_cube_mip_grad(tmp, g, S, fused):
    d, lam, (levels, t, mip), go = S.dev(dirs_of(g)[0]), S.dev(lam_of(g)), cube_of(g), S.dev(gout_of(g))
    gt, gm, gd, gl = S.acc(t.shape), S.acc(mip.shape), S.out(3), S.out(1)
    S.fs.texture_cube_mip_grad(S.vis_in.data_ptr(), d.data_ptr(), lam.data_ptr(), go.data_ptr(), t.data_ptr(), mip.data_ptr(), CUBE_N, C, g.n,
                               len(levels), gt.data_ptr(), gm.data_ptr(), gd.data_ptr(), gl.data_ptr(), fl(fused), stream())
    planes = done(gdir=gd, glam=gl)
    glev, off, flat = [gt.cpu().numpy()], 0, gm.cpu().numpy()
    for l in levels[1:]:
        glev.append(flat[off:off + l.size].reshape(l.shape))
        off += l.size
    return planes, {f"gtex level {l}": glev[l] for l in range(len(levels))}


def ref_texture_cube_mip_grad(tmp, g, v, fused):
    d, lam, levels, go = dirs_of(g)[0], lam_of(g), cube_of(g)[0], gout_of(g)
    accs = [cubemipref.Grad(CUBE_N, C, len(levels)) for _ in range(g.n)]
    want = [cubemipref.grad(tmp, [l[i] for l in levels], g.n_tris[i], v[i, 1], d[i], lam[i, 0], go[i], accs[i], fused=fused, prefill=SENTINEL)
            for i in range(g.n)]
    sums = {f"gtex level {l}": (np.stack([a.level(a.g, l) for a in accs]), np.stack([a.level(a.gabs, l) for a in accs]),
                                np.stack([a.level(a.count, l) for a in accs])[..., None], 0) for l in range(len(levels))}
    return {"gdir": np.stack([a for a, _ in want]), "glam": np.stack([b[None] for _, b in want])}, sums


def run_shadow(tmp, g, S, fused):
    (_, d, scw), out = shadow_of(g), S.out(1)
    sc = S.dev(scw)
    S.fs.shadow(S.vis_in.data_ptr(), sc.data_ptr(), d.data_ptr(), MAP, MAP, g.n, BIAS, WIDTH, out.data_ptr(), S.fs.interpolate_bytes(1), fl(fused),
                stream())
    return done(out=out), {}


def ref_shadow(tmp, g, v, fused):
    depth, _, sc = shadow_of(g)
    return {"out": np.stack([shadowref.forward(tmp, depth[i], g.n_tris[i], v[i, 1], sc[i], BIAS, WIDTH, fused, pre(g, 1)) for i in range(g.n)])}, {}


def run_shadow_grad(tmp, g, S, fused):
    (_, d, scw), go = shadow_of(g), S.dev(gout_of(g)[:, :1])
    sc, gm, gs = S.dev(scw), S.acc(d.shape), S.out(3)
    S.fs.shadow_grad(S.vis_in.data_ptr(), sc.data_ptr(), go.data_ptr(), d.data_ptr(), MAP, MAP, g.n, BIAS, WIDTH, gm.data_ptr(), gs.data_ptr(),
                     fl(fused), stream())
    return done(gsc=gs), {"gmap": gm.cpu().numpy()}


def ref_shadow_grad(tmp, g, v, fused):
    (depth, _, sc), go = shadow_of(g), gout_of(g)
    accs = [shadowref.Grad(depth.shape[-2:]) for _ in range(g.n)]
    gs = [shadowref.grad(tmp, depth[i], g.n_tris[i], v[i, 1], sc[i], go[i, :1], BIAS, WIDTH, accs[i], True, fused, pre(g, 3)) for i in range(g.n)]
    return {"gsc": np.stack(gs)}, {"gmap": (np.stack([a.gmap for a in accs]), np.stack([a.gabs for a in accs]),
                                            np.stack([a.count for a in accs]), 0)}


BOTH = (False, True)  # (perspective writes every word whatever the flags say: its reference is the same for both)
PASSES = {"shade_visibility": (run_shade_visibility, ref_shade_visibility, BOTH), "gbuffer": (run_gbuffer, ref_gbuffer, BOTH),
          "motion": (run_motion, ref_motion, BOTH), "interpolate": (run_interpolate, ref_interpolate, BOTH),
          "interpolate_grad": (run_interpolate_grad, ref_interpolate_grad, BOTH),
          "interpolate_deriv": (run_interpolate_deriv, ref_interpolate_deriv, BOTH),
          "position_grad": (run_position_grad, ref_position_grad, BOTH), "perspective": (run_perspective, ref_perspective, BOTH),
          "perspective_grad": (run_perspective_grad, ref_perspective_grad, BOTH),
          "interpolate_deriv_persp": (run_interpolate_deriv_persp, ref_interpolate_deriv_persp, BOTH),
          "texture": (run_texture, ref_texture, BOTH), "texture_grad": (run_texture_grad, ref_texture_grad, BOTH),
          "texture_mip": (run_texture_mip, ref_texture_mip, BOTH), "texture_mip_grad": (run_texture_mip_grad, ref_texture_mip_grad, BOTH),
          "texture_cube": (run_texture_cube, ref_texture_cube, BOTH), "texture_cube_grad": (run_texture_cube_grad, ref_texture_cube_grad, BOTH),
          "cube_level": (run_cube_level, ref_cube_level, BOTH), "texture_cube_mip": (run_texture_cube_mip, ref_texture_cube_mip, BOTH),
          "texture_cube_mip_grad": (run_texture_cube_mip_grad, ref_texture_cube_mip_grad, BOTH),
          "shadow": (run_shadow, ref_shadow, BOTH), "shadow_grad": (run_shadow_grad, ref_shadow_grad, BOTH)}


@pytest.mark.parametrize("geo", list(GEOMETRIES))
@pytest.mark.parametrize("name", list(PASSES))
def test_every_shard_gives_the_whole_frames_words(geos, tmp_path, name, geo):
    run, ref, fused_options = PASSES[name]
    g = geos(geo)
    if name == "motion":  # the point of this one: rows whose band is not lb * world + rank, at lb >= 1, are among those compared
        assert all(shardkit.rotated_rows(g.H, r, w) > 0 for (w, r) in ((3, 0), (3, 1), (3, 2), (5, 1), (5, 2)))
    hold_pass(tmp_path, g, name, run, owner_pass(ref), fused_options)


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_what_a_shard_refuses_leaves_the_output_untouched(geos, geo):
    """antialias, antialias_grad and SRZ_MV_TARGET need rows of other ranks (tests/test_gpu_antialias.py, tests/test_gpu_motion.py pin
    the refusals); here: on the rank without a band, too, nothing is launched"""
    import srz
    g = geos(geo)
    S, L = g.shard(8, 7), srz.lib()
    planes, gout, out = S.dev(g.planes(3, 3)), S.dev(g.planes(4, 3)), S.out(5)
    gp = torch.full((g.n, g.T, 3, 3), 5.0, dtype=torch.float32, device="cuda")
    v, o, h = S.vis_in.data_ptr(), out.data_ptr(), S.ctx.h
    for what in (abi.MV_TARGET, abi.MV_ALL):
        assert L.srz_frameset_motion(h, S.fs.h, v, o, S.fs.motion_bytes(what), what, 1, F, None) == abi.SRZ_E_INVALID
    with pytest.raises(srz.SrzError):
        S.fs.antialias(v, planes.data_ptr(), 3, o, S.fs.interpolate_bytes(3), F, stream())
    with pytest.raises(srz.SrzError):
        S.fs.antialias_grad(v, planes.data_ptr(), gout.data_ptr(), 3, o, g.T, gp.data_ptr(), F, stream())
    torch.cuda.synchronize()
    assert (words(out) == SENTINEL).all() and (gp == 5.0).all()
