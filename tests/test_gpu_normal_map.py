"""-m gpu: tangent-space normal mapping over a visibility buffer and its gradients (srz_frameset_normal_map / _normal_map_grad,
k_normal_map, k_normal_map_grad) with srz.visibility.normal_map / normal_map_grad.  The visibility buffer is the GPU's own
render_visibility; the planes are written by hand (tangentref.branch_planes: every branch of the rule) or come out of the chain
mesh_tangents -> corner_attr -> interpolate; the expected values are tests/tangentref.py's binary32 build on those very buffers
(pinned on the CPU by tests/test_tangent_ref.py), BIT FOR BIT — both kernels are per pixel, without atomics; a NaN on one side must
be a NaN on the other."""
import numpy as np
import pytest
import torch

import lightref
import tangentref as tr
import texref
import vgkit
from srz import abi, parallel
from srz import visibility as V
from support import SENTINEL, ccw, ctx, filled, frame, scene_pair, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
N_FRAMES = 3
# 64 x 64: whole tiles and aligned quads; 45 x 37: a width that is a multiple of neither 32 nor 4 (no aligned quad, a partial last
# tile column) and a partial last band
SIZES = [(64, 64, 60), (45, 37, 30)]


def n_tris(f):
    return f if isinstance(f, int) else sum(len(t) for t in f.tris)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = tr.same_or_nan(g.view(np.float32), w.view(np.float32))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def owners(v, frames):
    return np.stack([((v[i, 1] & 0x7fffffff) - np.uint32(1)) < n_tris(f) for i, f in enumerate(frames)])


def make_frames(w, h, n, flags=F, k=N_FRAMES):
    """k frames of one soup in front of a backdrop that leaves the far corner free, each shifted: owners, holes and differing buffers"""
    frames = []
    backdrop = ccw((-8, -8), (1.3 * w, -8), (-8, 1.3 * h), z=80.0)
    for i in range(k):
        t = np.concatenate([soup(1, n, w, h, ZS, big=w < 50), backdrop])
        t["pos"][:-1, :, :2] += np.float32([1.5 * i, -1.0 * i])
        frames.append(frame(t, w, h, flags=flags))
    return frames


def planes_for(seed, n, h, w, own=None):
    """branch_planes per frame -> (nrm, tan, m, gout, kind) stacked; nobody's words NaN where own is given: they may hold anything"""
    out = [np.stack(t) for t in zip(*(tr.branch_planes(seed + i, (h, w)) for i in range(n)))]
    if own is not None:
        for t in out[:4]:
            t[np.broadcast_to(~own[:, None], t.shape)] = np.nan
    return out


def fwd(fs, vis, nrm, tan, m, flags=F, fill=0):
    """the forward pass into a buffer prefilled with the word `fill` -> uint32 [n, 3, rows, W]; nrm, tan, m: device tensors"""
    out = filled(fs.interpolate_shape(3), fill)
    torch.cuda.synchronize()
    fs.normal_map(vis.data_ptr(), nrm.data_ptr(), tan.data_ptr(), m.data_ptr(), out.data_ptr(), fs.interpolate_bytes(3), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def bwd(fs, vis, nrm, tan, m, gout, want=(True, True, True), flags=F, fill=0):
    """the backward pass -> (gnrm [n, 3, ..], gtan [n, 4, ..], gm [n, 3, ..]) uint32 from `fill`, None where not wanted"""
    g = dev(gout)
    outs = [filled(fs.interpolate_shape(c), fill) if w_ else None for c, w_ in zip((3, 4, 3), want)]
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    torch.cuda.synchronize()
    fs.normal_map_grad(vis.data_ptr(), nrm.data_ptr(), tan.data_ptr(), m.data_ptr(), g.data_ptr(), *(ptr(t) for t in outs), flags, stream())
    torch.cuda.synchronize()
    return tuple(None if t is None else words(t) for t in outs)


def expect_fwd(tmp_path, frames, v, nw, tw, mw, fused=True, fill=0):
    return np.stack([tr.nm_forward(tmp_path, n_tris(f), v[i, 1], nw[i], tw[i], mw[i], fused, fill) for i, f in enumerate(frames)])


def expect_bwd(tmp_path, frames, v, nw, tw, mw, gout, fused=True, fill=0, want=(True, True, True)):
    per = [tr.nm_grad(tmp_path, n_tris(f), v[i, 1], nw[i], tw[i], mw[i], gout[i], fused, fill, want) for i, f in enumerate(frames)]
    return tuple(None if per[0][k] is None else np.stack([q[k] for q in per]) for k in range(3))


def check_planes(got, want, what):
    for name, g, w in zip(("gnrm", "gtan", "gm"), got, want):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            same(g, w, f"{what} {name}")


# ------------------------------------------------------------------------------------------------------ every branch, both sizes
@pytest.mark.parametrize("w,h,n", SIZES)
def test_every_branch_fused_and_not(ctx, tmp_path, w, h, n):
    """three frames of hand-written planes that drive every branch of classify() under the GPU's own visibility buffer: forward and
    the three gradient planes, with the fused clear (nobody's words become 0) and without it (the prefilled sentinel survives on
    exactly nobody's pixels); each NULL-able gradient output left out in turn gives the same words for the others"""
    for flags, fused in ((F, True), (0, False)):  # (the flag of the call; the frames' own flag is 0 without it: either one fuses the clear)
        frames = make_frames(w, h, n, flags=F if fused and w == 64 else 0)
        fs = ctx.frameset(frames)
        vis = visibility(fs)
        v = words(vis)
        own = owners(v, frames)
        assert own.any(1).any(1).all() and (~own).sum() > 50
        nw, tw, mw, gout, kind = planes_for(w, N_FRAMES, h, w, own)
        cls = np.stack([tr.nm_classify(tmp_path, n_tris(f), v[i, 1], nw[i], tw[i], mw[i]) for i, f in enumerate(frames)])
        for want in (0, tr.OWNED, tr.OWNED | tr.LIT, tr.OWNED | tr.LIT | tr.FRAME, 15):
            assert int((cls == want).sum()) >= 20, (want, int((cls == want).sum()))
        assert ((kind == 7) & own & ~np.isfinite(gout).all(1)).sum() >= 10
        nrm, tan, m = dev(nw), dev(tw), dev(mw)
        what = f"{w}x{h} fused {fused}"
        got = fwd(fs, vis, nrm, tan, m, flags, SENTINEL)
        same(got, expect_fwd(tmp_path, frames, v, nw, tw, mw, fused, SENTINEL), what)
        nobody = np.broadcast_to(~own[:, None], got.shape)
        assert (got[nobody] == (0 if fused else SENTINEL)).all() and (got[~nobody] != SENTINEL).all()
        res = bwd(fs, vis, nrm, tan, m, gout, flags=flags, fill=SENTINEL)
        check_planes(res, expect_bwd(tmp_path, frames, v, nw, tw, mw, gout, fused, SENTINEL), what)
        for q in res:
            nb = np.broadcast_to(~own[:, None], q.shape)
            assert (q[nb] == (0 if fused else SENTINEL)).all()
        assert not res[1][:, 3][own].any()  # the w plane of gtan: +0 at every owner
        for k in range(3):  # each output left out in turn
            want = tuple(i != k for i in range(3))
            part = bwd(fs, vis, nrm, tan, m, gout, want, flags, SENTINEL)
            assert part[k] is None
            for i in range(3):
                if i != k:
                    assert np.array_equal(part[i], res[i]), (what, k, i)
        assert np.isnan(got.view(np.float32)).sum() == 0  # (the forward stops every NaN: a NaN normal is not lit, a NaN frame gives N)
        assert np.isnan(res[0].view(np.float32)).any()    # (a non-finite gout propagates)
        fs.close()


def test_not_clearing_frames_and_ids_out_of_range(ctx, tmp_path):
    """frames that do not clear; ids out of range and bare class bits written into the buffer: nobody, with and without the flag"""
    t = soup(3, 40, 96, 80, ZS)
    frames = [frame(t, 96, 80, flags=0) for _ in range(N_FRAMES)]
    fs = ctx.frameset(frames)
    vn = visibility(fs).cpu().numpy()
    ids = vn[0, 1].view(np.uint32)
    ids[0, :16], ids[1, :16], ids[2, :16], ids[3, :16], ids[4, :16] = len(t) + 1, 0x7fffffff, 0xffffffff, (len(t) + 1) | 0x80000000, 0x80000000
    vis = torch.as_tensor(vn).cuda()
    vw = vn.view(np.uint32)
    own = owners(vw, frames)
    assert (~own[0])[:5, :16].all() and (~own[0]).sum() > 500 and own[0].sum() > 200
    nw, tw, mw, gout, _ = planes_for(23, N_FRAMES, 80, 96, own)
    nrm, tan, m = dev(nw), dev(tw), dev(mw)
    for flags, fused in ((F, True), (0, False)):
        same(fwd(fs, vis, nrm, tan, m, flags, SENTINEL), expect_fwd(tmp_path, frames, vw, nw, tw, mw, fused, SENTINEL), f"fused {fused}")
        check_planes(bwd(fs, vis, nrm, tan, m, gout, flags=flags, fill=SENTINEL),
                     expect_bwd(tmp_path, frames, vw, nw, tw, mw, gout, fused, SENTINEL), f"fused {fused}")
    fs.close()


# ------------------------------------------------------------------------------------------------------ sharded
def test_sharded_world_2(ctx, tmp_path):
    """a 64 x 100 frame is four bands, the last one partial; rank 0 holds bands 0 and 2, rank 1 bands 1 and 3: each rank's rows equal
    the whole frame's, bit for bit"""
    import srz
    w, h = 64, 100
    frames = make_frames(w, h, 50)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    nw, tw, mw, gout, _ = planes_for(29, N_FRAMES, h, w)
    full = fwd(fs, vis, dev(nw), dev(tw), dev(mw))
    same(full, expect_fwd(tmp_path, frames, v, nw, tw, mw), "whole frame")
    whole = bwd(fs, vis, dev(nw), dev(tw), dev(mw), gout)
    check_planes(whole, expect_bwd(tmp_path, frames, v, nw, tw, mw, gout), "whole frame")
    fs.close()
    for rank in (0, 1):
        c = srz.Context(0)
        c.set_shard(rank, 2)
        sfs = c.frameset(frames)
        svis = visibility(sfs)
        rows = parallel.band_rows(h, rank, 2)
        assert len(rows) == 2
        local = [np.zeros(sfs.interpolate_shape(ch), np.float32) for ch in (3, 4, 3, 3)]
        for (lb, _, r0, r1) in rows:
            for dst, src in zip(local, (nw, tw, mw, gout)):
                dst[:, :, lb * 32: lb * 32 + r1 - r0] = src[:, :, r0:r1]
        sn, st, sm, sg = local
        shard = fwd(sfs, svis, dev(sn), dev(st), dev(sm))
        part = bwd(sfs, svis, dev(sn), dev(st), dev(sm), sg)
        for (lb, _, r0, r1) in rows:
            same(shard[:, :, lb * 32: lb * 32 + r1 - r0], full[:, :, r0:r1], f"rank {rank} band {lb}")
            for k in range(3):
                same(part[k][:, :, lb * 32: lb * 32 + r1 - r0], whole[k][:, :, r0:r1], f"plane {k} rank {rank} band {lb}")
        sfs.close(), c.close()


# ------------------------------------------------------------------------------------------------------ autograd
def test_autograd_is_the_plain_call(ctx, tmp_path, monkeypatch):
    import srz
    w, h = 45, 37
    frames = make_frames(w, h, 30)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    nw, tw, mw, gout, _ = planes_for(31, N_FRAMES, h, w)
    gout = np.where(np.isfinite(gout), gout, np.float32(0.5))
    calls = []
    real = srz.FrameSet.normal_map_grad
    monkeypatch.setattr(srz.FrameSet, "normal_map_grad", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    nt, tt, mt = (dev(t).requires_grad_(True) for t in (nw, tw, mw))
    out = V.normal_map(fs, vis, nt, tt, mt)
    assert out.shape == (N_FRAMES, 3, h, w) and out.requires_grad
    same(words(out.detach()), fwd(fs, vis, dev(nw), dev(tw), dev(mw)), "forward")
    out.backward(dev(gout))
    torch.cuda.synchronize()
    assert len(calls) == 1  # one launch for every gradient
    plain = V.normal_map_grad(fs, vis, dev(nw), dev(tw), dev(mw), dev(gout))
    want = expect_bwd(tmp_path, frames, v, nw, tw, mw, gout)
    for name, a, b, c_ in zip(("nrm", "tan", "m"), (nt.grad, tt.grad, mt.grad), plain, want):
        same(words(a), words(b), name + ".grad against the plain call")
        same(words(b), c_, name + ": the plain call against the reference")
    # one input needs a gradient: the call asks for that output alone; none: there is no backward
    m2 = dev(mw).requires_grad_(True)
    V.normal_map(fs, vis, dev(nw), dev(tw), m2).backward(dev(gout))
    same(words(m2.grad), want[2], "m alone")
    assert len(calls) == 3 and V.normal_map(fs, vis, dev(nw), dev(tw), dev(mw)).grad_fn is None
    assert V.normal_map_grad(fs, vis, dev(nw), dev(tw), dev(mw), dev(gout), want_gnrm=False, want_gm=False)[::2] == (None, None)
    with pytest.raises(ValueError):
        V.normal_map_grad(fs, vis, dev(nw), dev(tw), dev(mw), dev(gout), False, False, False)
    with pytest.raises(ValueError):
        V.normal_map(fs, vis, dev(nw), dev(tw[:, :3]), dev(mw))
    fs.close()


# ------------------------------------------------------------------------------------------------------ a real scene, the chain
def scene(ctx, slot=3, size=64):
    """a wavy 16 x 16 grid under two perspective views -> (fs, T, positions, faces, uv, the set's visibility buffer)"""
    ident = np.eye(4, dtype=np.float32).reshape(16)
    posn, faces = vgkit.grid(16, 16, 3, extra=1)
    posn[:, 2] += (0.08 * np.sin(7.0 * posn[:, 0]) * np.cos(5.0 * posn[:, 1])).astype(np.float32)
    mvps = [vgkit.perspective(50.0, 46.0, 5.0, 6.0), vgkit.perspective(38.0, 52.0, 14.0, 3.0, w=1.5, wx=-0.2, wy=0.3, wz=0.25, sz=2.0, oz=4.0)]
    faces = vgkit.oriented(posn, faces, mvps[0])
    uv = tr.degenerate_face(tr.make_uv(posn, "folded"), faces, 5)
    v8 = vgkit.verts8(posn)
    v8[:, 6:8] = uv
    sframes, plain = [], []
    for i, mm in enumerate(mvps):
        sf, f = scene_pair([(v8, faces, abi.SHADER_NORMAL, -1, mm, ident)], size, size, (0.0, 0.0, 1.0), [], 1.75, 0.5,
                           ctx=ctx if i == 0 else None, slots=[slot])
        sframes.append(sf), plain.append(f)
    fs = ctx.frameset(sframes)
    return fs, max(f.n_tris for f in plain), posn, faces, uv, visibility(fs)


def test_a_real_scene_through_the_chain(ctx, tmp_path):
    """mesh_tangents -> corner_attr -> interpolate -> normal_map on a sceneset: the tangent planes carry both handednesses, the pass
    equals the reference on the planes the chain produced, T and B come out orthonormal to N, and a gradient reaches the vertices
    through the tangents and through the normals"""
    SLOT = 3
    fs, T, posn, faces, uv, vis = scene(ctx, SLOT)
    v = words(vis)
    own = owners(v, [T, T])
    assert own.sum() > 500
    verts = dev(posn).requires_grad_(True)
    tan = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: V.mesh_tangents(ctx, SLOT, verts)}, pos_tris=T))
    nrm = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: V.mesh_normals(ctx, SLOT, verts)}, pos_tris=T))
    tw, nw = tan.detach().cpu().numpy(), nrm.detach().cpu().numpy()
    assert tuple(tan.shape) == (2, 4, 64, 64) and (tw[:, 3][own] < 0).sum() > 50 and (tw[:, 3][own] > 0).sum() > 50
    # the slot's own uv (None) and the explicit tensor give the same tangents
    assert torch.equal(V.mesh_tangents(ctx, SLOT, verts.detach()), V.mesh_tangents(ctx, SLOT, verts.detach(), dev(uv)))
    rng = np.random.default_rng(37)
    for mvec in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), None):
        mw = np.float32(rng.normal(0, 0.4, (2, 3, 64, 64)) + np.float32([0, 0, 1]).reshape(1, 3, 1, 1)) if mvec is None else \
            np.broadcast_to(np.float32(mvec).reshape(1, 3, 1, 1), (2, 3, 64, 64)).copy()
        out = V.normal_map(fs, vis, nrm, tan, dev(mw))
        same(words(out.detach()), expect_fwd(tmp_path, [T, T], v, nw, tw, mw), f"scene forward m {mvec}")
        if mvec is not None:
            # T, then B: unit, orthogonal to the interpolated normal.  DERIVED (tests/test_tangent_ref.py): a component of the output is
            # within (192 rho + 73) u of the exact one, rho = |t| / |Tp|, so its dot product with the unit normal is within three times
            # that of 0; its length is within 5 u of 1 (the last normalisation alone: 4.5 u)
            o, n, t3 = np.float64(out.detach().cpu().numpy()), np.float64(nw), np.float64(tw[:, :3])
            ok = own & np.stack([tr.well_conditioned(nw[i], tw[i], mw[i]) for i in range(2)])
            assert ok.sum() > 400
            N = n / np.where(ok[:, None], np.sqrt((n * n).sum(1, keepdims=True)), 1.0)
            Tp = t3 - N * (N * t3).sum(1, keepdims=True)
            rho = np.sqrt((t3 * t3).sum(1) / np.where(ok, (Tp * Tp).sum(1), 1.0))
            assert (np.abs((o * N).sum(1)) <= 3 * (192 * rho + 73) * 2.0 ** -24)[ok].all()
            assert np.abs(np.sqrt((o * o).sum(1)) - 1)[ok].max() <= 5 * 2.0 ** -24
    weight = dev(rng.normal(0, 1, (2, 3, 64, 64)))
    (out * weight).sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(verts.grad).all()) and int((verts.grad != 0).sum()) > verts.grad.numel() // 2
    both = verts.grad.clone()
    verts.grad = None
    tan2 = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: V.mesh_tangents(ctx, SLOT, verts)}, pos_tris=T))
    (V.normal_map(fs, vis, nrm.detach(), tan2, dev(mw)) * weight).sum().backward()
    assert bool((verts.grad != 0).any()) and not torch.equal(verts.grad, both)
    fs.close()


def test_the_chain_into_light_with_m_from_a_texture(ctx, tmp_path):
    """out = light(normal_map(nrm, tan, texture(normal_tex, uv)), pos, ...): the gradient planes of m, nrm and tan equal the CPU
    references COMPOSED — lightref's gradient of the shading normal fed to tangentref's backward — bit for bit (both are per pixel),
    and the texel gradient of the normal texture lies within texref's bound for its atomics: gamma_n * sum |w * g|, n the texel's
    adds, u = 2^-24, the products being the float32 products themselves"""
    SLOT = 3
    fs, T, posn, faces, uv, vis = scene(ctx, SLOT)
    v = words(vis)
    rng = np.random.default_rng(41)
    verts = dev(posn)
    tan = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: V.mesh_tangents(ctx, SLOT, verts)}, pos_tris=T)).requires_grad_(True)
    nrm = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: V.mesh_normals(ctx, SLOT, verts)}, pos_tris=T)).requires_grad_(True)
    pos = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: verts}, pos_tris=T))
    uvp = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: dev(uv)}, pos_tris=T))
    texn = np.float32(rng.normal(0, 0.3, (16, 16, 3)) + np.float32([0, 0, 1]))  # a learned map: signed values, stored directly
    tex = dev(texn).requires_grad_(True)
    m = V.texture(fs, vis, tex, uvp)
    m.retain_grad()
    sn = V.normal_map(fs, vis, nrm, tan, m)
    sn.retain_grad()
    centre = posn.mean(0)
    lights = dev([[*(centre + (0.3, 0.2, 1.5)), 9.0, 8.0, 7.0], [*(centre + (-0.4, 0.3, -1.2)), 3.0, 4.0, 5.0]])
    eye, ka, ks = (dev(t) for t in (centre + (0.1, -0.1, 2.0), (0.05, 0.06, 0.07), (0.5, 0.4, 0.3)))
    img = V.light(fs, vis, sn, pos, None, lights, eye, ka, ks, 7)
    weight = rng.normal(0, 1, tuple(img.shape)).astype(np.float32)
    (img * dev(weight)).sum().backward()
    torch.cuda.synchronize()
    nw, tw, mw, pw = (t.detach().cpu().numpy() for t in (nrm, tan, m, pos))
    par = V.light_params(fs, lights, eye, ka, ks).cpu().numpy()[0]
    # the references composed, frame by frame
    snw = expect_fwd(tmp_path, [T, T], v, nw, tw, mw)
    same(words(sn.detach()), snw, "the shading normal")
    gsn = np.stack([lightref.grad(tmp_path, T, v[i, 1], snw[i], pw[i], None, par, 7, weight[i])[0] for i in range(2)])
    same(words(sn.grad), gsn, "light's gradient of the shading normal")
    assert (gsn != 0).sum() > 1000
    gn, gt, gm = expect_bwd(tmp_path, [T, T], v, nw, tw, mw, gsn)
    same(words(m.grad), gm, "d_gm"), same(words(nrm.grad), gn, "d_gnrm"), same(words(tan.grad), gt, "d_gtan")
    assert (gm != 0).sum() > 1000 and (gt[:, :3] != 0).sum() > 1000 and not gt[:, 3].any()
    acc = texref.Grad(texn.shape)
    for i in range(2):
        texref.grad(tmp_path, texn, texref.CLAMP, T, v[i, 1], uvp.detach().cpu().numpy()[i], gm[i], acc, False)
    got = tex.grad.cpu().numpy()
    err = np.abs(got.astype(np.float64) - acc.gtex)
    print("texel gradient: max err / bound", float(np.max(err[acc.bound() > 0] / acc.bound()[acc.bound() > 0])))
    assert (err <= acc.bound()).all() and (got[acc.count == 0] == 0).all() and (acc.gtex != 0).sum() > 100
    fs.close()
