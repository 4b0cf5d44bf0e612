"""-m gpu: mipmapped texture sampling over a visibility buffer and its gradients (srz_texture_mip_build / _fold, k_mip_build,
k_mip_fold; srz_frameset_interpolate_deriv, k_interp_deriv; srz_frameset_texture_mip / _texture_mip_grad, k_tex_mip, k_tex_mip_grad).
The visibility buffer is the GPU's own render_visibility, uv the GPU's own interpolate and uvd the GPU's own interpolate_deriv of the
frames' uv, the pyramid the GPU's own build — except where a test writes them by hand; the expected values are tests/mipref.py's on
those very buffers, with the reference's OWN pyramid (pinned on the CPU by tests/test_mip_ref.py).  Build, fold, the derivative
planes, forward and guv: a NaN on one side must be a NaN on the other, every other word matches bit for bit.  gtex and gmip, per
level: exact where every partial sum is representable (the dyadic case) and where an element has one contributing add, else within
gamma_n * sum |(w lw) g|, gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing adds — one rounding per add, the
products being float32 products on both sides: derived, not measured."""
import numpy as np
import pytest
import torch

import interpref
import mipref
import texref
from mipref import CLAMP, WRAP
from srz import abi, parallel
from support import SENTINEL, ctx, filled, frame, padded_positions, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = mipref.ZS
FRAME_SIZES = [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6)]
CHANNELS = (1, 3, 5, 17, 64)
U = 2.0 ** -24


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def ptr(t):
    return t.data_ptr() if t is not None else None


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def tex_dims(tex):
    return (tex.shape[0] if tex.ndim == 4 else 1), tex.shape[-3], tex.shape[-2], tex.shape[-1]


def tex_of(t, i):
    return t[i] if t.ndim == 4 else t


def full_levels(tex):
    import srz
    return srz.mip_levels(tex.shape[-2], tex.shape[-3])


def gpu_build(c, tex, L, fill=None):
    """the GPU's pyramid of tex → a flat float32 tensor on the device (empty for L == 1)"""
    import srz
    tf, h, w, C = tex_dims(tex)
    nbytes = srz.mip_bytes(w, h, C, tf, L)
    mip = torch.zeros((nbytes // 4,), dtype=torch.float32, device="cuda") if fill is None else filled((nbytes // 4,), fill).view(torch.float32)
    t = dev(tex)
    c.mip_build(t.data_ptr(), w, h, C, tf, L, mip.data_ptr(), nbytes, stream())
    torch.cuda.synchronize()
    return mip


def interp_uv(fs, vis, frames, scale=1.0):
    """the GPU's interpolate and interpolate_deriv of the frames' own uv (times `scale`) → uv [n, 2, rows, W] and uvd [n, 4, rows, W]
    on the device, and the attributes [n, T, 3, 2] they came from"""
    T = max(f.n_tris for f in frames)
    a = np.zeros((len(frames), T, 3, 2), np.float32)
    for i, f in enumerate(frames):
        a[i, :f.n_tris] = texref.frame_uv(f) * np.float32(scale)
    a_dev = dev(a)
    uv, uvd = torch.zeros(fs.interpolate_shape(2), dtype=torch.float32, device="cuda"), torch.zeros(fs.interpolate_shape(4), dtype=torch.float32, device="cuda")
    fs.interpolate(vis.data_ptr(), a_dev.data_ptr(), 2, len(frames), T, uv.data_ptr(), fs.interpolate_bytes(2), F, stream())
    fs.interpolate_deriv(vis.data_ptr(), a_dev.data_ptr(), 2, len(frames), T, uvd.data_ptr(), fs.interpolate_bytes(4), F, stream())
    torch.cuda.synchronize()
    return uv, uvd, a


def fwd(fs, vis, uv, uvd, tex, mode, L, flags=F, fill=0, mip=None):
    """the forward pass into a buffer prefilled with the word `fill` → uint32 [n, C, rows, W]"""
    tf, h, w, C = tex_dims(tex)
    out, t = filled(fs.interpolate_shape(C), fill), dev(tex)
    mip = (gpu_build(fs.ctx, tex, L) if L > 1 else None) if mip is None else mip
    fs.texture_mip(vis.data_ptr(), uv.data_ptr(), ptr(uvd) if L > 1 else None, t.data_ptr(), w, h, C, tf, mode, ptr(mip) if L > 1 else None, L,
                   out.data_ptr(), fs.interpolate_bytes(C), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def bwd(fs, vis, uv, uvd, gout, tex, mode, L, want_tex=True, want_uv=True, flags=F, fill=0, into=None):
    """the backward pass → (gtex float32 of tex's shape and gmip flat float32, added into `into` = (gtex, gmip) or zeros; guv uint32
    [n, 2, rows, W] from `fill`)"""
    import srz
    tf, h, w, C = tex_dims(tex)
    t, g = dev(tex), dev(gout)
    assert tuple(g.shape) == tuple(fs.interpolate_shape(C))
    mip = gpu_build(fs.ctx, tex, L) if L > 1 else None
    n_mip = srz.mip_bytes(w, h, C, tf, L) // 4
    gt = (torch.zeros_like(t) if into is None else dev(into[0])) if want_tex else None
    gm = (torch.zeros((n_mip,), dtype=torch.float32, device="cuda") if into is None else dev(into[1])) if want_tex and L > 1 else None
    gu = filled(fs.interpolate_shape(2), fill) if want_uv else None
    fs.texture_mip_grad(vis.data_ptr(), uv.data_ptr(), ptr(uvd) if L > 1 else None, g.data_ptr(), t.data_ptr(), ptr(mip), w, h, C, tf, mode, L,
                        ptr(gt), ptr(gm), ptr(gu), flags, stream())
    torch.cuda.synchronize()
    return (gt.cpu().numpy() if want_tex else None), (gm.cpu().numpy() if gm is not None else np.zeros(0, np.float32)), (words(gu) if want_uv else None)


def expect_fwd(tmp_path, frames, v, uvw, uvdw, tex, mode, L, fused=True, fill=0):
    out = []
    for i, f in enumerate(frames):
        pre = np.full((tex.shape[-1],) + v.shape[2:], fill, np.uint32)
        t = tex_of(tex, i)
        out.append(mipref.forward(tmp_path, t, mipref.build(tmp_path, t, L), mode, L, f.n_tris, v[i, 1], uvw[i], uvdw[i] if L > 1 else None, fused, pre))
    return np.stack(out)


def expect_bwd(tmp_path, frames, v, uvw, uvdw, gout, tex, mode, L, fused=True, fill=0):
    """(a mipref.Grad per texture frame — one for a shared texture —, guv [n, 2, rows, W] float32)"""
    shared = tex.ndim == 3
    accs = [mipref.Grad(tmp_path, tex.shape[-3:], L) for _ in range(1 if shared else len(frames))]
    gu = []
    for i, f in enumerate(frames):
        pre = np.full((2,) + v.shape[2:], fill, np.uint32)
        t = tex_of(tex, i)
        gu.append(mipref.grad(tmp_path, t, mipref.build(tmp_path, t, L), mode, L, f.n_tris, v[i, 1], uvw[i], uvdw[i] if L > 1 else None, gout[i],
                              accs[0 if shared else i], True, fused, pre))
    return accs, np.stack(gu)


def check_levels(tmp_path, gt, gm, accs, tex_shape, L, what, exact=False, init=None):
    """every level of the texel gradients: level 0 in gt, the others in the flat gm; init = (gtex, gmip) the buffers held before the
    call (one more term of every element's sum).  Finite references only."""
    got = [gt.reshape((-1,) + tuple(tex_shape[-3:]))] + [x.reshape((len(accs),) + x.shape[-3:]) for x in mipref.views(tmp_path, gm, tex_shape, L)]
    inits = None
    if init is not None:
        inits = [init[0].reshape(got[0].shape)] + [x.reshape((len(accs),) + x.shape[-3:]) for x in mipref.views(tmp_path, init[1], tex_shape, L)]
    worst = 0.0
    for l in range(L):
        ref = np.stack([a.level(l)[0] for a in accs])
        mag = np.stack([a.level(l)[1] for a in accs])
        cnt = np.stack([np.broadcast_to(a.level(l)[2][:, :, None], a.level(l)[0].shape) for a in accs]).astype(np.float64)
        g = got[l]
        assert g.shape == ref.shape, (what, l, g.shape, ref.shape)
        if inits is not None:
            ref, mag, cnt = ref + inits[l].astype(np.float64), mag + np.abs(inits[l].astype(np.float64)), cnt + 1
        assert np.isfinite(ref).all()
        nu = cnt * U
        bound = nu / (1.0 - nu) * mag
        if exact:
            assert (ref.astype(np.float32).astype(np.float64) == ref).all(), "the case is not dyadic"
            bound = np.zeros_like(bound)
        err = np.abs(g.astype(np.float64) - ref)
        if (bound > 0).any():
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
        bad = ~(err <= bound)
        assert not bad.any(), f"{what} level {l}: {int(bad.sum())} elements beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
        one = cnt == 1
        same((g + np.float32(0))[one], (ref.astype(np.float32) + np.float32(0))[one], f"{what} level {l} (n = 1)")
        assert (g[cnt == 0] == 0).all()
    print(f"{what}: max err / bound {worst:.3f}; adds per level {[int(accs[0].level(l)[2].sum()) for l in range(L)]}")


def rand_gout(seed, shape, own=None):
    g = np.random.default_rng([seed, 8]).normal(0, 2, shape).astype(np.float32)
    if own is not None:
        g[np.broadcast_to(~own[:, None], g.shape)] = np.nan  # nobody's words may hold anything
    return g


def owners(v, frames):
    return np.stack([((v[i, 1] & 0x7fffffff) - np.uint32(1)) < f.n_tris for i, f in enumerate(frames)])


def rendered(ctx, w, h, n, scale=1.0, flags=None):
    frames = mipref.soup_frames(w, h, n, flags=flags)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    uv, uvd, attr = interp_uv(fs, vis, frames, scale)
    return frames, fs, vis, words(vis), uv, uvd, attr


# ------------------------------------------------------------------------------------------------------ build and fold
@pytest.mark.parametrize("tw,th", mipref.TEX_SIZES)
def test_build_and_fold(ctx, tmp_path, tw, th):
    import srz
    full = srz.mip_levels(tw, th)
    assert full == mipref.levels(tmp_path, tw, th)
    for k, C in enumerate(CHANNELS):
        tex = mipref.make_tex(k, tw, th, C, frames=3)
        tex[0, 0, 0, 0] = np.inf if C == 5 else tex[0, 0, 0, 0]  # non-finite texels propagate as IEEE has them
        for t in (tex, tex[0]):
            for L in sorted({1, min(2, full), full}):
                nbytes = srz.mip_bytes(tw, th, C, tex_dims(t)[0], L)
                got = gpu_build(ctx, t, L, fill=SENTINEL).cpu().numpy()
                want = mipref.build(tmp_path, t, L)
                assert got.size * 4 == nbytes == want.size * 4
                same(got, want, f"build {tw}x{th} C {C} {t.ndim} L {L}")
                # fold: a gradient pyramid into a buffer that is not zero
                rng = np.random.default_rng([tw, th, C, L])
                gm, g0 = rng.normal(0, 2, want.size).astype(np.float32), rng.normal(0, 2, t.shape).astype(np.float32)
                if L == 1:
                    continue
                gmd, g0d = dev(gm), dev(g0)
                ctx.mip_fold(gmd.data_ptr(), nbytes, tw, th, C, tex_dims(t)[0], L, g0d.data_ptr(), stream())
                torch.cuda.synchronize()
                same(g0d.cpu().numpy(), mipref.fold(tmp_path, gm, t.shape, L, g0), f"fold {tw}x{th} C {C} {t.ndim} L {L}")
                assert np.array_equal(gmd.cpu().numpy(), gm)  # read only
    if full > 1:
        assert (mipref.build(tmp_path, tex, full) != 0).any()


# ------------------------------------------------------------------------------------------------------ interpolate_deriv
def deriv(fs, vis, attr, flags=F, fill=0):
    """attr [T, 3, C] or [n, T, 3, C] → uint32 [n, 2 C, rows, W]"""
    a = dev(attr)
    C = attr.shape[-1]
    out = filled(fs.interpolate_shape(2 * C), fill)
    fs.interpolate_deriv(vis.data_ptr(), a.data_ptr(), C, attr.shape[0] if attr.ndim == 4 else 1, attr.shape[-3], out.data_ptr(),
                         fs.interpolate_bytes(2 * C), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def expect_deriv(tmp_path, frames, v, attr, fused=True, fill=0):
    T = attr.shape[-3]
    pos = padded_positions(frames, T)
    out = []
    for i, f in enumerate(frames):
        pre = np.full((2 * attr.shape[-1],) + v.shape[2:], fill, np.uint32)
        out.append(mipref.deriv(tmp_path, tex_of(attr, i), pos[i], f.n_tris, v[i, 1], fused, pre))
    return np.stack(out)


@pytest.mark.parametrize("w,h,n", FRAME_SIZES)
def test_deriv_on_rendered_buffers(ctx, tmp_path, w, h, n):
    frames = mipref.soup_frames(w, h, n)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    own = owners(v, frames)
    assert own.any(1).any(1).all()
    T = frames[0].n_tris + 3
    wide = np.random.default_rng([w, h]).normal(0, 2, (2, T, 3, 32)).astype(np.float32)
    wide[0, 1, 2, 0], wide[1, 0, 0, 1] = np.nan, np.inf
    full = deriv(fs, vis, wide, F, SENTINEL)
    same(full, expect_deriv(tmp_path, frames, v, wide, fill=SENTINEL), f"{w}x{h} C 32")
    assert (full[np.broadcast_to(~own[:, None], full.shape)] == 0).all()
    for C in (1, 2, 3, 5, 17):
        for a in (wide[..., :C], wide[1][..., :C]):
            got = deriv(fs, vis, a, F, SENTINEL)
            same(got, expect_deriv(tmp_path, frames, v, a, fill=SENTINEL), f"{w}x{h} C {C} {a.ndim}")
            if a.ndim == 4:
                assert np.array_equal(got, full[:, :2 * C])
    fs.close()


def test_deriv_not_fused_hand_written_ids_and_degenerate_triangles(ctx, tmp_path):
    t = soup(3, 40, 96, 80, ZS)
    t["pos"][5, 1] = t["pos"][5, 0]  # a zero area under an id written by hand below: inf / NaN as IEEE has them
    frames = [frame(t, 96, 80, flags=0), frame(t, 96, 80, flags=0)]
    fs = ctx.frameset(frames)
    vn = visibility(fs).cpu().numpy()
    ids = vn[0, 1].view(np.uint32)
    ids[0, :16], ids[1, :16], ids[2, :16], ids[3, :16], ids[4, :16] = len(t) + 1, 0x7fffffff, 0xffffffff, (len(t) + 1) | 0x80000000, 0x80000000
    ids[5, :16], ids[6, :16] = 6, 6 | 0x80000000
    vis = torch.as_tensor(vn).cuda()
    vw = vn.view(np.uint32)
    own = owners(vw, frames)
    assert (~own[0, :5, :16]).all() and own[0, 5:7, :16].all() and (~own[0]).sum() > 500 and own[0].sum() > 200
    attr = np.random.default_rng(2).normal(0, 2, (len(t), 3, 6)).astype(np.float32)
    fused, kept = deriv(fs, vis, attr, F, SENTINEL), deriv(fs, vis, attr, 0, SENTINEL)
    same(fused, expect_deriv(tmp_path, frames, vw, attr, True, SENTINEL), "fused")
    same(kept, expect_deriv(tmp_path, frames, vw, attr, False, SENTINEL), "not fused")
    assert (fused[0][:, ~own[0]] == 0).all() and (kept[0][:, ~own[0]] == SENTINEL).all() and (kept[0][:, own[0]] != SENTINEL).all()
    assert not np.isfinite(fused.view(np.float32)[0, :, 5:7, :16]).any()
    fs.close()


def test_deriv_sceneset_equals_the_frameset_of_its_stream(ctx, tmp_path):
    from srz import scenes as pscenes
    wl = pscenes.spot_bunny_1080p()
    wl.upload_meshes(ctx)
    frames = [wl.frame(3), wl.frame(4)]
    fs, ss = ctx.frameset(frames), ctx.frameset([wl.scene_frame(3), wl.scene_frame(4)])
    vis_f, vis_s = visibility(fs), visibility(ss)
    assert torch.equal(vis_f.view(torch.int32), vis_s.view(torch.int32))
    v = words(vis_f)
    T = max(f.n_tris for f in frames)
    attr = np.random.default_rng(4).normal(0, 1, (T, 3, 2)).astype(np.float32)
    want = expect_deriv(tmp_path, frames, v, attr)
    for name, s, vis in (("frameset", fs, vis_f), ("sceneset", ss, vis_s)):
        got = deriv(s, vis, attr)
        same(got, want, name)
        assert (got[0, 0] != 0).sum() > 10000
    fs.close(), ss.close()


def test_deriv_sharded_world_2(ctx, tmp_path):
    import srz
    w, h, tris = 64, 128, 50
    frames = mipref.soup_frames(w, h, tris - 1)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    attr = np.random.default_rng(6).normal(0, 1, (2, tris, 3, 3)).astype(np.float32)
    full = deriv(fs, vis, attr)
    same(full, expect_deriv(tmp_path, frames, words(vis), attr), "whole frame")
    fs.close()
    for rank in (0, 1):
        c = srz.Context(0, rank, 2)
        sfs = c.frameset(frames)
        shard = deriv(sfs, visibility(sfs), attr)
        rows = parallel.band_rows(h, rank, 2)
        assert len(rows) == 2
        for (lb, _, r0, r1) in rows:
            same(shard[:, :, lb * 32: lb * 32 + r1 - r0], full[:, :, r0:r1], f"rank {rank} band {lb}")
        sfs.close(), c.close()


# ------------------------------------------------------------------------------------------------------ forward and guv
@pytest.mark.parametrize("w,h,n", FRAME_SIZES)
def test_forward_and_guv_on_rendered_buffers(ctx, tmp_path, w, h, n):
    """every texture size, CLAMP and WRAP, shared and per frame, the channel counts in turn; n_levels 1, 2 and full; the uv attribute
    scaled by 2 at the 64 x 64 frame so that some pixels reach past the border texels and the coarser levels"""
    frames, fs, vis, v, uv, uvd, _ = rendered(ctx, w, h, n, scale=2.0 if w == 64 else 1.0)
    uvw, uvdw = uv.cpu().numpy(), uvd.cpu().numpy()
    own = owners(v, frames)
    k = 0
    for (tw, th) in mipref.TEX_SIZES:
        for mode in (CLAMP, WRAP):
            C = CHANNELS[k % len(CHANNELS)]
            tex = mipref.make_tex(k, tw, th, C, frames=2)
            tex = tex if k % 2 else tex[0]
            k += 1
            full = full_levels(tex)
            for L in sorted({1, min(2, full), full}):
                what = f"{w}x{h} tex {tw}x{th} C {C} mode {mode} {tex.ndim} L {L}"
                got = fwd(fs, vis, uv, uvd, tex, mode, L, F, SENTINEL)
                same(got, expect_fwd(tmp_path, frames, v, uvw, uvdw, tex, mode, L, fill=SENTINEL), what)
                assert (got[np.broadcast_to(~own[:, None], got.shape)] == 0).all()
                gout = rand_gout(k, got.shape, own)
                _, _, gu = bwd(fs, vis, uv, uvd, gout, tex, mode, L, want_tex=False, fill=SENTINEL)
                same(gu, expect_bwd(tmp_path, frames, v, uvw, uvdw, gout, tex, mode, L, fill=SENTINEL)[1], what + " guv")
    fs.close()


def hand_frames(w, h, n, tris, flags=F):
    return [frame(soup(1, tris, w, h, ZS), w, h, flags=flags) for _ in range(n)]


def hand_vis(ids):
    v = np.zeros((ids.shape[0], 4) + ids.shape[1:], np.float32)
    v[:, 1] = ids.view(np.float32)
    return v


def rand_ids(rng, n, h, w, tris, holes=True):
    ids = rng.integers(1, tris + 1, (n, h, w)).astype(np.uint32)
    ids |= (rng.random((n, h, w)) < 0.4).astype(np.uint32) << 31
    if holes:
        ids[rng.random((n, h, w)) < 0.1] = 0
    return ids


def hand_uvd(rng, shape, tw, th, L):
    """[n, 4, h, w]: rho drawn log-uniformly over 2^-2 .. 2^(L + 1) in a random direction, then 0, exact powers of two, NaN, +-inf
    and 3e38 dealt over a third of the pixels"""
    n, h, w = shape
    rho = np.exp2(rng.uniform(-2, L + 1, shape))
    a, b = rng.uniform(0, 2 * np.pi, shape), rng.uniform(0, 1, shape)
    d = np.stack([rho * np.cos(a) / tw, b * rho * np.sin(a) / tw, rho * np.sin(a) / th, -b * rho * np.cos(a) / th], 1).astype(np.float32)
    kind = rng.integers(0, 24, shape)
    for p in range(4):
        d[:, p][kind == 0] = 0.0
    pw = np.exp2(rng.integers(0, L + 2, shape)).astype(np.float32)
    for p, size in ((0, tw), (2, th)):  # exactly 2^k texels along one axis, nothing along the other
        sel = kind == 1 + p
        for q in range(4):
            d[:, q][sel] = 0.0
        d[:, p][sel] = (pw / np.float32(size))[sel]
    special = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38])
    for j, s in enumerate(special):
        sel = kind == 4 + j
        d[:, j % 4][sel] = s
    return d


@pytest.mark.parametrize("tw,th", [(64, 64), (96, 64), (32, 8), (100, 70)])
def test_forward_and_guv_on_hand_written_planes(ctx, tmp_path, tw, th):
    rng = np.random.default_rng([tw, th, 1])
    n, h, w, tris = 2, 50, 70, 20
    frames = hand_frames(w, h, n, tris, flags=0)  # (frames that do not clear: the calls below fuse the clear, or do not)
    fs = ctx.frameset(frames)
    ids = rand_ids(rng, n, h, w, tris)
    v = hand_vis(ids)
    vis = torch.as_tensor(v).cuda()
    vw = v.view(np.uint32)
    uvw = rng.uniform(-0.5, 1.5, (n, 2, h, w)).astype(np.float32)
    special = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, 1.0, -0.0, 0.5])
    hit = rng.random(uvw.shape) < 0.1
    uvw[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    full = mipref.levels(tmp_path, tw, th)
    uvdw = hand_uvd(rng, (n, h, w), tw, th, full)
    l0, f = mipref.lod(tmp_path, (th, tw), full, np.moveaxis(uvdw, 1, 0))
    assert len(set(l0.ravel().tolist())) == full and ((f > 0) & (f < 1)).sum() > 500 and (~np.isfinite(uvdw)).sum() > 200
    uv, uvd = dev(uvw), dev(uvdw)
    for mode, C, per_frame in ((CLAMP, 3, False), (WRAP, 5, True)):
        tex = mipref.make_tex(C, tw, th, C, frames=2 if per_frame else None)
        for L in sorted({1, 2, full}):
            what = f"hand tex {tw}x{th} C {C} mode {mode} L {L}"
            got = fwd(fs, vis, uv, uvd, tex, mode, L, F, SENTINEL)
            same(got, expect_fwd(tmp_path, frames, vw, uvw, uvdw, tex, mode, L, fill=SENTINEL), what)
            gout = rand_gout(L, got.shape)
            _, _, gu = bwd(fs, vis, uv, uvd, gout, tex, mode, L, want_tex=False, fill=SENTINEL)
            same(gu, expect_bwd(tmp_path, frames, vw, uvw, uvdw, gout, tex, mode, L, fill=SENTINEL)[1], what + " guv")
    # not fused: nobody's words stay
    tex = mipref.make_tex(9, tw, th, 2)
    kept = fwd(fs, vis, uv, uvd, tex, CLAMP, full, 0, SENTINEL)
    same(kept, expect_fwd(tmp_path, frames, vw, uvw, uvdw, tex, CLAMP, full, False, SENTINEL), "not fused")
    nobody = ~owners(vw, frames)
    assert (kept[np.broadcast_to(nobody[:, None], kept.shape)] == SENTINEL).all() and nobody.sum() > 300
    _, _, gu = bwd(fs, vis, uv, uvd, rand_gout(1, kept.shape), tex, CLAMP, full, want_tex=False, flags=0, fill=SENTINEL)
    assert (gu[np.broadcast_to(nobody[:, None], gu.shape)] == SENTINEL).all()
    fs.close()


def test_one_level_is_the_bilinear_pass_and_channels_are_slices(ctx, tmp_path):
    frames, fs, vis, v, uv, uvd, _ = rendered(ctx, 100, 70, 120)
    own = owners(v, frames)
    for mode in (CLAMP, WRAP):
        wide = mipref.make_tex(1, 96, 64, 64, frames=2)
        gwide = rand_gout(mode, (2, 64, 70, 100), own)
        # n_levels == 1: FrameSet.texture's words, with the derivative planes and the pyramid null or not
        t, out = dev(wide), filled(fs.interpolate_shape(64), SENTINEL)
        fs.texture(vis.data_ptr(), uv.data_ptr(), t.data_ptr(), 96, 64, 64, 2, mode, out.data_ptr(), fs.interpolate_bytes(64), F, stream())
        torch.cuda.synchronize()
        assert np.array_equal(fwd(fs, vis, uv, uvd, wide, mode, 1, F, SENTINEL), words(out))
        gt1, gu1 = torch.zeros_like(t), filled(fs.interpolate_shape(2), SENTINEL)
        g = dev(np.nan_to_num(gwide))
        fs.texture_grad(vis.data_ptr(), uv.data_ptr(), g.data_ptr(), t.data_ptr(), 96, 64, 64, 2, mode, gt1.data_ptr(), gu1.data_ptr(), F, stream())
        torch.cuda.synchronize()
        _, _, gu = bwd(fs, vis, uv, uvd, np.nan_to_num(gwide), wide, mode, 1, want_tex=False, fill=SENTINEL)
        assert np.array_equal(gu, words(gu1))
        # a C-channel call is the slice of a wider call; want_tex=False gives the same guv
        full = fwd(fs, vis, uv, uvd, wide, mode, 6, F, SENTINEL)
        for C in CHANNELS[:-1]:
            assert np.array_equal(fwd(fs, vis, uv, uvd, wide[..., :C], mode, 6, F, SENTINEL), full[:, :C]), C
        for C in (3, 17):
            gt, gm, gu_both = bwd(fs, vis, uv, uvd, gwide[:, :C], wide[..., :C], mode, 6, fill=SENTINEL)
            _, _, gu_only = bwd(fs, vis, uv, uvd, gwide[:, :C], wide[..., :C], mode, 6, want_tex=False, fill=SENTINEL)
            assert np.array_equal(gu_both, gu_only) and np.isfinite(gt).all() and np.isfinite(gm).all()
    fs.close()


# ------------------------------------------------------------------------------------------------------ gtex and gmip
@pytest.mark.parametrize("w,h,n", FRAME_SIZES[:3])
def test_texel_gradients_on_rendered_buffers_and_accumulation(ctx, tmp_path, w, h, n):
    frames, fs, vis, v, uv, uvd, _ = rendered(ctx, w, h, n, scale=2.0 if w == 64 else 1.0)
    uvw, uvdw = uv.cpu().numpy(), uvd.cpu().numpy()
    own = owners(v, frames)
    for (tw, th), C, per_frame, mode in (((64, 64), 3, True, WRAP), ((96, 64), 17, False, CLAMP), ((32, 8), 5, True, CLAMP), ((100, 70), 1, False, WRAP),
                                         ((5, 7), 4, False, WRAP), ((1, 1), 2, True, CLAMP)):
        tex = mipref.make_tex(C, tw, th, C, frames=2 if per_frame else None)
        L = full_levels(tex)
        gout = rand_gout(C, (2, C, h, w), own)
        gt, gm, gu = bwd(fs, vis, uv, uvd, gout, tex, mode, L)
        accs, want_gu = expect_bwd(tmp_path, frames, v, uvw, uvdw, gout, tex, mode, L)
        same(gu, want_gu, f"guv {tw}x{th}")
        check_levels(tmp_path, gt, gm, accs, tex.shape, L, f"{w}x{h} tex {tw}x{th} C {C}")
        gt2, gm2, _ = bwd(fs, vis, uv, uvd, gout, tex, mode, L, want_uv=False)
        check_levels(tmp_path, gt2, gm2, accs, tex.shape, L, f"{w}x{h} tex {tw}x{th} C {C} alone")
        if L > 1:
            assert (gm != 0).any()
    # accumulation into buffers that are not zero: one more term per element (the last texture: 1 x 1; then a pyramid)
    tex = mipref.make_tex(7, 32, 8, 5)
    rng = np.random.default_rng(4)
    init = (rng.normal(0, 5, tex.shape).astype(np.float32), rng.normal(0, 5, mipref.mip_floats(tmp_path, tex.shape, 6)).astype(np.float32))
    gout = rand_gout(7, (2, 5, h, w), own)
    gt, gm, _ = bwd(fs, vis, uv, uvd, gout, tex, WRAP, 6, want_uv=False, into=init)
    accs, _ = expect_bwd(tmp_path, frames, v, uvw, uvdw, gout, tex, WRAP, 6)
    check_levels(tmp_path, gt, gm, accs, tex.shape, 6, "into non-zero buffers", init=init)
    assert (gt != init[0]).any() and (gm != init[1]).any()
    fs.close()


@pytest.mark.parametrize("mode", [CLAMP, WRAP])
@pytest.mark.parametrize("C", [1, 5, 8])
@pytest.mark.parametrize("w,h,n,tw,th", [(96, 96, 2, 64, 32), (50, 37, 2, 16, 16), (64, 64, 9, 32, 8)])
def test_texel_gradients_exact_on_dyadic_inputs(ctx, tmp_path, mode, C, w, h, n, tw, th):
    """power-of-two textures; uv on eighths of a texel of the COARSER level a pixel touches, u = (i + 0.5 + k / 8) / w_l1 (hence on
    quarters at the finer one): tx and ty are multiples of 1/8 at both levels, the weights of 1/64; rho = 2^k or 1.5 * 2^k along one
    axis, so f is 0 or 0.5 and the level weights 1 or 0.5; integer gout in [-16, 16] and integer buffers to add into: every product
    and every partial sum is a small multiple of 2^-7, any order of adds gives the same bits"""
    rng = np.random.default_rng([C, w, mode, tw])
    L = mipref.levels(tmp_path, tw, th)
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    ids = rand_ids(rng, n, h, w, 20)
    v = hand_vis(ids)
    vis = torch.as_tensor(v).cuda()
    shape = (n, h, w)
    k = rng.integers(0, L + 1, shape)
    half = rng.integers(0, 2, shape)
    rho = np.exp2(k) * np.where(half == 1, 1.5, 1.0)
    axis = rng.integers(0, 2, shape)
    uvdw = np.zeros((n, 4, h, w), np.float32)
    uvdw[:, 0] = np.where(axis == 0, rho / tw, 0)
    uvdw[:, 3] = np.where(axis == 1, rho / th, 0)
    l0, f = mipref.lod(tmp_path, (th, tw), L, np.moveaxis(uvdw, 1, 0))
    assert set(np.unique(f).tolist()) == {0.0, 0.5} and len(set(l0.ravel().tolist())) == L
    l1 = np.minimum(l0 + (f != 0), L - 1).astype(np.int64)  # the coarser level the pixel touches
    sz = np.array(mipref.sizes(tmp_path, tw, th, L))  # [L, 2]: (w_l, h_l)
    lo = -2 if mode == WRAP else 0
    wl, hl = sz[l1, 0], sz[l1, 1]
    uvw = np.stack([(rng.integers(lo * wl, (1 - lo) * wl, shape) + 0.5 + rng.integers(0, 8, shape) / 8.0) / wl,
                    (rng.integers(lo * hl, (1 - lo) * hl, shape) + 0.5 + rng.integers(0, 8, shape) / 8.0) / hl], 1).astype(np.float32)
    uv, uvd = dev(uvw), dev(uvdw)
    shared = n != 2
    tex = rng.integers(-8, 9, ((th, tw, C) if shared else (n, th, tw, C))).astype(np.float32)
    gout = rng.integers(-16, 17, (n, C, h, w)).astype(np.float32)
    init = (rng.integers(-64, 65, tex.shape).astype(np.float32), rng.integers(-64, 65, mipref.mip_floats(tmp_path, tex.shape, L)).astype(np.float32))
    gt, gm, gu = bwd(fs, vis, uv, uvd, gout, tex, mode, L, fill=SENTINEL, into=init)
    accs, want_gu = expect_bwd(tmp_path, frames, v.view(np.uint32), uvw, uvdw, gout, tex, mode, L, fill=SENTINEL)
    same(gu, want_gu, "dyadic guv")
    check_levels(tmp_path, gt, gm, accs, tex.shape, L, f"dyadic {w}x{h} tex {tw}x{th} C {C} mode {mode}", exact=True, init=init)
    assert (gt != init[0]).any() and (gm != init[1]).any()
    same(fwd(fs, vis, uv, uvd, tex, mode, L), expect_fwd(tmp_path, frames, v.view(np.uint32), uvw, uvdw, tex, mode, L), "dyadic forward")
    fs.close()


def test_texel_gradients_of_a_minified_tile_land_on_level_3(ctx, tmp_path):
    """the minified regime of tests/test_gpu_texture.py's table test — a 256 x 256 texture across one 32 x 32 tile, where the bilinear
    pass's tile touches 4096 distinct texels of level 0, twice its table — with uvd set to that footprint (8 texels per pixel, rho = 8
    exactly): l0 = 3, f = 0, every add lands on the 32 x 32 level 3, whose 33 x 33 or fewer distinct texels fit the table"""
    w = h = 32
    n, C, tw, th, L = 2, 5, 256, 256, 9
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    uvw = np.stack([np.stack([(xs + 0.37) / 32, (ys + 0.61) / 32]).astype(np.float32)] * n)
    uvdw = np.zeros((n, 4, h, w), np.float32)
    uvdw[:, 0], uvdw[:, 3] = 1 / 32, 1 / 32
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    v = hand_vis(rand_ids(np.random.default_rng(31), n, h, w, 20, holes=False))
    vis, uv, uvd = torch.as_tensor(v).cuda(), dev(uvw), dev(uvdw)
    for tex in (mipref.make_tex(8, tw, th, C), mipref.make_tex(8, tw, th, C, frames=n)):
        gout = rand_gout(11, (n, C, h, w))
        gt, gm, gu = bwd(fs, vis, uv, uvd, gout, tex, CLAMP, L, fill=SENTINEL)
        accs, want_gu = expect_bwd(tmp_path, frames, v.view(np.uint32), uvw, uvdw, gout, tex, CLAMP, L, fill=SENTINEL)
        same(gu, want_gu, "minified guv")
        check_levels(tmp_path, gt, gm, accs, tex.shape, L, f"minified {tex.ndim}")
        per_level = [int(accs[0].level(l)[2].sum()) for l in range(L)]
        assert per_level == [0, 0, 0, 4 * w * h * (n if tex.ndim == 3 else 1)] + [0] * (L - 4) and (gt == 0).all() and (gm != 0).any()
        assert int((accs[0].level(3)[2] > 0).sum()) <= 33 * 33
    fs.close()


@pytest.mark.parametrize("mode", [CLAMP, WRAP])
def test_texel_gradients_past_the_table_add_straight_to_memory(ctx, tmp_path, mode):
    """the opposite regime (tests/test_gpu_cube.py's test_table_overflow): mipref.overflow_planes over four tiles a frame — every tile
    touches 4 096 distinct texels of level 0 against the table's 2 048 slots, in frame 1 next to a level 1 that fits —, so corners
    without a slot add straight to memory at level 0, with and without a second level; C = 5: two chunks, the second with a masked
    tail.  The bound is test_texel_gradients_on_rendered_buffers_and_accumulation's."""
    w = h = 64
    n, C, tw, th, L = 2, 5, 256, 256, 9
    uvw, uvdw = mipref.overflow_planes(w, h, tw, th)
    frames = hand_frames(w, h, n, 20)
    ids = rand_ids(np.random.default_rng(31), n, h, w, 20, holes=False)
    for i in range(n):  # every tile really exceeds the table at level 0; frame 1 adds into level 1 too
        per_tile = mipref.tile_texels(tmp_path, ids[i], uvw[i], uvdw[i], (th, tw), mode, L, 20)
        assert per_tile.shape == (2, 2, L) and (per_tile[..., 0] > mipref.TG_SLOTS).all() and (per_tile[..., 2:] == 0).all()
        assert ((per_tile[..., 1] > 0) == (i == 1)).all() and (per_tile[..., 1] <= mipref.TG_SLOTS).all()
    fs = ctx.frameset(frames)
    v = hand_vis(ids)
    vis, uv, uvd = torch.as_tensor(v).cuda(), dev(uvw), dev(uvdw)
    for tex in (mipref.make_tex(8, tw, th, C), mipref.make_tex(8, tw, th, C, frames=n)):
        gout = rand_gout(11, (n, C, h, w))
        gt, gm, gu = bwd(fs, vis, uv, uvd, gout, tex, mode, L, fill=SENTINEL)
        accs, want_gu = expect_bwd(tmp_path, frames, v.view(np.uint32), uvw, uvdw, gout, tex, mode, L, fill=SENTINEL)
        same(gu, want_gu, "overflow guv")
        check_levels(tmp_path, gt, gm, accs, tex.shape, L, f"overflow {tex.ndim} mode {mode}")
        assert (gt != 0).any() and (gm != 0).any()
    fs.close()


# ------------------------------------------------------------------------------------------------------ the chain, autograd
def test_guv_chains_into_interpolate_grad(ctx, tmp_path):
    frames, fs, vis, v, uv, uvd, attr = rendered(ctx, 100, 70, 120)
    uvw, uvdw = uv.cpu().numpy(), uvd.cpu().numpy()
    tex = mipref.make_tex(14, 96, 64, 4)
    gout = rand_gout(15, (2, 4, 70, 100), owners(v, frames))
    _, _, gu = bwd(fs, vis, uv, uvd, gout, tex, WRAP, 6, want_tex=False, fill=SENTINEL)
    want_gu = expect_bwd(tmp_path, frames, v, uvw, uvdw, gout, tex, WRAP, 6, fill=SENTINEL)[1]
    same(gu, want_gu, "guv")
    guv = torch.as_tensor(gu.view(np.float32)).cuda()
    gattr = torch.zeros(attr.shape, dtype=torch.float32, device="cuda")
    fs.interpolate_grad(vis.data_ptr(), guv.data_ptr(), None, 2, 2, attr.shape[1], gattr.data_ptr(), None, F, stream())
    torch.cuda.synchronize()
    got = gattr.cpu().numpy()
    for i, f in enumerate(frames):
        acc = interpref.Grad(attr.shape[1:])
        interpref.grad(tmp_path, attr[i], f.n_tris, v[i], want_gu[i], into=acc, want_bary=False)
        err = np.abs(got[i].astype(np.float64) - acc.gattr)
        assert (err <= acc.bound()).all() and (got[i][acc.count == 0] == 0).all() and (acc.gattr != 0).sum() > 100
    fs.close()


def folded_reference(tmp_path, acc, tw, th, L):
    """(the exact fold of an accumulator's level sums, its bound) in float64, per element of level 0.
    THE BOUND, derived: the pass leaves in level l a sum S^_l within b_l = gamma_(n_l) * sum |product| of the exact sum S_l of its
    float32 products (one rounding per add).  The fold computes acc_(L-1) = S^_(L-1) and acc_l = fl(k_(l+1) acc_(l+1) + S^_l), one
    rounding per fma (the product by a power of two is exact).  With A_l the exact fold of the exact sums, |A_l| <= M_l = k_(l+1)
    M_(l+1) + sum_l |product|, and E_l = |acc_l - A_l|:  E_(L-1) = b_(L-1);  E_l <= (1 + u) (k_(l+1) E_(l+1) + b_l) + u M_l — the
    per-level bounds carried through the fold's factors, plus one rounding per fma, u = 2^-24.  E_0 is the bound of tex.grad."""
    lv = [acc.level(l) for l in range(L)]

    def up(a, l):  # level l + 1's values under each texel of level l
        hl, wl = lv[l][0].shape[:2]
        return a[np.arange(hl) >> 1][:, np.arange(wl) >> 1]

    def gamma(cnt):
        nu = cnt.astype(np.float64)[:, :, None] * U
        return nu / (1.0 - nu)
    A, M, E = lv[L - 1][0].copy(), lv[L - 1][1].copy(), gamma(lv[L - 1][2]) * lv[L - 1][1]
    for l in range(L - 2, -1, -1):
        k = mipref.level(tmp_path, tw, th, l + 1)[2]
        b = gamma(lv[l][2]) * lv[l][1]
        A, M = k * up(A, l) + lv[l][0], k * up(M, l) + lv[l][1]
        E = (1 + U) * (k * up(E, l) + b) + U * M
    return A, E


def test_autograd(ctx, tmp_path, monkeypatch):
    """texture_mip(fs, vis, tex, interpolate(fs, vis, a), interpolate_deriv(fs, vis, a).detach()) backpropagates to tex and to a:
    tex.grad within folded_reference's bound (derived there), a.grad within interpref's; exactly one texture_mip_grad call and one
    fold per backward, no call when nothing requires a gradient"""
    import srz
    from srz.visibility import interpolate, interpolate_deriv, mip_build, mip_views, texture_mip, texture_mip_grad
    frames, fs, vis, v, uv, uvd, attr = rendered(ctx, 100, 70, 120)
    uvw, uvdw = uv.cpu().numpy(), uvd.cpu().numpy()
    calls = {"grad": 0, "fold": 0, "build": 0}
    real_grad, real_fold, real_build = srz.FrameSet.texture_mip_grad, srz.Context.mip_fold, srz.Context.mip_build
    monkeypatch.setattr(srz.FrameSet, "texture_mip_grad", lambda self, *a, **k: (calls.__setitem__("grad", calls["grad"] + 1), real_grad(self, *a, **k))[1])
    monkeypatch.setattr(srz.Context, "mip_fold", lambda self, *a, **k: (calls.__setitem__("fold", calls["fold"] + 1), real_fold(self, *a, **k))[1])
    monkeypatch.setattr(srz.Context, "mip_build", lambda self, *a, **k: (calls.__setitem__("build", calls["build"] + 1), real_build(self, *a, **k))[1])
    a = dev(attr).requires_grad_(True)
    same(words(interpolate_deriv(fs, vis, a)), words(uvd), "interpolate_deriv")
    assert not interpolate_deriv(fs, vis, a).requires_grad
    for wrap, shape in ((False, (64, 96, 3)), (True, (2, 8, 32, 5))):
        texn = np.random.default_rng(16).normal(0, 3, shape).astype(np.float32)
        tw, th, L = shape[-2], shape[-3], 6
        tex = dev(texn).requires_grad_(True)
        a.grad = None
        before = dict(calls)
        out = texture_mip(fs, vis, tex, interpolate(fs, vis, a), interpolate_deriv(fs, vis, a).detach(), wrap=wrap)
        assert out.requires_grad and calls["build"] == before["build"] + 1
        same(words(out.detach()), fwd(fs, vis, uv, uvd, texn, int(wrap), L), "forward")
        # the pyramid as views
        lv = mip_views(mip_build(fs, tex.detach()), tex.shape)
        want_lv = mipref.views(tmp_path, mipref.build(tmp_path, texn, L), texn.shape, L)
        assert len(lv) == L - 1 and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(lv, want_lv))
        before = dict(calls)
        out.square().sum().backward()
        torch.cuda.synchronize()
        assert calls["grad"] == before["grad"] + 1 and calls["fold"] == before["fold"] + 1 and calls["build"] == before["build"]
        g = (2 * out.detach()).contiguous().cpu().numpy()  # float32: what the backward was handed
        accs, want_gu = expect_bwd(tmp_path, frames, v, uvw, uvdw, g, texn, int(wrap), L)
        tg = tex.grad.cpu().numpy().reshape((-1,) + shape[-3:])
        for i, acc in enumerate(accs):
            ref, bound = folded_reference(tmp_path, acc, tw, th, L)
            err = np.abs(tg[i].astype(np.float64) - ref)
            print(f"tex.grad {shape}: max err {err.max():.3e}, max err / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}")
            assert (err <= bound).all() and (tg[i] != 0).sum() > 100
        got = a.grad.cpu().numpy()
        for i, f in enumerate(frames):
            acc = interpref.Grad(attr.shape[1:])
            interpref.grad(tmp_path, attr[i], f.n_tris, v[i], want_gu[i], into=acc, want_bary=False)
            assert (np.abs(got[i].astype(np.float64) - acc.gattr) <= acc.bound()).all() and (got[i] != 0).sum() > 100
        # the plain call: the same guv, gtex within the same bound, the parts apart with fold=False
        gt, gu = texture_mip_grad(fs, vis, tex.detach(), uv, uvd, dev(g), wrap=wrap)
        same(words(gu), want_gu, "plain guv")
        ref, bound = folded_reference(tmp_path, accs[0], tw, th, L)
        assert (np.abs(gt.cpu().numpy().reshape(tg.shape)[0].astype(np.float64) - ref) <= bound).all()
        gt0, gm0, gu0 = texture_mip_grad(fs, vis, tex.detach(), uv, uvd, dev(g), wrap=wrap, want_guv=False, fold=False)
        assert gu0 is None
        check_levels(tmp_path, gt0.cpu().numpy(), gm0.cpu().numpy(), accs, texn.shape, L, "plain call, not folded")
    # nothing needs a gradient: no backward is there to launch; one input does: the call asks for that output alone
    before = dict(calls)
    out = texture_mip(fs, vis, tex.detach(), uv, uvd, wrap=True)
    assert not out.requires_grad and out.grad_fn is None
    uvt = uv.clone().requires_grad_(True)
    texture_mip(fs, vis, tex.detach(), uvt, uvd, wrap=True).sum().backward()
    torch.cuda.synchronize()
    assert calls["grad"] == before["grad"] + 1 and calls["fold"] == before["fold"] and uvt.grad is not None
    t2 = tex.detach().clone().requires_grad_(True)
    texture_mip(fs, vis, t2, uv, uvd, wrap=True, n_levels=1).sum().backward()  # one level: no pyramid, no fold
    assert calls["grad"] == before["grad"] + 2 and calls["fold"] == before["fold"] and t2.grad is not None
    fs.close()
