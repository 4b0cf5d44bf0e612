"""-m gpu: the mipmapped cube lookup by direction and level and its gradients (srz_cube_mip_build / _fold,
srz_frameset_texture_cube_mip / _texture_cube_mip_grad, srz_frameset_cube_level; k_cube_mip, k_cube_mip_grad, k_cube_level).  The
expected values are tests/cubemipref.py's binary32 build on the very buffers the GPU read (pinned on the CPU by
tests/test_cubemip_ref.py).  Forward, gdir, glam and the footprint level: a NaN on one side must be a NaN on the other, every other
word matches bit for bit.  gtex / gmip: exact where every partial sum is representable (the dyadic case) and where an element has one
contributing add, else within gamma_n * sum |product|, gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing adds (+ 1
when the buffer held a value) — one rounding per add, the products being float32 products on both sides: derived, not measured."""
import numpy as np
import pytest
import torch

import cubemipref
import cuberef
from srz import abi, parallel
from support import SENTINEL, ctx, filled, frame, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
W, H = 96, 72  # three tile columns, two full tile rows and a partial one
CUBE_SIZES = (1, 2, 4, 6, 8, 64)
TG_SLOTS = 2048  # the capacity of k_cube_mip_grad's table of distinct texels per tile


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


def n_tris(f):
    return f if isinstance(f, int) else sum(len(t) for t in f.tris)


def hand_frames(w, h, n, tris, flags=F):
    return [frame(soup(1, tris, w, h, ZS), w, h, flags=flags) for _ in range(n)]


def hand_vis(ids):
    """a visibility buffer [n, 4, h, w] float32 with these id words (z, alpha, beta: zeros — the cube passes read none of them)"""
    v = np.zeros((ids.shape[0], 4) + ids.shape[1:], np.float32)
    v[:, 1] = ids.view(np.float32)
    return v


def rand_ids(rng, n, h, w, tris, holes=True):
    ids = rng.integers(1, tris + 1, (n, h, w)).astype(np.uint32)
    ids |= (rng.random((n, h, w)) < 0.4).astype(np.uint32) << 31
    if holes:
        ids[rng.random((n, h, w)) < 0.1] = 0
    return ids


def owners(v, frames):
    return np.stack([((v[i, 1] & 0x7fffffff) - np.uint32(1)) < n_tris(f) for i, f in enumerate(frames)])


def rand_levels(seed, N, C, L, frames=None):
    """a pyramid of the caller's own: every level independent noise (the lookup takes whatever it is handed)"""
    rng = np.random.default_rng([seed, N, C, L])
    lead = () if frames is None else (frames,)
    return [rng.normal(0, 3, lead + (6, N >> l, N >> l, C)).astype(np.float32) for l in range(L)]


def of_frame(levels, i):
    return [l[i] if l.ndim == 5 else l for l in levels]


def fwd(fs, vis, dirs, lam, levels, flags=F, fill=0):
    """the forward pass into a buffer prefilled with the word `fill` → uint32 [n, C, rows, W]"""
    t, L = dev(levels[0]), len(levels)
    tf, N, C = (t.shape[0] if t.dim() == 5 else 1), t.shape[-2], t.shape[-1]
    mip = dev(cubemipref.flat(levels, 1)) if L > 1 else None
    out = filled(fs.interpolate_shape(C), fill)
    fs.texture_cube_mip(vis.data_ptr(), dirs.data_ptr(), ptr(lam), t.data_ptr(), N, C, tf, ptr(mip), L, out.data_ptr(), fs.interpolate_bytes(C),
                        flags, stream())
    torch.cuda.synchronize()
    return words(out)


def bwd(fs, vis, dirs, lam, gout, levels, want_tex=True, want_dir=True, want_lam=True, flags=F, fill=0, into=None):
    """the backward pass → (the pyramid's gradient as a list of levels, float32, added into `into` (a list of levels) or zeros; gdir
    uint32 [n, 3, rows, W]; glam uint32 [n, 1, rows, W], both from `fill`)"""
    t, L, g = dev(levels[0]), len(levels), dev(gout)
    tf, N, C = (t.shape[0] if t.dim() == 5 else 1), t.shape[-2], t.shape[-1]
    mip = dev(cubemipref.flat(levels, 1)) if L > 1 else None
    gt = gm = None
    if want_tex:
        gt = torch.zeros_like(t) if into is None else dev(into[0])
        if L > 1:
            gm = torch.zeros_like(mip) if into is None else dev(cubemipref.flat(into, 1))
    gd = filled(fs.interpolate_shape(3), fill) if want_dir else None
    gl = filled(fs.interpolate_shape(1), fill) if want_lam else None
    fs.texture_cube_mip_grad(vis.data_ptr(), dirs.data_ptr(), ptr(lam), g.data_ptr(), t.data_ptr(), ptr(mip), N, C, tf, L, ptr(gt), ptr(gm), ptr(gd),
                             ptr(gl), flags, stream())
    torch.cuda.synchronize()
    glev = None
    if want_tex:
        glev, off, flat = [gt.cpu().numpy()], 0, gm.cpu().numpy() if gm is not None else None
        for l in levels[1:]:
            glev.append(flat[off:off + l.size].reshape(l.shape))
            off += l.size
    return glev, (words(gd) if want_dir else None), (words(gl) if want_lam else None)


def expect_fwd(tmp_path, frames, v, dw, lw, levels, fused=True, fill=0):
    out = []
    for i, f in enumerate(frames):
        pre = np.full((levels[0].shape[-1],) + v.shape[2:], fill, np.uint32)
        out.append(cubemipref.forward(tmp_path, of_frame(levels, i), n_tris(f), v[i, 1], dw[i], None if lw is None else lw[i, 0], fused, pre))
    return np.stack(out)


def expect_bwd(tmp_path, frames, v, dw, lw, gout, levels, fused=True, fill=0):
    """(Grad per cube frame — one for a shared cube —, gdir [n, 3, rows, W], glam [n, 1, rows, W])"""
    shared = levels[0].ndim == 4
    N, C, L = levels[0].shape[-2], levels[0].shape[-1], len(levels)
    accs = [cubemipref.Grad(N, C, L) for _ in range(1 if shared else len(frames))]
    gd, gl = [], []
    for i, f in enumerate(frames):
        a, b = cubemipref.grad(tmp_path, of_frame(levels, i), n_tris(f), v[i, 1], dw[i], None if lw is None else lw[i, 0], gout[i],
                               accs[0 if shared else i], fused=fused, prefill=fill)
        gd.append(a), gl.append(b[None])
    return accs, np.stack(gd), np.stack(gl)


def check_gpyr(got, accs, what, exact=False, init=None):
    """got: the list of gradient levels; init: what the buffers held before the call (one more term of every element's sum)"""
    for l, g in enumerate(got):
        ref = np.stack([a.level(a.g, l) for a in accs]).reshape(g.shape)
        mag = np.stack([a.level(a.gabs, l) for a in accs]).reshape(g.shape)
        cnt = np.stack([np.broadcast_to(a.level(a.count, l)[..., None], a.level(a.g, l).shape) for a in accs]).reshape(g.shape).astype(np.float64)
        if init is not None:
            ref, mag, cnt = ref + init[l].astype(np.float64), mag + np.abs(init[l].astype(np.float64)), cnt + 1
        assert np.isfinite(ref).all()
        nu = cnt * 2.0 ** -24
        bound = nu / (1.0 - nu) * mag
        if exact:
            assert (ref.astype(np.float32).astype(np.float64) == ref).all(), "the case is not dyadic"
            bound = np.zeros_like(bound)
        err = np.abs(g.astype(np.float64) - ref)
        print(f"{what} level {l}: max err {err.max():.3e}, max err / bound {np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0:.3f}, "
              f"max n {int(cnt.max())}, elements with one add {int((cnt == 1).sum())}, untouched {int((cnt == 0).sum())}")
        bad = ~(err <= bound)
        assert not bad.any(), f"{what} level {l}: {int(bad.sum())} elements beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
        one = cnt == 1
        same((g + np.float32(0))[one], (ref.astype(np.float32) + np.float32(0))[one], f"{what} level {l} (n = 1)")
        assert (g[cnt == 0] == (0 if init is None else init[l][cnt == 0])).all()


def rand_gout(seed, shape, own=None):
    g = np.random.default_rng([seed, 8]).normal(0, 2, shape).astype(np.float32)
    if own is not None:
        g[np.broadcast_to(~own[:, None], g.shape)] = np.nan  # nobody's words may hold anything
    return g


# ------------------------------------------------------------------------------------------------------ the pyramid
@pytest.mark.parametrize("n", CUBE_SIZES)
def test_build_and_fold_are_the_2d_passes_on_the_reshaped_cube(ctx, n):
    import srz
    from srz import visibility as V
    for C, tf in ((1, None), (5, 3)):
        cube = cuberef.make_cube(n, n, C, frames=tf)
        t = dev(cube)
        L = srz.cube_mip_levels(n)
        mip = V.cube_mip_build(ctx, t)
        as2d = t.reshape(-1, n, n, C)
        assert torch.equal(mip, V.mip_build(ctx, as2d)) and mip.numel() * 4 == srz.cube_mip_bytes(n, C, tf or 1, L)
        views = V.cube_mip_views(mip, cube.shape)
        ref = cubemipref.build(cube)
        assert len(views) == L - 1
        for l, v in enumerate(views, 1):
            same(v.cpu().numpy(), ref[l], f"n {n} level {l}")
        for Lp in {1, max(1, L - 1)}:  # fewer levels than there are
            part = V.cube_mip_build(ctx, t, Lp)
            assert torch.equal(part, mip[:part.numel()]) and part.numel() * 4 == srz.cube_mip_bytes(n, C, tf or 1, Lp)
        gmip = dev(np.random.default_rng(n).normal(0, 1, mip.shape))
        g0 = dev(np.random.default_rng(n + 1).normal(0, 1, cube.shape))
        a, b = g0.clone(), g0.clone().reshape(-1, n, n, C)
        ctx.cube_mip_fold(gmip.data_ptr(), mip.numel() * 4, n, C, tf or 1, L, a.data_ptr(), stream())
        ctx.mip_fold(gmip.data_ptr(), mip.numel() * 4, n, n, C, 6 * (tf or 1), L, b.data_ptr(), stream())
        torch.cuda.synchronize()
        assert torch.equal(a.reshape(b.shape), b) and (L == 1 or not torch.equal(a, g0))


# ------------------------------------------------------------------------------------------------------ forward, gdir, glam, gtex
def hostile_planes(rng, n, N, L):
    """direction and level planes [n, 3, H, W], [n, 1, H, W] by hand: rows 0 .. 29 the twelve edges (cuberef.edge_dirs) and the eight
    vertices at every level and half level; below them cuberef.hostile_dirs (every face, edges from both sides, vertex regions, ties,
    +-0, NaN, inf, zero, subnormal) under cubemipref.hostile_lam (every clamp, integers, fractions, NaN, +-inf)"""
    dw = np.stack([cuberef.hostile_dirs(rng, (H, W), N) for _ in range(n)])
    lw = np.stack([cubemipref.hostile_lam(rng, (1, H, W), L) for _ in range(n)])
    e = cuberef.edge_dirs()[0]
    corners = np.float32([(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)])
    strip = np.concatenate([e, corners, e * np.float32(0.37), corners * np.float32(3)])[:30 * W // 4 * 4]
    k = 30 * W
    idx = np.arange(k)
    dw[:, :, :30] = strip[idx % len(strip)].T.reshape(3, 30, W)
    lw[:, 0, :30] = (np.float32(0.5) * ((idx // len(strip) + idx) % (2 * L))).reshape(30, W)
    return np.ascontiguousarray(dw), np.ascontiguousarray(lw)


@pytest.mark.parametrize("N", CUBE_SIZES)
def test_hand_written_planes_every_cube_size(ctx, tmp_path, N):
    """hostile directions and levels under a hand-written visibility buffer with holes, a tile of unsampled owners and a tile of
    nobody (nothing to add there); 1, 5 (one above ATTR_CHUNK) and 17 channels, shared and per-frame pyramids of the caller's own,
    with and without the fused clear onto prefilled buffers; into gradient buffers that are not zero; each output alone"""
    n, L = 2, cubemipref.n_levels(N)
    rng = np.random.default_rng([N, 43])
    ids = rand_ids(rng, n, H, W, 20)
    dw, lw = hostile_planes(rng, n, N, L)
    ids[:, 32:64, 32:64] = 0     # a tile of nobody
    dw[:, :, 32:64, 0:32] = np.nan  # a tile whose owners are not sampled
    C = (1, 5, 17)[CUBE_SIZES.index(N) % 3]
    for flags in (F, 0):
        frames = hand_frames(W, H, n, 20, flags)
        fs = ctx.frameset(frames)
        v = hand_vis(ids)
        vw = v.view(np.uint32)
        vis = torch.as_tensor(v).cuda()
        own = owners(vw, frames)
        if flags == F:
            cls = np.stack([cubemipref.classify(tmp_path, N, L, 20, ids[i], dw[i], lw[i, 0])[0] for i in range(n)])
            smp = (cls & cubemipref.SAMPLED) != 0
            assert (own & ~smp).sum() >= 1000 and smp.sum() >= 6000
            if L > 1:
                for bit in (cubemipref.CLAMP_LOW, cubemipref.CLAMP_HIGH, cubemipref.FRACTIONAL):
                    assert ((cls & bit) != 0).sum() >= 300, bit
                assert ((cls & cubemipref.CROSSED_ABOVE0) != 0).sum() >= 200
        d2 = dw.copy()
        d2[np.broadcast_to(~own[:, None], dw.shape)] = np.nan  # never read
        l2 = lw.copy()
        l2[~own[:, None]] = np.nan
        dirs, lam = dev(d2), dev(l2)
        fused = flags == F
        for levels in (rand_levels(N, N, C, L), rand_levels(N + 1, N, C, L, frames=n)):
            what = f"N {N} C {C} L {L} {levels[0].ndim} fused {fused}"
            got = fwd(fs, vis, dirs, lam, levels, flags, SENTINEL)
            same(got, expect_fwd(tmp_path, frames, vw, d2, l2, levels, fused, SENTINEL), what)
            assert (got[np.broadcast_to(~own[:, None], got.shape)] == (0 if fused else SENTINEL)).all()
            gout = rand_gout(N, got.shape, own)
            init = [np.random.default_rng(l.size).normal(0, 5, l.shape).astype(np.float32) for l in levels]
            gp, gd, gl = bwd(fs, vis, dirs, lam, gout, levels, flags=flags, fill=SENTINEL, into=init)
            accs, want_gd, want_gl = expect_bwd(tmp_path, frames, vw, d2, l2, gout, levels, fused, SENTINEL)
            same(gd, want_gd, what + " gdir")
            same(gl, want_gl, what + " glam")
            check_gpyr(gp, accs, what + " gtex/gmip into a non-zero buffer", init=init)
            if fused and levels[0].ndim == 4:  # each output alone; zeros to add into
                assert np.array_equal(bwd(fs, vis, dirs, lam, gout, levels, want_tex=False, want_lam=False, fill=SENTINEL)[1], gd)
                assert np.array_equal(bwd(fs, vis, dirs, lam, gout, levels, want_tex=False, want_dir=False, fill=SENTINEL)[2], gl)
                check_gpyr(bwd(fs, vis, dirs, lam, gout, levels, want_dir=False, want_lam=False)[0], accs, what + " gtex/gmip alone")
        fs.close()


@pytest.mark.parametrize("N", CUBE_SIZES)
def test_one_level_is_texture_cube_bit_for_bit(ctx, tmp_path, N):
    """n_levels == 1: neither d_lam nor d_mip is read (null, or a plane of NaN), and every output is the flat pass's"""
    n, C = 2, 5
    rng = np.random.default_rng([N, 47])
    frames = hand_frames(W, H, n, 20)
    fs = ctx.frameset(frames)
    ids = rand_ids(rng, n, H, W, 20)
    vw = hand_vis(ids).view(np.uint32)
    vis = torch.as_tensor(hand_vis(ids)).cuda()
    dw = np.stack([cuberef.hostile_dirs(rng, (H, W), N) for _ in range(n)])
    dirs = dev(dw)
    nan_lam = dev(np.full((n, 1, H, W), np.nan))
    for cube in (cuberef.make_cube(N, N, C), cuberef.make_cube(N, N, C, frames=n)):
        t, g = dev(cube), dev(rand_gout(N, (n, C, H, W)))
        tf = n if cube.ndim == 5 else 1
        flat_out = filled(fs.interpolate_shape(C), SENTINEL)
        fs.texture_cube(vis.data_ptr(), dirs.data_ptr(), t.data_ptr(), N, C, tf, flat_out.data_ptr(), fs.interpolate_bytes(C), F, stream())
        flat_gd, flat_gt = filled(fs.interpolate_shape(3), SENTINEL), torch.zeros_like(t)
        fs.texture_cube_grad(vis.data_ptr(), dirs.data_ptr(), g.data_ptr(), t.data_ptr(), N, C, tf, None, flat_gd.data_ptr(), F, stream())
        fs.texture_cube_grad(vis.data_ptr(), dirs.data_ptr(), g.data_ptr(), t.data_ptr(), N, C, tf, flat_gt.data_ptr(), None, F, stream())
        for lam in (None, nan_lam):
            same(fwd(fs, vis, dirs, lam, [cube], F, SENTINEL), words(flat_out), f"N {N} forward")
            gp, gd, gl = bwd(fs, vis, dirs, lam, g.cpu().numpy(), [cube], fill=SENTINEL)
            same(gd, words(flat_gd), f"N {N} gdir")
            assert (gl == 0).all()  # (every pixel written: the fused clear; L == 1 has no level gradient)
            # gtex: the flat pass's terms, in whatever order: both lie within the bound of the one-level reference's sums
            accs = expect_bwd(tmp_path, frames, vw, dw, None, g.cpu().numpy(), [cube], fill=SENTINEL)[0]
            check_gpyr(gp, accs, f"N {N} gtex")
            check_gpyr([flat_gt.cpu().numpy()], accs, f"N {N} the flat pass's gtex")
    fs.close()


def dyadic_dirs(rng, shape):
    """directions whose major component is +-1, +-2 or +-0.5 and whose others are k / 16 of it: s and t are k / 16 exactly"""
    d = np.zeros(shape + (3,), np.float32)
    m = rng.integers(0, 3, shape)
    major = rng.choice(np.float32([1, -1, 2, -2, 0.5, -0.5]), shape)
    a, b = rng.integers(-16, 17, shape), rng.integers(-16, 17, shape)
    for ax in range(3):
        sel = m == ax
        d[sel, ax] = major[sel]
        d[sel, (ax + 1) % 3] = np.abs(major[sel]) * a[sel] / 16
        d[sel, (ax + 2) % 3] = np.abs(major[sel]) * b[sel] / 16
    return d


@pytest.mark.parametrize("n", [2, 9])
def test_gtex_and_gmip_exact_on_dyadic_inputs(ctx, tmp_path, n):
    """N = 8, two levels, s and t multiples of 1 / 16 (edges, ties and vertices among them), lam in {0, 1/2, 1}, integer gout in
    [-16, 16], integer buffers to add into: the weights are multiples of 1 / 16 at level 0 and of 1 / 64 at level 1, the level weight
    of 1 / 2, so every product is a multiple of 2^-7 below 2^5 and every partial sum of the at most 4 n W H of them stays below 2^17:
    24 bits, representable — any order of adds gives the same bits.  Nine frames: the walk's other branch (frame = workgroup mod 8),
    the table handed from tile to tile"""
    rng = np.random.default_rng([n, 3])
    w = h = 64
    C = 5
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    ids = rand_ids(rng, n, h, w, 20)
    v = hand_vis(ids)
    vis = torch.as_tensor(v).cuda()
    dw = np.ascontiguousarray(dyadic_dirs(rng, (n, h, w)).transpose(0, 3, 1, 2))
    lw = rng.choice(np.float32([0, 0.5, 0.5, 1]), (n, 1, h, w))
    shared = n != 2
    lead = () if shared else (n,)
    levels = [rng.integers(-8, 9, lead + (6, 8 >> l, 8 >> l, C)).astype(np.float32) for l in range(2)]
    gout = rng.integers(-16, 17, (n, C, h, w)).astype(np.float32)
    init = [rng.integers(-64, 65, l.shape).astype(np.float32) for l in levels]
    gp, gd, gl = bwd(fs, vis, dev(dw), dev(lw), gout, levels, fill=SENTINEL, into=init)
    accs, want_gd, want_gl = expect_bwd(tmp_path, frames, v.view(np.uint32), dw, lw, gout, levels, fill=SENTINEL)
    same(gd, want_gd, "dyadic gdir")
    same(gl, want_gl, "dyadic glam")
    check_gpyr(gp, accs, f"dyadic n {n}", exact=True, init=init)
    assert (gp[0] != init[0]).any() and (gp[1] != init[1]).any()
    same(fwd(fs, vis, dev(dw), dev(lw), levels), expect_fwd(tmp_path, frames, v.view(np.uint32), dw, lw, levels), "dyadic forward")
    fs.close()


def test_table_overflow_with_both_levels_fractional(ctx, tmp_path):
    """independent random directions per pixel on N = 64 over one 32 x 32 tile, every lam fractional: up to 4 096 distinct texels of
    level l0 and as many of level l0 + 1 against the table's 2 048 slots — the corners without a slot add straight to memory, at both
    levels, and the bound still holds"""
    w = h = 32
    n, C, N, L = 2, 5, 64, 3
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    rng = np.random.default_rng(31)
    ids = rand_ids(rng, n, h, w, 20, holes=False)
    v = hand_vis(ids)
    vis = torch.as_tensor(v).cuda()
    dw = rng.normal(0, 1, (n, 3, h, w)).astype(np.float32)
    lw = rng.uniform(0.1, 0.9, (n, 1, h, w)).astype(np.float32)
    lw[1] += 1  # frame 1: levels 1 and 2
    for levels in (rand_levels(8, N, C, L), rand_levels(9, N, C, L, frames=n)):
        gout = rand_gout(11, (n, C, h, w))
        gp, gd, gl = bwd(fs, vis, dev(dw), dev(lw), gout, levels, fill=SENTINEL)
        accs, want_gd, want_gl = expect_bwd(tmp_path, frames, v.view(np.uint32), dw, lw, gout, levels, fill=SENTINEL)
        if levels[0].ndim == 5:  # the tile really exceeds the table (counted from the reference's own adds: each names its texel)
            assert int((accs[0].count > 0).sum()) > TG_SLOTS and int(accs[0].count.sum()) == 8 * w * h
            assert int((accs[0].level(accs[0].count, 0) > 0).sum()) > TG_SLOTS and int((accs[0].level(accs[0].count, 1) > 0).sum()) > TG_SLOTS // 2
        same(gd, want_gd, "overflow gdir")
        same(gl, want_gl, "overflow glam")
        check_gpyr(gp, accs, f"overflow {levels[0].ndim}")
        assert all((g != 0).any() for g in gp)
    fs.close()


# ------------------------------------------------------------------------------------------------------ a geometric scene
def sphere_frames(w, h, radius, rings=14, segs=40, flags=F):
    """two frames of one sphere-like mesh (the front hemisphere, orthographic), its unit normals the directions: frame 0 seen from
    +z, frame 1 the same triangles with the normals mirrored in z — together every face of the cube, the rims at grazing angles"""
    th = np.linspace(0, np.pi / 2, rings + 1)
    ph = np.linspace(0, 2 * np.pi, segs, endpoint=False)
    p = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(segs))], -1)  # [ring][seg][3]
    tris = []
    for i in range(rings):
        for j in range(segs):
            j2 = (j + 1) % segs
            quad = [p[i, j], p[i + 1, j], p[i + 1, j2], p[i, j2]]
            for a, b, c in ((quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])):
                if i == 0 and np.allclose(a, c) or np.allclose(a, b) or np.allclose(b, c):
                    continue
                tris.append((a, b, c))
    out = []
    for mirror in (1.0, -1.0):
        t = np.zeros(len(tris), abi.TRI_DTYPE)
        for k, (a, b, c) in enumerate(tris):
            xy = np.float32([(w / 2 + 0.3 + radius * q[0], h / 2 - 0.2 + radius * q[1]) for q in (a, b, c)])
            e1, e2 = xy[1] - xy[0], xy[2] - xy[0]
            order = [0, 1, 2] if e1[0] * e2[1] - e1[1] * e2[0] < 0 else [0, 2, 1]  # support.ccw's winding
            for s, o in enumerate(order):
                q = (a, b, c)[o]
                t["pos"][k, s] = (xy[o][0], xy[o][1], 50 - 20 * q[2])
                t["nrm"][k, s] = (q[0], q[1], mirror * q[2])
        out.append(frame(t, w, h, flags=flags))
    return out


def test_footprint_level_and_lookup_on_a_sphere(ctx, tmp_path):
    """cube_level from the GPU's own interpolate / interpolate_deriv planes of a sphere's normals is the reference's level bit for
    bit, and the lookup at that level the reference's lookup; checked on the reference's classification first, so the test cannot
    pass while exercising one branch only"""
    N, L, C = 64, 4, 3
    frames = sphere_frames(W, H, 33.0)
    n, T = len(frames), n_tris(frames[0])
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    attr = np.stack([np.concatenate([t["nrm"] for t in f.tris]) for f in frames]).astype(np.float32)
    a_dev = dev(attr)
    dirs = torch.zeros(fs.interpolate_shape(3), dtype=torch.float32, device="cuda")
    dird = torch.zeros(fs.interpolate_shape(6), dtype=torch.float32, device="cuda")
    fs.interpolate(vis.data_ptr(), a_dev.data_ptr(), 3, n, T, dirs.data_ptr(), fs.interpolate_bytes(3), F, stream())
    fs.interpolate_deriv(vis.data_ptr(), a_dev.data_ptr(), 3, n, T, dird.data_ptr(), fs.interpolate_bytes(6), F, stream())
    lam = filled(fs.interpolate_shape(1), SENTINEL)
    fs.cube_level(vis.data_ptr(), dirs.data_ptr(), dird.data_ptr(), N, L, lam.data_ptr(), fs.interpolate_bytes(1), F, stream())
    torch.cuda.synchronize()
    dw, ddw, lw = dirs.cpu().numpy(), dird.cpu().numpy(), lam.cpu().numpy().view(np.float32)
    want_lam = np.stack([cubemipref.level(tmp_path, N, L, T, v[i, 1], dw[i], ddw[i], prefill=SENTINEL)[None] for i in range(n)])
    same(lw, want_lam, "cube_level")
    own = owners(v, frames)
    cls, face, l0, f = (np.stack(x) for x in zip(*(cubemipref.classify(tmp_path, N, L, T, v[i, 1], dw[i], lw[i, 0]) for i in range(n))))
    smp = (cls & cubemipref.SAMPLED) != 0
    assert own.sum() >= 5000 and (smp == own).all()
    assert ((cls & cubemipref.FRACTIONAL) != 0).sum() >= own.sum() / 4
    assert ((cls & cubemipref.CLAMP_LOW) != 0).any() and ((cls & cubemipref.CLAMP_HIGH) != 0).any()
    assert (((cls & (cubemipref.CLAMP_LOW | cubemipref.CLAMP_HIGH)) == 0) & smp).any()
    assert set(face[smp]) == set(range(6)) and ((cls & cubemipref.CROSSED_ABOVE0) != 0).any()
    assert set(l0[smp]) == set(range(L))
    # without the fused clear (a set of the same frames that do not clear) nobody's words stay
    fs0 = ctx.frameset(sphere_frames(W, H, 33.0, flags=0))
    kept = filled(fs0.interpolate_shape(1), SENTINEL)
    fs0.cube_level(vis.data_ptr(), dirs.data_ptr(), dird.data_ptr(), N, L, kept.data_ptr(), fs0.interpolate_bytes(1), 0, stream())
    torch.cuda.synchronize()
    fs0.close()
    kw = words(kept)
    assert (kw[~own[:, None]] == SENTINEL).all() and np.array_equal(kw[own[:, None]], lw.view(np.uint32)[own[:, None]])
    cube = cuberef.make_cube(5, N, C)
    levels = cubemipref.build(cube, L)  # the box-filtered pyramid, as the GPU builds it (test_build_and_fold pins that)
    got = fwd(fs, vis, dirs, lam, levels, F, SENTINEL)
    same(got, expect_fwd(tmp_path, frames, v, dw, lw, levels, True, SENTINEL), "lookup at the footprint level")
    gout = rand_gout(2, got.shape, own)
    gp, gd, gl = bwd(fs, vis, dirs, lam, gout, levels, fill=SENTINEL)
    accs, want_gd, want_gl = expect_bwd(tmp_path, frames, v, dw, lw, gout, levels, True, SENTINEL)
    same(gd, want_gd, "sphere gdir")
    same(gl, want_gl, "sphere glam")
    check_gpyr(gp, accs, "sphere gtex/gmip")
    fs.close()


# ------------------------------------------------------------------------------------------------------ sharded
def test_sharded_world_3(ctx, tmp_path):
    """three ranks, one band of the 72 rows each: every rank's rows of the forward, of gdir and of glam are the whole frame's rows, and
    the ranks' partial texel sums add up to the whole frame's within the bound"""
    import srz
    N, L, C, n = 8, 4, 5, 2
    rng = np.random.default_rng(77)
    frames = hand_frames(W, H, n, 20)
    ids = rand_ids(rng, n, H, W, 20)
    dw, lw = hostile_planes(rng, n, N, L)
    levels = rand_levels(3, N, C, L)
    gout = rand_gout(13, (n, C, H, W))
    accs, want_gd, want_gl = expect_bwd(tmp_path, frames, hand_vis(ids).view(np.uint32), dw, lw, gout, levels)
    want = expect_fwd(tmp_path, frames, hand_vis(ids).view(np.uint32), dw, lw, levels)
    total = [np.zeros(l.shape, np.float64) for l in levels]
    for rank in range(3):
        c = srz.Context(0, rank, 3)
        sfs = c.frameset(frames)
        rows = parallel.band_rows(H, rank, 3)
        assert len(rows) == 1

        def local(a):
            out = np.zeros(a.shape[:2] + (sfs.local_rows, W), a.dtype)
            for (lb, _, r0, r1) in rows:
                out[:, :, lb * 32: lb * 32 + r1 - r0] = a[:, :, r0:r1]
            return out
        svis, sdirs, slam = torch.as_tensor(local(hand_vis(ids))).cuda(), dev(local(dw)), dev(local(lw))
        shard = fwd(sfs, svis, sdirs, slam, levels)
        part, part_gd, part_gl = bwd(sfs, svis, sdirs, slam, local(gout), levels)
        for (lb, _, r0, r1) in rows:
            sl = slice(lb * 32, lb * 32 + r1 - r0)
            same(shard[:, :, sl], want[:, :, r0:r1], f"rank {rank} forward")
            same(part_gd[:, :, sl], want_gd[:, :, r0:r1], f"rank {rank} gdir")
            same(part_gl[:, :, sl], want_gl[:, :, r0:r1], f"rank {rank} glam")
        assert all((p != 0).any() for p in part)
        for t, p in zip(total, part):
            t += p.astype(np.float64)
        sfs.close(), c.close()
    # each rank's sums lie within the bound of its own adds; the three bounds add up to at most the whole frame's
    bound = accs[0].bound()
    off = 0
    for l, t in enumerate(total):
        err = np.abs(t.ravel() - accs[0].g[off:off + t.size])
        assert (err <= bound[off:off + t.size]).all(), (l, float((err - bound[off:off + t.size]).max()))
        off += t.size


# ------------------------------------------------------------------------------------------------------ autograd
def test_autograd_in_both_pyramid_modes(ctx, tmp_path, monkeypatch):
    import srz
    from srz import visibility as V
    N, C, n = 8, 5, 2
    L = 4
    rng = np.random.default_rng(91)
    frames = hand_frames(W, H, n, 20)
    fs = ctx.frameset(frames)
    ids = rand_ids(rng, n, H, W, 20)
    v = hand_vis(ids)
    vw = v.view(np.uint32)
    vis = torch.as_tensor(v).cuda()
    dw = np.stack([cuberef.hostile_dirs(rng, (H, W), N) for _ in range(n)])
    finite = np.isfinite(dw).all(1, keepdims=True) & (np.abs(dw).max(1, keepdims=True) > 1e-30)
    dw = np.where(finite, dw, np.float32(1)).astype(np.float32)  # (finite gradients: the loss below squares the output)
    lw = rng.uniform(-0.5, L - 0.5, (n, 1, H, W)).astype(np.float32)
    calls = []
    real = srz.FrameSet.texture_cube_mip_grad
    monkeypatch.setattr(srz.FrameSet, "texture_cube_mip_grad", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    cuben = cuberef.make_cube(16, N, C)
    # ---- mip=None: the pyramid is built inside, its gradient folded into cube.grad
    cube, dt, lt = dev(cuben).requires_grad_(True), dev(dw).requires_grad_(True), dev(lw).requires_grad_(True)
    out = V.texture_cube_mip(fs, vis, cube, dt, lt)
    levels = cubemipref.build(cuben)
    same(words(out.detach()), expect_fwd(tmp_path, frames, vw, dw, lw, levels), "autograd forward")
    out.square().sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == 1  # one call for all three gradients
    g = (2 * out.detach()).contiguous().cpu().numpy()
    accs, want_gd, want_gl = expect_bwd(tmp_path, frames, vw, dw, lw, g, levels)
    same(words(dt.grad), want_gd, "dirs.grad")
    same(words(lt.grad), want_gl, "lam.grad")
    # cube.grad = level 0's adds + the fold of the others: compare against the plain call's parts, folded by the 2D fold's own rule
    gt, gm, gd, gl = V.texture_cube_mip_grad(fs, vis, cube.detach(), dev(dw), dev(lw), dev(g), fold=False)
    parts = [gt.cpu().numpy()] + [x.cpu().numpy() for x in V.cube_mip_views(gm, cuben.shape)]
    check_gpyr(parts, accs, "plain gtex / gmip")
    folded = gt.clone()
    ctx.cube_mip_fold(gm.data_ptr(), gm.numel() * 4, N, C, 1, L, folded.data_ptr(), stream())
    torch.cuda.synchronize()
    ref = accs[0].level(accs[0].g, 0).copy()
    mag, cnt = accs[0].level(accs[0].gabs, 0).copy(), accs[0].level(accs[0].count, 0).astype(np.float64)[..., None] * np.ones(C)
    for l in range(1, L):  # the fold is linear with weights 4^-l: exact scalings of level l's sums, of their magnitudes, and n adds more
        up = lambda a: np.repeat(np.repeat(a, 1 << l, 1), 1 << l, 2)  # noqa: E731
        ref += up(accs[0].level(accs[0].g, l)) * 0.25 ** l
        mag += up(accs[0].level(accs[0].gabs, l)) * 0.25 ** l
        cnt += up(accs[0].level(accs[0].count, l).astype(np.float64)[..., None] * np.ones(C)) + 1
    nu = cnt * 2.0 ** -24
    for got in (cube.grad.cpu().numpy(), folded.cpu().numpy()):
        assert (np.abs(got.astype(np.float64) - ref) <= nu / (1 - nu) * mag).all()
    # ---- a caller's pyramid: cube and mip are separate differentiable inputs, no fold
    own_levels = rand_levels(5, N, C, L)
    cube, mip = dev(own_levels[0]).requires_grad_(True), dev(cubemipref.flat(own_levels, 1)).requires_grad_(True)
    lt = dev(lw).requires_grad_(True)
    out = V.texture_cube_mip(fs, vis, cube, dev(dw), lt, mip=mip)
    same(words(out.detach()), expect_fwd(tmp_path, frames, vw, dw, lw, own_levels), "caller's pyramid forward")
    out.square().sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == 3
    g = (2 * out.detach()).contiguous().cpu().numpy()
    accs, _, want_gl = expect_bwd(tmp_path, frames, vw, dw, lw, g, own_levels)
    same(words(lt.grad), want_gl, "caller's pyramid lam.grad")
    check_gpyr([cube.grad.cpu().numpy()] + [x.cpu().numpy() for x in V.cube_mip_views(mip.grad, own_levels[0].shape)], accs, "cube.grad / mip.grad")
    # nothing needs a gradient: no backward; lam alone: the call asks for glam alone; one level: texture_cube
    k = len(calls)
    assert not V.texture_cube_mip(fs, vis, cube.detach(), dev(dw), dev(lw)).requires_grad and len(calls) == k
    lt = dev(lw).requires_grad_(True)
    V.texture_cube_mip(fs, vis, cube.detach(), dev(dw), lt, n_levels=2).sum().backward()
    assert len(calls) == k + 1 and lt.grad is not None and bool((lt.grad != 0).any())
    one = V.texture_cube_mip(fs, vis, cube.detach(), dev(dw), None, n_levels=1)
    assert torch.equal(one, V.texture_cube(fs, vis, cube.detach(), dev(dw)))
    lamp = V.cube_level(fs, vis, dev(dw), torch.zeros(fs.interpolate_shape(6), device="cuda"), N, L)
    assert tuple(lamp.shape) == (n, 1, H, W) and bool((lamp == 0).all())  # no footprint: level 0
    with pytest.raises(ValueError):
        V.texture_cube_mip(fs, vis, cube.detach(), dev(dw), dev(lw)[:, :, :8])
    with pytest.raises(ValueError):
        V.texture_cube_mip(fs, vis, cube.detach(), dev(dw), dev(lw), mip=mip.detach()[:-1])
    fs.close()
