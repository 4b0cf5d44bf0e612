"""-m gpu: the shadow-map lookup over a visibility buffer and its gradients (srz_frameset_shadow / _shadow_grad, k_shadow,
k_shadow_grad).  The visibility buffer is the GPU's own render_visibility, except where a test writes one by hand; the coordinate
planes are written by hand, except in the geometric tests, where they are the GPU's own interpolate; the expected values are
tests/shadowref.py's on those very buffers (pinned on the CPU by tests/test_shadow_ref.py).  Forward and gsc: a NaN on one side must
be a NaN on the other, every other word matches bit for bit.  gmap: exact where every partial sum is representable (the dyadic
cases) and where a texel has one contributing add, else within gamma_n * sum |term|, gamma_n = n u / (1 - n u), u = 2^-24, n the
texel's contributing adds (+ 1 when the buffer held a value) — one rounding per add, the terms being float32 terms on both sides:
derived, not measured."""
import numpy as np
import pytest
import torch

import shadowref as sr
from srz import abi, parallel
from support import SENTINEL, ccw, ctx, filled, frame, padded_positions, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
BACKDROP = ccw((-8, -8), (400, -8), (-8, 400), z=80.0)
SIZES = [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6), (1, 1, 3)]
MAP_SIZES = sr.MAP_SIZES
WIDTH = 5.0  # soft: an eighth of the spread of e (tests/test_shadow_ref.py)
TG_SLOTS = 2048  # the capacity of k_shadow_grad's table of distinct texels per tile


def n_tris(f):
    return f if isinstance(f, int) else sum(len(t) for t in f.tris)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def map_dims(m):
    return (m.shape[0] if m.ndim == 3 else 1), m.shape[-1], m.shape[-2]


def fwd(fs, vis, sc, m, bias, width, flags=F, fill=0):
    """the forward pass into a buffer prefilled with the word `fill` → uint32 [n, 1, rows, W]"""
    mf, mw, mh = map_dims(m)
    out, t = filled(fs.interpolate_shape(1), fill), dev(m)
    fs.shadow(vis.data_ptr(), sc.data_ptr(), t.data_ptr(), mw, mh, mf, bias, width, out.data_ptr(), fs.interpolate_bytes(1), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def bwd(fs, vis, sc, gout, m, bias, width, want_map=True, want_sc=True, flags=F, fill=0, into=None):
    """the backward pass → (gmap float32 of the map's shape, added into `into` or zeros; gsc uint32 [n, 3, rows, W] from `fill`)"""
    mf, mw, mh = map_dims(m)
    t, g = dev(m), dev(gout)
    assert tuple(g.shape) == tuple(fs.interpolate_shape(1))
    gm = (torch.zeros_like(t) if into is None else dev(into)) if want_map else None
    gs = filled(fs.interpolate_shape(3), fill) if want_sc else None
    fs.shadow_grad(vis.data_ptr(), sc.data_ptr(), g.data_ptr(), t.data_ptr(), mw, mh, mf, bias, width, gm.data_ptr() if want_map else None,
                   gs.data_ptr() if want_sc else None, flags, stream())
    torch.cuda.synchronize()
    return (gm.cpu().numpy() if want_map else None), (words(gs) if want_sc else None)


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def map_of(m, i):
    return m[i] if m.ndim == 3 else m


def expect_fwd(tmp_path, frames, v, scw, m, bias, width, fused=True, fill=0):
    """v: the visibility buffer's words [n, 4, rows, W]; scw: the coordinate planes float32 [n, 3, rows, W]"""
    out = []
    for i, f in enumerate(frames):
        pre = np.full((1,) + v.shape[2:], fill, np.uint32)
        out.append(sr.forward(tmp_path, map_of(m, i), n_tris(f), v[i, 1], scw[i], bias, width, fused, pre))
    return np.stack(out)


def expect_bwd(tmp_path, frames, v, scw, gout, m, bias, width, fused=True, fill=0):
    """(Grad per map frame — one for a shared map —, gsc [n, 3, rows, W] float32)"""
    shared = m.ndim == 2
    accs = [sr.Grad(m.shape[-2:]) for _ in range(1 if shared else len(frames))]
    gs = []
    for i, f in enumerate(frames):
        pre = np.full((3,) + v.shape[2:], fill, np.uint32)
        gs.append(sr.grad(tmp_path, map_of(m, i), n_tris(f), v[i, 1], scw[i], gout[i], bias, width, accs[0 if shared else i], True, fused, pre))
    return accs, np.stack(gs)


def check_gmap(got, accs, what, exact=False, init=None, need_adds=True):
    """init: what the buffer held before the call (one more term of every texel's sum)"""
    got = np.ascontiguousarray(got)
    ref = np.stack([a.gmap for a in accs]).reshape(got.shape)
    mag = np.stack([a.gabs for a in accs]).reshape(got.shape)
    cnt = np.stack([a.count for a in accs]).reshape(got.shape).astype(np.float64)
    assert not need_adds or cnt.sum() > 0, what
    untouched = cnt == 0
    if init is not None:
        ref, mag, cnt = ref + init.astype(np.float64), mag + np.abs(init.astype(np.float64)), cnt + 1
    assert np.isfinite(ref).all()
    nu = cnt * 2.0 ** -24
    bound = nu / (1.0 - nu) * mag
    if exact:
        assert (ref.astype(np.float32).astype(np.float64) == ref).all(), "the case is not dyadic"
        bound = np.zeros_like(bound)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{what}: max err {err.max():.3e}, max err / bound {np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0:.3f}, "
          f"max n {int(cnt.max())}, texels with one add {int((cnt == 1).sum())}, untouched {int(untouched.sum())}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} texels beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    one = cnt == 1
    same((got + np.float32(0))[one], (ref.astype(np.float32) + np.float32(0))[one], what + " (n = 1)")
    if init is None:
        assert (got.view(np.uint32)[untouched] == 0).all()  # never added to: the caller's +0 words
    else:
        assert np.array_equal(got.view(np.uint32)[untouched], np.ascontiguousarray(init).view(np.uint32)[untouched])


def pair(w, h, n, flags=F, k=2):
    t = np.concatenate([soup(1, n, w, h, ZS, big=w < 40), BACKDROP])
    return [frame(t, w, h, flags=flags) for _ in range(k)]


def rand_gout(seed, shape, own=None):
    g = np.random.default_rng([seed, 8]).normal(0, 2, shape).astype(np.float32)
    if own is not None:
        g[np.broadcast_to(~own[:, None], g.shape)] = np.nan  # nobody's words may hold anything
    return g


def owners(v, frames):
    return np.stack([((v[i, 1] & 0x7fffffff) - np.uint32(1)) < n_tris(f) for i, f in enumerate(frames)])


def hand_frames(w, h, n, tris):
    return [frame(soup(1, tris, w, h, ZS), w, h) for _ in range(n)]


def hand_vis(ids):
    """a visibility buffer [n, 4, h, w] float32 with these id words (z, alpha, beta: zeros — the shadow passes read none of them)"""
    v = np.zeros((ids.shape[0], 4) + ids.shape[1:], np.float32)
    v[:, 1] = ids.view(np.float32)
    return v


def rand_ids(rng, n, h, w, tris, holes=True):
    ids = rng.integers(1, tris + 1, (n, h, w)).astype(np.uint32)
    ids |= (rng.random((n, h, w)) < 0.4).astype(np.uint32) << 31
    if holes:
        ids[rng.random((n, h, w)) < 0.1] = 0
    return ids


def both_ways(tmp_path, fs, frames, vis, v, scw, m, bias, width, what, seed=0, flags=F, fill=SENTINEL, into=None, exact=False, need_adds=True,
              gscale=1.0):
    """forward, gsc and gmap of one call each against the reference on the same buffers → (out words, gmap, gsc words)"""
    sc = dev(scw)
    fused = flags == F or all(f.c.flags & F for f in frames if not isinstance(f, int))
    got = fwd(fs, vis, sc, m, bias, width, flags, fill)
    same(got, expect_fwd(tmp_path, frames, v, scw, m, bias, width, fused, fill), what)
    own = owners(v, frames)
    gout = rand_gout(seed, got.shape, own) if not exact else np.random.default_rng(seed).integers(-16, 17, got.shape).astype(np.float32)
    gout *= np.float32(gscale)
    gm, gs = bwd(fs, vis, sc, gout, m, bias, width, flags=flags, fill=fill, into=into)
    accs, want_gs = expect_bwd(tmp_path, frames, v, scw, gout, m, bias, width, fused, fill)
    same(gs, want_gs, what + " gsc")
    check_gmap(gm, accs, what + " gmap", exact=exact, init=into, need_adds=need_adds and width > 0)
    if width == 0:
        assert all(a.count.sum() == 0 for a in accs)
    return got, gm, gs


# ------------------------------------------------------------------------------------------------------ forward, gsc and gmap
@pytest.mark.parametrize("w,h,n", SIZES)
def test_sizes_maps_hard_and_soft(ctx, tmp_path, w, h, n):
    """the GPU's own visibility buffers of every frame size under hand-written coordinates (shadowref.hostile_coords: the generator's
    spread, exact texel hits, both borders from both sides, NaN / inf / 1e30) over every map size, shared and per frame, with
    non-finite texels; hard and soft; every bias.  The maps' extents are their own: none of the kernels' indexing may lean on the
    frame's (one pair coincides, 64 x 64 under the 64 x 64 frame; every other one differs in both axes)"""
    frames = pair(w, h, n)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    own = owners(v, frames)
    assert own.any(1).any(1).all()
    rng = np.random.default_rng([w, h, 5])
    for k, (mw, mh) in enumerate(MAP_SIZES):
        scw = np.stack([sr.hostile_coords(rng, (h, w), mw, mh) for _ in frames])
        scw[np.broadcast_to(~own[:, None], scw.shape)] = np.nan  # never read
        m = sr.hostile_map(rng, mw, mh, frames=2)
        m = m if (k + w) % 2 else m[0]
        for width in (0.0, WIDTH):
            bias = sr.BIASES[(k + (width > 0)) % 3]
            what = f"{w}x{h} map {mw}x{mh} {m.ndim} width {width} bias {bias}"
            got, gm, gs = both_ways(tmp_path, fs, frames, vis, v, scw, m, bias, width, what, seed=k, need_adds=w >= 50 and mw > 1)
            assert (got[~own[:, None]] == 0).all() and (gs[np.broadcast_to(~own[:, None], gs.shape)] == 0).all()
            assert not np.isnan(got.view(np.float32)).any()  # a NaN texel or coordinate never reaches out
    fs.close()


@pytest.mark.parametrize("width", (0.0, 4.0, sr.TINY_WIDTH))
def test_kat_values_in_every_lane_of_a_quad(ctx, tmp_path, width):
    """the coordinate values of the CPU KATs in every lane position of a thread's quad, over maps holding the KATs' texels, under a
    hand-written visibility buffer with holes (quads that are partly owned) and one frame nobody owns"""
    w, h, n, tris = 64, 64, 3, 20
    rng = np.random.default_rng(17)
    frames = hand_frames(w, h, n, tris)
    fs = ctx.frameset(frames)
    ids = rand_ids(rng, n, h, w, tris)
    ids[2] = 0  # an all-nobody frame
    v = hand_vis(ids)
    vw = v.view(np.uint32)
    vis = torch.as_tensor(v).cuda()
    own = owners(vw, frames)
    part = own[:2].reshape(2, h, w // 4, 4).sum(-1)
    assert ((part > 0) & (part < 4)).sum() > 200 and not own[2].any()
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    for mw, mh in ((2, 2), (5, 3)):
        kx, ky = sr.kat_coords(mw), sr.kat_coords(mh)
        ix, iy = (xs + ys) % len(kx), (xs + 3 * ys) % len(ky)
        sd = np.float32([np.nan, 60.0, np.inf, 50.0, 70.0, -np.inf, 60.0])[(xs + 5 * ys) % 7]
        scw = np.broadcast_to(np.stack([kx[ix], ky[iy], sd]), (n, 3, h, w)).copy()
        for value in range(len(kx)):  # every value meets every lane, on owned pixels, in sx and in sy
            for lane in range(4):
                assert (own[0] & (ix == value) & (xs % 4 == lane)).any() and (own[0] & (iy == value) & (xs % 4 == lane)).any()
        m = np.float32([60.0, np.inf, -np.inf, np.nan, 50.0, 70.0, 60.0, 60.5])[rng.integers(0, 8, (n, mh, mw))]
        for mm in (m, m[0]):
            got, gm, gs = both_ways(tmp_path, fs, frames, vis, vw, scw, mm, 0.0, width, f"KATs map {mw}x{mh} {mm.ndim} width {width}", seed=3,
                                    gscale=2.0 ** -100 if width == sr.TINY_WIDTH else 1.0)  # (a term is w g / width: kept finite)
            assert (got[2] == 0).all() and (gs[2] == 0).all()
            unsampled = own & ~np.isfinite(scw).all(1)
            assert unsampled.sum() > 500 and (got[:, 0][unsampled] == np.float32(1).view(np.uint32)).all()
            assert (gs[np.broadcast_to(unsampled[:, None], gs.shape)] == 0).all()
    fs.close()


def test_not_fused_and_ids_out_of_range(ctx, tmp_path):
    """frames that do not clear; ids out of range and bare class bits written into the buffer: with the fused clear nobody's words
    become 0, without it the prefilled sentinel survives on exactly nobody's pixels"""
    t = soup(3, 40, 96, 80, ZS)
    frames = [frame(t, 96, 80, flags=0), frame(t, 96, 80, flags=0)]
    fs = ctx.frameset(frames)
    vn = visibility(fs).cpu().numpy()
    ids = vn[0, 1].view(np.uint32)
    ids[0, :16], ids[1, :16], ids[2, :16], ids[3, :16], ids[4, :16] = len(t) + 1, 0x7fffffff, 0xffffffff, (len(t) + 1) | 0x80000000, 0x80000000
    vis = torch.as_tensor(vn).cuda()
    vw = vn.view(np.uint32)
    own = owners(vw, frames)
    nobody = ~own[0]
    assert nobody[:5, :16].all() and nobody.sum() > 500 and own[0].sum() > 200
    rng = np.random.default_rng(21)
    scw = np.stack([sr.hostile_coords(rng, (80, 96), 5, 3) for _ in range(2)])
    scw[np.broadcast_to(~own[:, None], scw.shape)] = np.nan  # never read
    m = sr.make_map(6, 5, 3)
    for width in (0.0, WIDTH):
        fused, _, gs_f = both_ways(tmp_path, fs, frames, vis, vw, scw, m, 0.375, width, f"fused width {width}", flags=F)
        kept, _, gs_k = both_ways(tmp_path, fs, frames, vis, vw, scw, m, 0.375, width, f"not fused width {width}", flags=0)
        assert (fused[0][:, nobody] == 0).all() and (kept[0][:, nobody] == SENTINEL).all()  # exactly the owned words change
        assert (kept[0][:, own[0]] != SENTINEL).all() and np.array_equal(kept[:, 0][own], fused[:, 0][own])
        assert (gs_f[0][:, nobody] == 0).all() and (gs_k[0][:, nobody] == SENTINEL).all() and (gs_k[0][:, own[0]] != SENTINEL).all()
    fs.close()


def test_nine_frames_wrap_the_frame_deal(ctx, tmp_path):
    """eight frames and more take the walk's other branch (workgroup b serves the frames f = b mod 8): with nine frames of four tiles
    the workgroups of frame 0 go on to a tile of frame 8 — k_shadow_grad's table is handed from one tile to the next, its keys
    released in between"""
    t = np.concatenate([soup(11, 60, 64, 64, ZS), BACKDROP])
    frames = []
    for i in range(9):
        t2 = t.copy()
        t2["pos"][:-1, :, :2] += np.float32([1.5 * i, -1.0 * i])
        frames.append(frame(t2, 64, 64))
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    scw = np.stack([sr.make_coords(i, (64, 64), 64, 64) for i in range(9)])
    for m in (sr.make_map(4, 64, 64, frames=9), sr.make_map(4, 64, 64)):
        got, _, _ = both_ways(tmp_path, fs, frames, vis, v, scw, m, 0.0, WIDTH, f"nine frames {m.ndim}", seed=3)
    assert len({got[i].tobytes() for i in range(9)}) == 9
    fs.close()


# ------------------------------------------------------------------------------------------------------ gmap, by construction
@pytest.mark.parametrize("w,h,n", [(96, 96, 2), (50, 37, 2), (64, 64, 9)])
def test_gmap_exact_on_dyadic_inputs(ctx, tmp_path, w, h, n):
    """fractions that are multiples of 1 / 16 (0 among them), integer map depths against sd on the half integers within 1.5 of them,
    width 4, integer gout in [-16, 16], an integer buffer to add into: every corner is on the ramp, every term is a multiple of
    2^-10 and every partial sum is representable, so any order of adds gives the same bits"""
    rng = np.random.default_rng([w, 3])
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    ids = rand_ids(rng, n, h, w, 20)
    v = hand_vis(ids)
    vis = torch.as_tensor(v).cuda()
    mw, mh = 5, 3
    scw = np.stack([rng.integers(-1, mw, (n, h, w)) + rng.integers(0, 16, (n, h, w)) / 16.0,
                    rng.integers(-1, mh, (n, h, w)) + rng.integers(0, 16, (n, h, w)) / 16.0,
                    60.0 + rng.integers(-1, 2, (n, h, w)) + 0.5], 1).astype(np.float32)
    shared = n != 2
    m = (60.0 + rng.integers(0, 2, (mh, mw) if shared else (n, mh, mw))).astype(np.float32)
    init = rng.integers(-64, 65, m.shape).astype(np.float32)
    got, gm, gs = both_ways(tmp_path, fs, frames, vis, v.view(np.uint32), scw, m, 0.0, 4.0, f"dyadic {w}x{h}", seed=w, into=init, exact=True)
    assert (gm != init).any()
    fs.close()


def test_table_overflow_and_the_tile_without_a_moving_corner(ctx, tmp_path):
    """one 32 x 32 tile whose coordinates step 3 texels per pixel over the 160 x 160 map, every corner on the ramp: 4 096 distinct
    moving texels against the table's 2 048 slots — the corners without a slot add straight to memory, in frame 0 each texel has one
    add (exact), and the bound holds.  Then the same call with width 0 and d_gmap given: no corner moves, every tile skips the table, and the
    buffer comes back bit for bit"""
    w = h = 32
    n, mw, mh = 2, 160, 160
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    rng = np.random.default_rng(31)
    ids = rand_ids(rng, n, h, w, 20, holes=False)
    v = hand_vis(ids)
    vw = v.view(np.uint32)
    vis = torch.as_tensor(v).cuda()
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    scw = np.stack([np.stack([3 * xs + 0.37 + 40 * i, 3 * ys + 0.61 + 20 * i, np.full((h, w), 60.0, np.float32)]) for i in range(n)])
    scw[1, 0] += rng.uniform(0, 2.5, (h, w)).astype(np.float32)  # frame 1: neighbours now and then share a texel
    for m in (60.0 + rng.uniform(-1, 1, (mh, mw)).astype(np.float32), 60.0 + rng.uniform(-1, 1, (n, mh, mw)).astype(np.float32)):
        gout = rand_gout(11, (n, 1, h, w))
        accs, _ = expect_bwd(tmp_path, frames, vw, scw, gout, m, 0.0, 8.0)
        distinct = [int((a.count > 0).sum()) for a in accs]
        assert all(int(a.count.sum()) == 4 * w * h * (n if m.ndim == 2 else 1) for a in accs)  # every corner moves
        assert (distinct[0] > 2 * TG_SLOTS) if m.ndim == 2 else (distinct[0] == 4 * w * h and distinct[1] > TG_SLOTS)
        got, gm, gs = both_ways(tmp_path, fs, frames, vis, vw, scw, m, 0.0, 8.0, f"overflow {m.ndim}", seed=11)
        assert (gm != 0).sum() >= distinct[0]
        only_gm = bwd(fs, vis, dev(scw), gout, m, 0.0, 8.0, want_sc=False)[0]
        check_gmap(only_gm, accs, f"overflow {m.ndim} gmap alone")
        # the hard test adds nothing: the buffer is bit-unchanged, whatever it held
        init = rng.normal(0, 5, m.shape).astype(np.float32)
        init.reshape(-1)[:4] = np.float32([np.nan, np.inf, -0.0, 1e-42])
        hard = bwd(fs, vis, dev(scw), gout, m, 0.0, 0.0, into=init)[0]
        assert np.array_equal(hard.view(np.uint32), init.view(np.uint32))
        hard_alone = bwd(fs, vis, dev(scw), gout, m, 0.0, 0.0, want_sc=False, into=init)[0]
        assert np.array_equal(hard_alone.view(np.uint32), init.view(np.uint32))
    fs.close()


@pytest.mark.parametrize("w,h,n", SIZES[:3])
def test_gmap_on_rendered_buffers_and_accumulation(ctx, tmp_path, w, h, n):
    """a magnified map (many pixels per texel: long sums) and a minified one (most texels one add), each want flag alone, and
    accumulation into a buffer that is not zero"""
    frames = pair(w, h, n)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    own = owners(v, frames)
    for mw, mh in ((2, 2), (160, 160)):
        scw = np.stack([sr.make_coords(i + w, (h, w), mw, mh) for i in range(2)])
        sc = dev(scw)
        for m in (sr.make_map(mw, mw, mh, frames=2), sr.make_map(mw, mw, mh)):
            gout = rand_gout(mw, (2, 1, h, w), own)
            gm, gs = bwd(fs, vis, sc, gout, m, -1.25, WIDTH)
            accs, want_gs = expect_bwd(tmp_path, frames, v, scw, gout, m, -1.25, WIDTH)
            same(gs, want_gs, f"gsc map {mw}")
            check_gmap(gm, accs, f"{w}x{h} map {mw} {m.ndim}")
            only_gm = bwd(fs, vis, sc, gout, m, -1.25, WIDTH, want_sc=False)[0]
            check_gmap(only_gm, accs, f"{w}x{h} map {mw} {m.ndim} gmap alone")
            only_gs = bwd(fs, vis, sc, gout, m, -1.25, WIDTH, want_map=False)[1]
            assert np.array_equal(only_gs, gs)
    init = np.random.default_rng(4).normal(0, 5, m.shape).astype(np.float32)
    gm2, _ = bwd(fs, vis, sc, gout, m, -1.25, WIDTH, want_sc=False, into=init)
    check_gmap(gm2, accs, "into a non-zero buffer", init=init)
    assert (gm2 != init).any()
    fs.close()


# ------------------------------------------------------------------------------------------------------ sharded
def test_sharded_world_2(ctx, tmp_path):
    """rank 0 of 2 and rank 1 of 2 on one GPU: the planes match the unsharded call's band by band, bit for bit; the two ranks' gmap
    sum to the unsharded reference within the bound (+ 1 add: the sum of the two partial results); the map is whole on both"""
    import srz
    w, h, tris = 64, 128, 50
    t = np.concatenate([soup(5, tris - 1, w, h, ZS, big=True), BACKDROP])
    frames = [frame(t, w, h), frame(t, w, h)]
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    scw = np.stack([sr.make_coords(i, (h, w), 5, 3) for i in range(2)])
    m = sr.make_map(12, 5, 3)
    gout = rand_gout(13, (2, 1, h, w))
    full = fwd(fs, vis, dev(scw), m, 0.375, WIDTH)
    same(full, expect_fwd(tmp_path, frames, v, scw, m, 0.375, WIDTH), "whole frame")
    whole_gs = bwd(fs, vis, dev(scw), gout, m, 0.375, WIDTH, want_map=False)[1]
    accs, _ = expect_bwd(tmp_path, frames, v, scw, gout, m, 0.375, WIDTH)
    fs.close()
    total = np.zeros(m.shape, np.float64)
    for rank in (0, 1):
        c = srz.Context(0, rank, 2)
        sfs = c.frameset(frames)
        svis = visibility(sfs)
        rows = parallel.band_rows(h, rank, 2)
        assert len(rows) == 2
        ssc = np.zeros(sfs.interpolate_shape(3), np.float32)
        sg = np.zeros(sfs.interpolate_shape(1), np.float32)
        for (lb, _, r0, r1) in rows:
            ssc[:, :, lb * 32: lb * 32 + r1 - r0] = scw[:, :, r0:r1]
            sg[:, :, lb * 32: lb * 32 + r1 - r0] = gout[:, :, r0:r1]
        shard = fwd(sfs, svis, dev(ssc), m, 0.375, WIDTH)
        part, part_gs = bwd(sfs, svis, dev(ssc), sg, m, 0.375, WIDTH)
        for (lb, _, r0, r1) in rows:
            same(shard[:, :, lb * 32: lb * 32 + r1 - r0], full[:, :, r0:r1], f"rank {rank} band {lb}")
            same(part_gs[:, :, lb * 32: lb * 32 + r1 - r0], whole_gs[:, :, r0:r1], f"gsc rank {rank} band {lb}")
        assert (part != 0).any()
        total += part.astype(np.float64)
        sfs.close(), c.close()
    # each rank's sums lie within the bound of its own adds; the two bounds add up to at most the whole frame's
    err = np.abs(total - accs[0].gmap)
    assert (err <= accs[0].bound()).all(), float((err - accs[0].bound()).max())


# ------------------------------------------------------------------------------------------------------ geometry, end to end
SHEAR = 0.25            # the light's view: x' = x + SHEAR * z
# the occluder quad x0, y0, x1, y1 at z = 40, over a floor at z = 80.  Neither quad's diagonal passes through a pixel's sample point
# (the integers): a sample exactly on the edge two triangles share belongs to neither, and the floor would show through the crack
OCC = (20.5, 24.5, 36.5, 40.25)
FLOOR = (-40.5, -40.5, 72.5, 72.25)


def quad(x0, y0, x1, y1, z):
    return np.concatenate([ccw((x0, y0), (x1, y0), (x0, y1), z=z), ccw((x1, y1), (x0, y1), (x1, y0), z=z)])


def scene(w=64, h=64, n=2):
    """(camera frames, light frames, the light set's positions [n, T, 3, 3]): floor (triangles 0, 1, both in both views), occluder
    (2, 3) and a far triangle outside both views (4); the light frames are the same triangles sheared"""
    t = np.concatenate([quad(*FLOOR, 80.0), quad(*OCC, 40.0), ccw((300, 300), (310, 300), (300, 310), z=60.0)])
    tl = t.copy()
    tl["pos"][:, :, 0] += np.float32(SHEAR) * tl["pos"][:, :, 2]
    cam, light = [frame(t, w, h) for _ in range(n)], [frame(tl, w, h) for _ in range(n)]
    return cam, light, padded_positions(light, len(t)).reshape(n, len(t), 3, 3)


def test_a_quad_casts_its_sheared_shadow_on_the_floor(ctx, tmp_path):
    """the coordinates are the GPU's interpolate, over the camera set, of the light set's positions; the map is plane 0 of the light
    set's visibility buffer.  Bit for bit the reference on those buffers; and, independently, the shadow lies where the shear puts
    it: the occluder's footprint moved by SHEAR * (40 - 80) = -10 pixels on the floor"""
    w = h = 64
    cam, light, pos_l = scene(w, h)
    fs_c, fs_l = ctx.frameset(cam), ctx.frameset(light)
    vis_c, vis_l = visibility(fs_c), visibility(fs_l)
    v = words(vis_c)
    a = dev(pos_l)
    sc = torch.zeros(fs_c.interpolate_shape(3), dtype=torch.float32, device="cuda")
    fs_c.interpolate(vis_c.data_ptr(), a.data_ptr(), 3, 2, pos_l.shape[1], sc.data_ptr(), fs_c.interpolate_bytes(3), F, stream())
    torch.cuda.synchronize()
    scw = sc.cpu().numpy()
    m = vis_l[:, 0].cpu().numpy()
    assert ((np.abs(m - 40.0) < 1e-3) | (np.abs(m - 80.0) < 1e-3)).all() and (m < 50).sum() > 2 * 200  # the floor, and the occluder on it
    tri = (v[:, 1] & 0x7fffffff).astype(np.int64) - 1
    floor, occ = (tri == 0) | (tri == 1), (tri == 2) | (tri == 3)
    assert floor.sum() > 2 * 3500 and occ.sum() > 2 * 200 and (floor | occ).all()
    assert all((tri == k).sum() > 2 * 100 for k in range(4))
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    x0, y0, x1, y1 = OCC
    dx = SHEAR * (40.0 - 80.0)
    # signed distance to the footprint's rectangle, positive inside
    inside = np.minimum(np.minimum(xs - (x0 + dx), (x1 + dx) - xs), np.minimum(ys - y0, y1 - ys))
    for bias, width in ((0.5, 0.0), (0.5, 0.25), (3.0, 4.0)):  # (soft: bias > width / 2, so that the lit side is off the ramp)
        got = fwd(fs_c, vis_c, sc, m, bias, width)
        same(got, expect_fwd(tmp_path, cam, v, scw, m, bias, width), f"shadow bias {bias} width {width}")
        lit = got.view(np.float32)[:, 0]
        for i in range(2):
            assert (lit[i][floor[i] & (inside > 1.5)] == 0).all() and (floor[i] & (inside > 1.5)).sum() > 80
            assert (lit[i][floor[i] & (inside < -1.5)] == 1).all()
            assert (lit[i][occ[i]] == 1).all()
    fs_c.close(), fs_l.close()


def test_autograd(ctx, tmp_path, monkeypatch):
    import srz
    from srz.visibility import shadow, shadow_grad
    frames = pair(100, 70, 120)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    scw = np.stack([sr.make_coords(i, (70, 100), 5, 3) for i in range(2)])
    sc = dev(scw)
    calls = []
    real = srz.FrameSet.shadow_grad
    monkeypatch.setattr(srz.FrameSet, "shadow_grad", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    for shape in ((3, 5), (2, 3, 5), (2, 1, 3, 5)):
        mn = sr.make_map(16, 5, 3, frames=2).reshape((2,) + shape[1:]) if len(shape) > 2 else sr.make_map(16, 5, 3)
        m = dev(mn).requires_grad_(True)
        st = sc.clone().requires_grad_(True)
        out = shadow(fs, vis, m, st, 0.375, WIDTH)
        assert out.shape == (2, 1, 70, 100) and out.requires_grad
        m3 = mn.reshape(2, 3, 5) if len(shape) > 2 else mn
        same(words(out.detach()), fwd(fs, vis, sc, m3, 0.375, WIDTH), "forward")
        n = len(calls)
        out.square().sum().backward()
        torch.cuda.synchronize()
        assert len(calls) == n + 1  # one call for both gradients
        g = (2 * out.detach()).contiguous()  # float32: what the backward was handed
        gm, gs = shadow_grad(fs, vis, m.detach(), sc, g, 0.375, WIDTH)
        assert gm.shape == m.shape == m.grad.shape
        same(words(st.grad), words(gs), "sc.grad")
        accs, want_gs = expect_bwd(tmp_path, frames, v, scw, g.cpu().numpy(), m3, 0.375, WIDTH)
        same(words(gs), want_gs, "plain gsc")
        check_gmap(m.grad.cpu().numpy().reshape(m3.shape), accs, "map.grad")
        check_gmap(gm.cpu().numpy().reshape(m3.shape), accs, "plain gmap")
        assert shadow_grad(fs, vis, m.detach(), sc, g, 0.375, WIDTH, want_gsc=False)[1] is None
        assert shadow_grad(fs, vis, m.detach(), sc, g, 0.375, WIDTH, want_gmap=False)[0] is None
    # nothing needs a gradient: no backward is there to launch; one input does: the call asks for that output alone
    n = len(calls)
    out = shadow(fs, vis, m.detach(), sc, 0.375, WIDTH)
    assert not out.requires_grad and out.grad_fn is None and len(calls) == n
    st = sc.clone().requires_grad_(True)
    m.grad = None
    shadow(fs, vis, m.detach(), st, 0.375, WIDTH).sum().backward()
    assert len(calls) == n + 1 and st.grad is not None and m.grad is None
    m2 = m.detach().clone().requires_grad_(True)
    shadow(fs, vis, m2, sc).sum().backward()  # the hard test: the map's gradient exists and is zero
    assert len(calls) == n + 2 and m2.grad is not None and not bool(m2.grad.any())
    # a non-contiguous map (a plane of a visibility buffer) is made contiguous
    buf = torch.zeros((2, 4, 3, 5), device="cuda")
    buf[:, 0] = dev(m3)
    assert not buf[:, 0].is_contiguous()
    same(words(shadow(fs, vis, buf[:, 0], sc, 0.375, WIDTH)), fwd(fs, vis, sc, m3, 0.375, WIDTH), "non-contiguous map")
    with pytest.raises(ValueError):
        shadow(fs, vis, dev(np.zeros((3, 3, 5))), sc)
    with pytest.raises(ValueError):
        shadow(fs, vis, m.detach(), sc[:, :2])
    with pytest.raises(ValueError):
        shadow(fs, vis, m.detach(), sc, 0.0, -1.0)
    fs.close()


def test_the_whole_chain_reaches_the_light_positions(ctx, tmp_path):
    """shadow(fs_cam, vis_cam, depth(fs_l, vis_l, pos_l), interpolate(fs_cam, vis_cam, pos_l)): a finite, non-zero gradient arrives on
    pos_l — the receivers' share through interpolate, the occluders' through depth — on the floor's and the occluder's triangles
    only; it is the chain composed from the plain calls"""
    from srz import visibility as V
    cam, light, pos_n = scene()
    fs_c, fs_l = ctx.frameset(cam), ctx.frameset(light)
    vis_c, vis_l = visibility(fs_c), visibility(fs_l)
    pos_l = dev(pos_n).requires_grad_(True)
    zmap = V.depth(fs_l, vis_l, pos_l)
    sc = V.interpolate(fs_c, vis_c, pos_l.view(2, -1, 3, 3))
    zmap.retain_grad(), sc.retain_grad()
    lit = V.shadow(fs_c, vis_c, zmap, sc, 0.5, 4.0)
    assert lit.shape == (2, 1, 64, 64)
    same(words(lit.detach()), fwd(fs_c, vis_c, sc.detach(), zmap.detach().cpu().numpy()[:, 0], 0.5, 4.0), "chain forward")
    weight = dev(np.random.default_rng(20).normal(0, 1, tuple(lit.shape)))
    (lit * weight).sum().backward()
    torch.cuda.synchronize()
    g = pos_l.grad
    assert bool(torch.isfinite(g).all()) and bool((g[:, :4] != 0).any(-1).any(-1).all()) and not bool(g[:, 4].any())
    gm, gs = V.shadow_grad(fs_c, vis_c, zmap.detach(), sc.detach(), weight.contiguous(), 0.5, 4.0)
    same(words(sc.grad), words(gs), "sc.grad against the plain call")
    v = words(vis_c)
    accs, want_gs = expect_bwd(tmp_path, cam, v, sc.detach().cpu().numpy(), weight.cpu().numpy(), zmap.detach().cpu().numpy()[:, 0], 0.5, 4.0)
    same(words(gs), want_gs, "plain gsc")
    check_gmap(zmap.grad.cpu().numpy()[:, 0], accs, "chain map.grad")
    assert bool((zmap.grad != 0).any()) and bool((sc.grad[:, 2] != 0).any())
    fs_c.close(), fs_l.close()
