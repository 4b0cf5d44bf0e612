"""-m gpu: perspective-correct barycentrics over a visibility buffer, their gradients and the attribute derivatives under them
(srz_frameset_perspective / _perspective_grad / _interpolate_deriv_persp; k_persp, k_persp_grad, k_interp_deriv_persp).  The
visibility buffer is the GPU's own render_visibility, except where a test writes one by hand; the expected values are
tests/perspref.py's on those very buffers (pinned on the CPU by tests/test_persp_ref.py).  The perspective buffer, gbary and the
derivative planes: a NaN on one side must be a NaN on the other, every other word matches bit for bit.  gq: exact where every partial
sum is representable (the dyadic case) and where an element has one contributing pixel, else within gamma_n * sum |term|,
gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing pixels (+ 1 when the buffer held a value) — one rounding per add,
the terms being float32 products on both sides: derived, not measured."""
import numpy as np
import pytest
import torch

import gbufref
import interpref
import perspref
from srz import abi, parallel
from support import SENTINEL, ccw, ctx, filled, frame, padded_positions, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
BACKDROP = ccw((-8, -8), (400, -8), (-8, 400), z=80.0, uv=((0.1, 0.2), (0.9, 0.3), (0.4, 0.95)))
SIZES = [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6), (1, 1, 3)]
PG_SLOTS = 128  # the capacity of k_persp_grad's table of distinct owners per tile (IG_SLOTS)


def n_tris(f):
    return f if isinstance(f, int) else sum(len(t) for t in f.tris)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def q_dims(q):
    return (q.shape[0] if q.ndim == 3 else 1), q.shape[-2]


def q_of(q, i):
    return q[i] if q.ndim == 3 else q


def fwd(fs, vis, q, flags=F, fill=SENTINEL, s=None):
    """the perspective buffer into a buffer prefilled with the word `fill` → uint32 [n, 4, rows, W], and the device tensor"""
    qf, T = q_dims(q)
    out, t = filled(fs.out_shape, fill), dev(q)
    fs.perspective(vis.data_ptr(), t.data_ptr(), qf, T, out.data_ptr(), fs.out_bytes, flags, stream() if s is None else s)
    torch.cuda.synchronize()
    return words(out), out.view(torch.float32)


def bwd(fs, vis, q, gbp, want_bary=True, want_q=True, flags=F, fill=SENTINEL, into=None):
    """(gq float32 of q's shape, added into `into` or zeros; gbary uint32 [n, 2, rows, W] from `fill`)"""
    qf, T = q_dims(q)
    t, g = dev(q), dev(gbp)
    assert tuple(g.shape) == tuple(fs.interpolate_shape(2))
    gq = (torch.zeros_like(t) if into is None else dev(into)) if want_q else None
    gb = filled(fs.interpolate_shape(2), fill) if want_bary else None
    fs.perspective_grad(vis.data_ptr(), t.data_ptr(), qf, T, g.data_ptr(), gb.data_ptr() if want_bary else None,
                        gq.data_ptr() if want_q else None, flags, stream())
    torch.cuda.synchronize()
    return (gq.cpu().numpy() if want_q else None), (words(gb) if want_bary else None)


def drv(fs, vis, q, attr, flags=F, fill=SENTINEL):
    qf, T = q_dims(q)
    af, At, C = (attr.shape[0] if attr.ndim == 4 else 1), attr.shape[-3], attr.shape[-1]
    out, t, a = filled(fs.interpolate_shape(2 * C), fill), dev(q), dev(attr)
    fs.interpolate_deriv_persp(vis.data_ptr(), t.data_ptr(), qf, T, a.data_ptr(), C, af, At, out.data_ptr(), fs.interpolate_bytes(2 * C), flags,
                               stream())
    torch.cuda.synchronize()
    return words(out)


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def expect_fwd(tmp_path, frames, v, q):
    return np.stack([perspref.forward(tmp_path, q_of(q, i), n_tris(f), v[i]) for i, f in enumerate(frames)])


def expect_bwd(tmp_path, frames, v, q, gbp, fused=True, fill=SENTINEL):
    """(Grad per q frame — one for a shared q —, gbary [n, 2, rows, W] float32)"""
    shared = q.ndim == 2
    accs = [perspref.Grad(q.shape[-2:]) for _ in range(1 if shared else len(frames))]
    gb = []
    for i, f in enumerate(frames):
        pre = np.full((2,) + v.shape[2:], fill, np.uint32)
        gb.append(perspref.grad(tmp_path, q_of(q, i), n_tris(f), v[i], gbp[i], accs[0 if shared else i], True, fused, pre))
    return accs, np.stack(gb)


def expect_drv(tmp_path, frames, v, q, attr, pos, fused=True, fill=SENTINEL):
    out = []
    for i, f in enumerate(frames):
        pre = np.full((2 * attr.shape[-1],) + v.shape[2:], fill, np.uint32)
        out.append(perspref.deriv(tmp_path, q_of(q, i), pos[i], attr[i] if attr.ndim == 4 else attr, n_tris(f), v[i], fused, pre))
    return np.stack(out)


def check_gq(got, accs, what, exact=False, init=None):
    """init: what the buffer held before the call (one more term of every element's sum)"""
    ref = np.stack([a.gq for a in accs]).reshape(got.shape)
    mag = np.stack([a.gabs for a in accs]).reshape(got.shape)
    cnt = np.stack([np.broadcast_to(a.count[:, None], a.gq.shape) for a in accs]).reshape(got.shape).astype(np.float64)
    touched = cnt > 0
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
          f"max n {int(cnt.max())}, elements with one pixel {int((cnt == 1).sum())}, untouched {int((~touched).sum())}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    if init is None:
        one = cnt == 1
        same((got + np.float32(0))[one], (ref.astype(np.float32) + np.float32(0))[one], what + " (n = 1)")
        assert (got[~touched] == 0).all()
    else:
        assert np.array_equal(got[~touched], init[~touched])


def pair(w, h, n, flags=F, k=2, backdrop=True):
    t = soup(1, n, w, h, ZS, big=w < 40)
    if backdrop:
        t = np.concatenate([t, BACKDROP])
    return [frame(t, w, h, flags=flags) for _ in range(k)]


def rand_planes(seed, shape, own=None, scale=2.0):
    g = np.random.default_rng([seed, 8]).normal(0, scale, shape).astype(np.float32)
    if own is not None:
        g[np.broadcast_to(~own[:, None], g.shape)] = np.nan  # nobody's words may hold anything
    return g


def owners(v, frames):
    return np.stack([((v[i, 1] & 0x7fffffff) - np.uint32(1)) < n_tris(f) for i, f in enumerate(frames)])


def hand_vis(rng, n, h, w, tris, holes=True, dyadic=False):
    """a visibility buffer [n, 4, h, w] float32 by hand: random owners of either class, holes, alpha and beta inside the triangle
    (dyadic: multiples of 1 / 8 with alpha + beta <= 1)"""
    ids = rng.integers(1, tris + 1, (n, h, w)).astype(np.uint32)
    ids |= (rng.random((n, h, w)) < 0.4).astype(np.uint32) << 31
    if holes:
        ids[rng.random((n, h, w)) < 0.1] = 0
    v = np.zeros((n, 4, h, w), np.float32)
    v[:, 0] = rng.uniform(1, 9, (n, h, w))
    v[:, 1] = ids.view(np.float32)
    if dyadic:
        a = rng.integers(0, 9, (n, h, w))
        b = (rng.random((n, h, w)) * (9 - a)).astype(np.int64)
        v[:, 2], v[:, 3] = a / 8.0, b / 8.0
    else:
        wgt = rng.dirichlet([1.0, 1.0, 1.0], (n, h, w))
        v[:, 2], v[:, 3] = wgt[..., 0], wgt[..., 1]
    return v


def hand_frames(w, h, n, tris):
    return [frame(soup(1, tris, w, h, ZS), w, h) for _ in range(n)]


# ------------------------------------------------------------------------------------------------------ the three passes, bit for bit
@pytest.mark.parametrize("w,h,n", SIZES)
def test_sizes_and_both_q_forms(ctx, tmp_path, w, h, n):
    frames = pair(w, h, n)
    T = n_tris(frames[0])
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    own = owners(v, frames)
    assert own.any(1).any(1).all()
    pos = padded_positions(frames, T + 3)
    attr = np.random.default_rng(w).normal(0, 2, (2, T + 3, 3, 5)).astype(np.float32)
    gbp = rand_planes(w, (2, 2, h, w), own)
    for q in (perspref.make_q(w, T + 3), perspref.make_q(w + 1, T + 3, frames=2)):  # shared and per frame, q_tris above the count
        what = f"{w}x{h} q {q.ndim}"
        want = expect_fwd(tmp_path, frames, v, q)
        for flags in (F, 0):  # every word is written whatever the flags say
            got, pv = fwd(fs, vis, q, flags)
            same(got, want, what)
        assert np.array_equal(got[:, :2], v[:, :2]) and (got[:, 2:] != v[:, 2:]).any()  # z and ids copied, some alpha, beta rewritten
        gq, gb = bwd(fs, vis, q, gbp)
        accs, want_gb = expect_bwd(tmp_path, frames, v, q, gbp)
        same(gb, want_gb, what + " gbary")
        check_gq(gq, accs, what + " gq")
        assert np.array_equal(bwd(fs, vis, q, gbp, want_q=False)[1], gb)  # d_gq null
        check_gq(bwd(fs, vis, q, gbp, want_bary=False)[0], accs, what + " gq alone")  # d_gbary null
        for a in (attr, attr[0], attr[..., :1], attr[0][..., :2]):
            same(drv(fs, vis, q, a), expect_drv(tmp_path, frames, v, q, a, pos), what + f" deriv C {a.shape[-1]} {a.ndim}")
        # composition: interpolate and gbuffer(UV) over the perspective buffer are the references over the reference's buffer
        out, a_dev = filled(fs.interpolate_shape(5), SENTINEL), dev(attr)
        fs.interpolate(pv.data_ptr(), a_dev.data_ptr(), 5, 2, T + 3, out.data_ptr(), fs.interpolate_bytes(5), F, stream())
        gb_out = filled(fs.gbuffer_shape(abi.GB_UV), SENTINEL)
        fs.gbuffer(pv.data_ptr(), gb_out.data_ptr(), fs.gbuffer_bytes(abi.GB_UV), abi.GB_UV, F, stream())
        torch.cuda.synchronize()
        same(words(out), np.stack([interpref.forward(tmp_path, attr[i], T, want[i]) for i in range(2)]), what + " interpolate over it")
        same(words(gb_out), np.stack([gbufref.expected(tmp_path, f, {}, want[i])[3:5] for i, f in enumerate(frames)]), what + " gbuffer(UV) over it")
    # accumulation into a buffer that is not zero: one more term per element
    init = np.random.default_rng(4).normal(0, 5, q.shape).astype(np.float32)
    gq2, _ = bwd(fs, vis, q, gbp, want_bary=False, into=init)
    check_gq(gq2, accs, "into a non-zero buffer", init=init)
    fs.close()


def test_not_fused_strangers_and_hostile_q(ctx, tmp_path):
    """Frames that do not clear and leave pixels to nobody; ids out of range and bare class bits written into the buffer; q with
    zeros, negatives, infinities, NaNs, subnormals and 3e38 in a third of the triangles; edge weights (negative, above 1) in some
    pixels.  Nobody's four words are copied.  With the fused clear nobody's gbary and derivative words become 0; without it the
    sentinel survives on exactly nobody's pixels.  A second buffer holds non-finite alpha, beta, which propagate as IEEE has them."""
    t = soup(3, 40, 96, 80, ZS)
    frames = [frame(t, 96, 80, flags=0), frame(t, 96, 80, flags=0)]
    fs = ctx.frameset(frames)
    vn = visibility(fs).cpu().numpy()
    ids = vn[0, 1].view(np.uint32)
    ids[0, :16], ids[1, :16], ids[2, :16], ids[3, :16], ids[4, :16] = len(t) + 1, 0x7fffffff, 0xffffffff, (len(t) + 1) | 0x80000000, 0x80000000
    rng = np.random.default_rng(5)
    wild = rng.random(vn[:, 2:].shape) < 0.02
    vn[:, 2:][wild] = rng.choice(np.float32([-0.25, 1.5, 1e-40, 0.0]), int(wild.sum()))  # (edge weights; finite, so that gq's sums are)
    vis = torch.as_tensor(vn).cuda()
    vw = vn.view(np.uint32)
    own = owners(vw, frames)
    nobody = ~own[0]
    assert nobody[:5, :16].all() and nobody.sum() > 500 and own[0].sum() > 200
    q = perspref.hostile_q(9, len(t) + 2)
    al, be = vn[0, 2], vn[0, 3]
    idx, s_class = perspref.owners(vw[0], len(t))
    with np.errstate(all="ignore"):
        qq = q[np.where(own[0], idx, 0)]
        one = np.float32(1)
        s = (al * qq[..., 0] + be * qq[..., 1]) + np.where(s_class, (one - al) - be, one - (al + be)) * qq[..., 2]
    invalid = own[0] & ~perspref.valid32(qq, s)
    assert invalid.sum() > 100 and (own[0] & ~invalid).sum() > 100
    want = expect_fwd(tmp_path, frames, vw, q)
    for flags in (F, 0):
        got, _ = fwd(fs, vis, q, flags)
        same(got, want, "hostile forward")
    assert np.array_equal(got[0][:, nobody], vw[0][:, nobody]) and np.array_equal(got[0][:, invalid], vw[0][:, invalid])
    gbp = rand_planes(5, (2, 2, 80, 96), own)
    pos = padded_positions(frames, len(t) + 2)
    attr = rng.normal(0, 2, (len(t) + 2, 3, 2)).astype(np.float32)
    for fl, fused in ((F, True), (0, False)):
        gq, gb = bwd(fs, vis, q, gbp, flags=fl)
        accs, want_gb = expect_bwd(tmp_path, frames, vw, q, gbp, fused)
        same(gb, want_gb, f"hostile gbary fused {fused}")
        assert (gb[0][:, nobody] == (0 if fused else SENTINEL)).all()
        assert np.array_equal(gb[0][:, invalid], gbp[0].view(np.uint32)[:, invalid])  # ga, gb passed through
        assert np.isfinite(accs[0].gq).all()  # (wild alpha, beta meet valid q only where the reference's sums stay finite)
        check_gq(gq, accs, f"hostile gq fused {fused}")
        d = drv(fs, vis, q, attr, fl)
        same(d, expect_drv(tmp_path, frames, vw, q, attr, pos, fused), f"hostile deriv fused {fused}")
        assert (d[0][:, nobody] == (0 if fused else SENTINEL)).all() and (d[0][:, own[0]] != SENTINEL).all()
    # non-finite alpha, beta: the planes, bit for bit (a NaN for a NaN); gq is left out, its reference sums would not be finite
    wild = rng.random(vn[:, 2:].shape) < 0.02
    vn[:, 2:][wild] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 3e38]), int(wild.sum()))
    vis, vw = torch.as_tensor(vn).cuda(), vn.view(np.uint32)
    got, _ = fwd(fs, vis, q)
    same(got, expect_fwd(tmp_path, frames, vw, q), "non-finite alpha, beta")
    assert np.isnan(got.view(np.float32)[:, 2:]).any()
    same(bwd(fs, vis, q, gbp, want_q=False)[1], expect_bwd(tmp_path, frames, vw, q, gbp)[1], "non-finite alpha, beta: gbary")
    same(drv(fs, vis, q, attr), expect_drv(tmp_path, frames, vw, q, attr, pos), "non-finite alpha, beta: deriv")
    fs.close()


# ------------------------------------------------------------------------------------------------------ gq, by construction
@pytest.mark.parametrize("w,h,n", [(96, 96, 2), (50, 37, 2), (64, 64, 9)])
def test_gq_exact_on_dyadic_inputs(ctx, tmp_path, w, h, n):
    """alpha, beta multiples of 1 / 8, the three q of a triangle one power of two (so s = q and alpha' = alpha exactly), integer
    gradients in [-4, 4], q in {0.5, 1, 2}, an integer buffer to add into: every term is a multiple of 1 / 128 below 24 in magnitude, a
    triangle has fewer than 2 000 pixels, and so every partial sum in any order stays below 2^17 = 2^24 / 128: representable, and any
    order of adds gives the same bits.  Nine frames take the walk's other branch: the table is handed from one
    tile to the next"""
    rng = np.random.default_rng([w, n, 3])
    tris = 20
    frames = hand_frames(w, h, n, tris)
    fs = ctx.frameset(frames)
    v = hand_vis(rng, n, h, w, tris, dyadic=True)
    vis = torch.as_tensor(v).cuda()
    shared = n != 2
    q = np.repeat(rng.choice(np.float32([0.5, 1, 2]), ((tris + 1, 1) if shared else (n, tris + 1, 1))), 3, -1)
    gbp = rng.integers(-4, 5, (n, 2, h, w)).astype(np.float32)
    init = rng.integers(-64, 65, q.shape).astype(np.float32)
    gq, gb = bwd(fs, vis, q, gbp, into=init)
    accs, want_gb = expect_bwd(tmp_path, frames, v.view(np.uint32), q, gbp)
    same(gb, want_gb, "dyadic gbary")
    check_gq(gq, accs, f"dyadic {w}x{h} n {n}", exact=True, init=init)
    assert (gq != init).any()
    same(fwd(fs, vis, q)[0], expect_fwd(tmp_path, frames, v.view(np.uint32), q), "dyadic forward")
    fs.close()


def test_table_overflow(ctx, tmp_path):
    """independent random owners per pixel over one 32 x 32 tile: several hundred distinct owners against the table's 128 slots — the
    owners without a slot add straight to memory, and the bound still holds"""
    w = h = 32
    n, tris = 2, 700
    frames = hand_frames(w, h, n, tris)
    fs = ctx.frameset(frames)
    rng = np.random.default_rng(31)
    v = hand_vis(rng, n, h, w, tris, holes=False)
    vis = torch.as_tensor(v).cuda()
    vw = v.view(np.uint32)
    for i in range(n):  # the tile really exceeds the table
        assert perspref.tile_owner_counts(vw[i], tris).max() > 3 * PG_SLOTS
    for q in (perspref.make_q(8, tris), perspref.make_q(8, tris, frames=n)):
        gbp = rand_planes(11, (n, 2, h, w))
        gq, gb = bwd(fs, vis, q, gbp)
        accs, want_gb = expect_bwd(tmp_path, frames, vw, q, gbp)
        same(gb, want_gb, "overflow gbary")
        check_gq(gq, accs, f"overflow {q.ndim}")
        assert (gq != 0).any()
    fs.close()


# ------------------------------------------------------------------------------------------------------ sharded, and a side stream
@pytest.mark.parametrize("world", [2, 3])
def test_sharded(ctx, tmp_path, world):
    import srz
    w, h, tris = 64, 200, 50
    t = np.concatenate([soup(5, tris - 1, w, h, ZS, big=True), BACKDROP])
    frames = [frame(t, w, h), frame(t, w, h)]
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    q = perspref.make_q(12, tris, frames=2)
    gbp = rand_planes(13, (2, 2, h, w))
    attr = np.random.default_rng(14).normal(0, 2, (tris, 3, 2)).astype(np.float32)
    full, _ = fwd(fs, vis, q)
    same(full, expect_fwd(tmp_path, frames, v, q), "whole frame")
    whole_gb = bwd(fs, vis, q, gbp, want_q=False)[1]
    whole_d = drv(fs, vis, q, attr)
    accs, _ = expect_bwd(tmp_path, frames, v, q, gbp)
    fs.close()
    total = np.zeros(q.shape, np.float64)
    for rank in range(world):
        c = srz.Context(0, rank, world)
        sfs = c.frameset(frames)
        svis = visibility(sfs)
        shard, _ = fwd(sfs, svis, q)
        sd = drv(sfs, svis, q, attr)
        rows = parallel.band_rows(h, rank, world)
        sg = np.zeros(sfs.interpolate_shape(2), np.float32)
        for (lb, _, r0, r1) in rows:
            same(shard[:, :, lb * 32: lb * 32 + r1 - r0], full[:, :, r0:r1], f"rank {rank} band {lb}")
            same(sd[:, :, lb * 32: lb * 32 + r1 - r0], whole_d[:, :, r0:r1], f"deriv rank {rank} band {lb}")
            sg[:, :, lb * 32: lb * 32 + r1 - r0] = gbp[:, :, r0:r1]
        part, part_gb = bwd(sfs, svis, q, sg)
        for (lb, _, r0, r1) in rows:
            same(part_gb[:, :, lb * 32: lb * 32 + r1 - r0], whole_gb[:, :, r0:r1], f"gbary rank {rank} band {lb}")
        assert (part != 0).any()
        total += part.astype(np.float64)
        sfs.close(), c.close()
    # each rank's sums lie within the bound of its own adds; the ranks' bounds add up to at most the whole frame's
    err = np.abs(total - np.stack([a.gq for a in accs]))
    bound = np.stack([a.bound() for a in accs])
    assert (err <= bound).all(), float((err - bound).max())


def test_side_stream(ctx, tmp_path):
    frames = pair(100, 70, 60)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    q = perspref.make_q(3, n_tris(frames[0]))
    side = torch.cuda.Stream()
    got, _ = fwd(fs, vis, q, s=side.cuda_stream)
    same(got, expect_fwd(tmp_path, frames, v, q), "side stream")
    fs.close()


# ------------------------------------------------------------------------------------------------------ the torch layer
def test_plain_torch_calls(ctx, tmp_path):
    from srz import visibility as V
    frames = pair(64, 64, 90)
    T = n_tris(frames[0])
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    q = perspref.make_q(2, T, frames=2)
    qd = dev(q)
    pv = V.perspective(fs, vis, qd)
    same(words(pv), expect_fwd(tmp_path, frames, v, q), "perspective()")
    out = torch.empty_like(vis)
    assert V.perspective(fs, vis, qd, out=out) is out and torch.equal(out, pv)
    gbp = rand_planes(3, (2, 2, 64, 64))
    gb, gq = V.perspective_grad(fs, vis, qd, dev(gbp))
    accs, want_gb = expect_bwd(tmp_path, frames, v, q, gbp, fill=0)
    same(words(gb), want_gb, "perspective_grad() gbary")
    check_gq(gq.cpu().numpy(), accs, "perspective_grad() gq")
    assert V.perspective_grad(fs, vis, qd, dev(gbp), want_gq=False)[1] is None
    assert V.perspective_grad(fs, vis, qd, dev(gbp), want_gbary=False)[0] is None
    attr = np.random.default_rng(6).normal(0, 2, (T, 3, 2)).astype(np.float32)
    d = V.interpolate_deriv_persp(fs, vis, dev(attr), qd)
    same(words(d), expect_drv(tmp_path, frames, v, q, attr, padded_positions(frames, T), fill=0), "interpolate_deriv_persp()")
    with pytest.raises(ValueError):
        V.perspective(fs, vis, qd[:, :, :2])
    with pytest.raises(ValueError):
        V.perspective_grad(fs, vis, qd, dev(gbp), want_gbary=False, want_gq=False)
    fs.close()
