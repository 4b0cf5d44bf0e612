"""-m gpu: caller attributes over a visibility buffer and their gradients (srz_frameset_interpolate / _interpolate_grad, k_interp,
k_interp_grad).  The visibility buffer is the GPU's own render_visibility, except where a test writes one by hand; the expected
values are tests/interpref.py's on that buffer (pinned on the CPU by tests/test_interp_ref.py).  Forward and gbary: a NaN on one
side must be a NaN on the other, every other word matches bit for bit.  gattr: exact where every partial sum is representable (the
dyadic cases), else within gamma_n * sum |w g|, gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing pixels — one
rounding per add, the products being float32 products on both sides: derived, not measured."""
import numpy as np
import pytest
import torch

import interpref
from srz import abi, parallel
from support import SENTINEL, ccw, ctx, frame, hostile_shading_frame, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
BACKDROP = ccw((-8, -8), (400, -8), (-8, 400), z=80.0)
SIZES = [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6), (1, 1, 3)]
CHANNELS = (1, 3, 4, 5, 17, 64)


def dims(fs, attr):
    return (attr.shape[0] if attr.ndim == 4 else 1), attr.shape[-3], attr.shape[-1]


def fwd(fs, vis, attr, flags=F, fill=0):
    """the forward pass into a buffer prefilled with the word `fill` → uint32 [n, C, rows, W]"""
    a = torch.as_tensor(np.ascontiguousarray(attr, np.float32)).cuda()
    af, T, C = dims(fs, attr)
    out = torch.full(fs.interpolate_shape(C), fill - (1 << 32) if fill >= 1 << 31 else fill, dtype=torch.int32, device="cuda")
    assert fs.interpolate_bytes(C) == out.numel() * 4
    fs.interpolate(vis.data_ptr(), a.data_ptr(), C, af, T, out.data_ptr(), fs.interpolate_bytes(C), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def bwd(fs, vis, gout, attr, want_attr=True, want_bary=True, flags=F, fill=0, into=None):
    """the backward pass → (gattr float32 of attr's shape, added into `into` or zeros; gbary uint32 [n, 2, rows, W] from `fill`)"""
    a = torch.as_tensor(np.ascontiguousarray(attr, np.float32)).cuda()
    g = torch.as_tensor(np.ascontiguousarray(gout, np.float32)).cuda()
    af, T, C = dims(fs, attr)
    assert tuple(g.shape) == tuple(fs.interpolate_shape(C))
    ga = (torch.zeros_like(a) if into is None else torch.as_tensor(into).cuda()) if want_attr else None
    gb = torch.full(fs.interpolate_shape(2), fill - (1 << 32) if fill >= 1 << 31 else fill, dtype=torch.int32, device="cuda") if want_bary else None
    fs.interpolate_grad(vis.data_ptr(), g.data_ptr(), a.data_ptr(), C, af, T, ga.data_ptr() if want_attr else None,
                        gb.data_ptr() if want_bary else None, flags, stream())
    torch.cuda.synchronize()
    return (ga.cpu().numpy() if want_attr else None), (words(gb) if want_bary else None)


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def n_tris(f):
    return sum(len(t) for t in f.tris)


def attr_of(a, i):
    return a[i] if a.ndim == 4 else a


def expect_fwd(tmp_path, frames, v, attr, fused=True, fill=0):
    out = []
    for i, f in enumerate(frames):
        pre = np.full((attr.shape[-1],) + v.shape[2:], fill, np.uint32)
        out.append(interpref.forward(tmp_path, attr_of(attr, i), n_tris(f), v[i], fused, pre))
    return np.stack(out)


def expect_bwd(tmp_path, frames, v, gout, attr, fused=True, fill=0):
    """(Grad per attribute frame — one for shared attributes —, gbary [n, 2, rows, W] float32)"""
    shared = attr.ndim == 3
    accs = [interpref.Grad(attr.shape[-3:]) for _ in range(1 if shared else len(frames))]
    gb = []
    for i, f in enumerate(frames):
        pre = np.full((2,) + v.shape[2:], fill, np.uint32)
        gb.append(interpref.grad(tmp_path, attr_of(attr, i), n_tris(f), v[i], gout[i], accs[0 if shared else i], True, fused, pre))
    return accs, np.stack(gb)


def check_gattr(got, accs, what, exact=False):
    ref = np.stack([a.gattr for a in accs]).reshape(got.shape)
    bound = np.stack([a.bound() for a in accs]).reshape(got.shape)
    cnt = np.stack([np.broadcast_to(a.count[:, None, None], a.gattr.shape) for a in accs]).reshape(got.shape)
    assert np.isfinite(ref).all()
    if exact:
        assert (ref.astype(np.float32).astype(np.float64) == ref).all(), "the case is not dyadic"
        bound = np.zeros_like(bound)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{what}: max err {err.max():.3e}, max err / bound {np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0:.3f}, "
          f"max n {int(cnt.max())}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    one = cnt == 1
    same((got + np.float32(0))[one], (ref.astype(np.float32) + np.float32(0))[one], what + " (n = 1)")
    assert (got[cnt == 0] == 0).all()


def pair(w, h, n, flags=F, k=2):
    t = np.concatenate([soup(1, n, w, h, ZS, big=w < 40), BACKDROP])
    return [frame(t, w, h, flags=flags) for _ in range(k)]


def rand_attr(seed, shape):
    return np.random.default_rng([seed, 99]).normal(0, 3, shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("w,h,n", SIZES)
def test_forward_sizes_and_channels(ctx, tmp_path, w, h, n):
    frames = pair(w, h, n)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    assert (v[:, 1] != 0).any(1).any(1).all()
    wide = rand_attr(1, (2, n + 3, 3, 64))
    full = fwd(fs, vis, wide, F, SENTINEL)
    same(full, expect_fwd(tmp_path, frames, v, wide, fill=SENTINEL), f"{w}x{h} C 64")
    for C in CHANNELS[:-1]:
        for a in (wide[..., :C], wide[0][..., :C]):  # per frame, shared
            got = fwd(fs, vis, a, F, SENTINEL)
            same(got, expect_fwd(tmp_path, frames, v, a, fill=SENTINEL), f"{w}x{h} C {C} {a.ndim}")
            if a.ndim == 4:
                assert np.array_equal(got, full[:, :C]), C  # every C is a slice of a wider call
    fs.close()


def test_nine_frames_wrap_the_frame_deal(ctx, tmp_path):
    t = np.concatenate([soup(11, 60, 64, 64, ZS), BACKDROP])
    frames = []
    for i in range(9):
        t2 = t.copy()
        t2["pos"][:-1, :, :2] += np.float32([1.5 * i, -1.0 * i])
        frames.append(frame(t2, 64, 64))
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    a = rand_attr(2, (9, 61, 3, 5))
    got = fwd(fs, vis, a, F, SENTINEL)
    same(got, expect_fwd(tmp_path, frames, v, a, fill=SENTINEL), "nine frames")
    assert len({got[i].tobytes() for i in range(9)}) == 9
    gout = np.random.default_rng(3).normal(0, 2, got.shape).astype(np.float32)
    for attr in (a, a[0]):
        ga, gb = bwd(fs, vis, gout, attr, fill=SENTINEL)
        accs, want_gb = expect_bwd(tmp_path, frames, v, gout, attr, fill=SENTINEL)
        same(gb, want_gb, "nine frames gbary")
        check_gattr(ga, accs, f"nine frames gattr {attr.ndim}")
    fs.close()


def test_not_fused_hostile_ids_and_non_finite_values(ctx, tmp_path):
    """frames that do not clear; ids out of range and bare class bits written into the buffer; NaN / inf in attr, alpha and beta"""
    t = soup(3, 40, 96, 80, ZS)
    frames = [frame(t, 96, 80, flags=0), frame(t, 96, 80, flags=0)]
    fs = ctx.frameset(frames)
    v = visibility(fs).cpu().numpy()
    ids = v[0, 1].view(np.uint32)
    ids[0, :16], ids[1, :16], ids[2, :16], ids[3, :16], ids[4, :16] = len(t) + 1, 0x7fffffff, 0xffffffff, (len(t) + 1) | 0x80000000, 0x80000000
    own = (ids != 0) & (((ids & 0x7fffffff) - 1) < len(t))
    ys, xs = np.nonzero(own)
    for j, val in enumerate((np.nan, np.inf, -np.inf)):
        v[0, 2][ys[j::7][:20], xs[j::7][:20]] = val
        v[0, 3][ys[j + 3::7][:20], xs[j + 3::7][:20]] = val
    vis = torch.as_tensor(v).cuda()
    vw = v.view(np.uint32)
    nobody = ~own
    assert nobody[:5, :16].all() and nobody.sum() > 500 and own.sum() > 200
    a = rand_attr(4, (40, 3, 6))
    a[::5, 0, 1], a[1::5, 2, 3], a[2::5, 1, 5] = np.nan, np.inf, -np.inf
    fused, kept = fwd(fs, vis, a, F, SENTINEL), fwd(fs, vis, a, 0, SENTINEL)
    same(fused, expect_fwd(tmp_path, frames, vw, a, True, SENTINEL), "fused")
    same(kept, expect_fwd(tmp_path, frames, vw, a, False, SENTINEL), "not fused")
    assert (fused[0][:, nobody] == 0).all() and (kept[0][:, nobody] == SENTINEL).all()  # exactly the owned words change
    assert (kept[0][:, own] != SENTINEL).all() and np.isnan(fused.view(np.float32)).any()
    gout = np.random.default_rng(5).normal(0, 2, fused.shape).astype(np.float32)
    for fl, fused_ in ((F, True), (0, False)):
        _, gb = bwd(fs, vis, gout, a, want_attr=False, flags=fl, fill=SENTINEL)
        same(gb, expect_bwd(tmp_path, frames, vw, gout, a, fused_, SENTINEL)[1], f"gbary fused {fused_}")
    fs.close()


@pytest.mark.parametrize("unified", [False, True])
def test_cross_checks_against_the_gbuffer_and_the_depth_plane(ctx, unified):
    flags = F | (abi.UNIFIED if unified else 0)
    frames = [frame(np.concatenate([soup(0, 90, 64, 64, ZS), BACKDROP]), 64, 64, flags=flags), hostile_shading_frame(0, "uv-edge", tame=True, flags=flags)]
    fs = ctx.frameset(frames)
    vis = visibility(fs, flags)
    v = words(vis)
    T = max(n_tris(f) for f in frames)
    uv, pos = np.zeros((2, T, 3, 2), np.float32), np.zeros((2, T, 3, 3), np.float32)
    for i, f in enumerate(frames):
        uv[i, :n_tris(f)], pos[i, :n_tris(f)] = interpref.frame_attr(f, "uv"), interpref.frame_attr(f, "pos")
    gb = torch.zeros(fs.gbuffer_shape(abi.GB_UV), dtype=torch.float32, device="cuda")
    fs.gbuffer(vis.data_ptr(), gb.data_ptr(), fs.gbuffer_bytes(abi.GB_UV), abi.GB_UV, F, stream())
    torch.cuda.synchronize()
    same(fwd(fs, vis, uv), words(gb), "uv against gbuffer(UV)")
    own, s_class = v[:, 1] != 0, (v[:, 1] >> 31) != 0
    assert own.sum() > 4000 and (s_class.any() != unified)
    assert np.array_equal(fwd(fs, vis, pos)[:, 2][own], v[:, 0][own])
    fs.close()


# ------------------------------------------------------------------------------------------------------ backward, exact
def run_ids(rng, n, h, w, tris, max_run, holes=True):
    """[n, h, w] id words: runs of 1 .. max_run pixels of one owner over the raster (they straddle quads, rows, tiles and bands),
    either class, some pixels nobody's"""
    total = n * h * w
    lens = rng.integers(1, max_run + 1, total)
    owner = rng.integers(1, tris + 1, total).astype(np.uint32)
    ids = np.repeat(owner, lens)[:total]
    ids |= (rng.random(total) < 0.4).astype(np.uint32) << 31
    if holes:
        ids[rng.random(total) < 0.1] = 0
    return ids.reshape(n, h, w)


def dyadic(rng, ids):
    """a visibility buffer [n, 4, h, w] float32 with these ids and alpha, beta multiples of 1/8, alpha + beta <= 1"""
    al = rng.integers(0, 9, ids.shape)
    be = (rng.integers(0, 9, ids.shape) * (8 - al)) // 8
    v = np.zeros((ids.shape[0], 4) + ids.shape[1:], np.float32)
    v[:, 1] = ids.view(np.float32)
    v[:, 2], v[:, 3] = al / 8.0, be / 8.0
    return v


def dyadic_case(name):
    """(w, h, frames, triangles, ids [n, h, w], shared attributes)"""
    rng = np.random.default_rng([len(name), 5])
    if name == "one owner, nine frames":
        return 64, 64, 9, 5, np.full((9, 64, 64), 3, np.uint32), True
    if name == "1024 owners in a tile":
        return 32, 32, 1, 1024, (rng.permutation(1024).astype(np.uint32) + 1).reshape(1, 32, 32), True
    if name == "runs, mixed classes":
        return 96, 96, 2, 300, run_ids(rng, 2, 96, 96, 300, 13), False
    if name == "long runs":
        return 96, 96, 2, 7, run_ids(rng, 2, 96, 96, 7, 150), True
    if name == "partial tiles":
        return 50, 37, 2, 40, run_ids(rng, 2, 37, 50, 40, 9), False
    raise KeyError(name)


DYADIC = ("one owner, nine frames", "1024 owners in a tile", "runs, mixed classes", "long runs", "partial tiles")


@pytest.mark.parametrize("name", DYADIC)
@pytest.mark.parametrize("C", [1, 5, 8])
def test_backward_exact_on_dyadic_inputs(ctx, tmp_path, name, C):
    """alpha, beta multiples of 1/8, integer gout in [-16, 16], integer attr: every partial sum is representable, any order of adds
    gives the same bits"""
    w, h, n, tris, ids, shared = dyadic_case(name)
    rng = np.random.default_rng([C, 17])
    frames = [frame(soup(1, tris, w, h, ZS), w, h) for _ in range(n)]
    fs = ctx.frameset(frames)
    v = dyadic(rng, ids)
    vis = torch.as_tensor(v).cuda()
    attr = rng.integers(-8, 9, ((tris + 1, 3, C) if shared else (n, tris + 1, 3, C))).astype(np.float32)
    gout = rng.integers(-16, 17, (n, C, h, w)).astype(np.float32)
    ga, gb = bwd(fs, vis, gout, attr, fill=SENTINEL)
    accs, want_gb = expect_bwd(tmp_path, frames, v.view(np.uint32), gout, attr, fill=SENTINEL)
    same(gb, want_gb, name + " gbary")
    check_gattr(ga, accs, name, exact=True)
    assert (ga != 0).any()
    same(fwd(fs, vis, attr), expect_fwd(tmp_path, frames, v.view(np.uint32), attr), name + " forward")
    fs.close()


# ------------------------------------------------------------------------------------------------------ backward, rendered
@pytest.mark.parametrize("w,h,n", SIZES[:3])
def test_backward_on_rendered_buffers(ctx, tmp_path, w, h, n):
    frames = pair(w, h, n)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    own = v[:, 1] != 0
    for C in (3, 17):
        attr = rand_attr(C, (2, n + 1, 3, C))
        gout = np.random.default_rng([C, 8]).normal(0, 2, (2, C, h, w)).astype(np.float32)
        gout[np.broadcast_to(~own[:, None], gout.shape)] = np.nan  # nobody's words may hold anything
        for a in (attr, attr[1]):
            ga, gb = bwd(fs, vis, gout, a)
            accs, want_gb = expect_bwd(tmp_path, frames, v, gout, a)
            assert np.isfinite(ga).all()
            same(gb, want_gb, f"gbary C {C}")
            check_gattr(ga, accs, f"{w}x{h} C {C} {a.ndim}")
            only_gb = bwd(fs, vis, gout, a, want_attr=False)[1]
            assert np.array_equal(only_gb, gb)
    # accumulation: a second call into the first one's result is twice one call (the bound of 2 n adds on twice the sums)
    ga2, _ = bwd(fs, vis, gout, attr, want_bary=False, into=bwd(fs, vis, gout, attr, want_bary=False)[0])
    accs, _ = expect_bwd(tmp_path, frames, v, gout, attr)
    for a in accs:
        a.gattr *= 2
        a.gabs *= 2
        a.count *= 2
    err = np.abs(ga2.astype(np.float64) - np.stack([a.gattr for a in accs]))
    assert (err <= np.stack([a.bound() for a in accs])).all()
    fs.close()


# ------------------------------------------------------------------------------------------------------ sharded
def test_sharded_world_2(ctx, tmp_path):
    import srz
    w, h, tris = 64, 128, 50
    t = np.concatenate([soup(5, tris - 1, w, h, ZS, big=True), BACKDROP])
    frames = [frame(t, w, h), frame(t, w, h)]
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    attr = rand_attr(6, (tris, 3, 5))
    full = fwd(fs, vis, attr)
    rng = np.random.default_rng(12)
    hv = dyadic(rng, run_ids(rng, 2, h, w, tris, 40))
    iattr = rng.integers(-8, 9, (tris, 3, 5)).astype(np.float32)
    gout = rng.integers(-16, 17, (2, 5, h, w)).astype(np.float32)
    whole, whole_gb = bwd(fs, torch.as_tensor(hv).cuda(), gout, iattr)
    fs.close()
    total = np.zeros_like(whole)
    for rank in (0, 1):
        c = srz.Context(0, rank, 2)
        sfs = c.frameset(frames)
        svis = visibility(sfs)
        shard = fwd(sfs, svis, attr)
        rows = parallel.band_rows(h, rank, 2)
        assert len(rows) == 2
        sv = np.zeros(sfs.out_shape, np.float32)
        sg = np.zeros(sfs.interpolate_shape(5), np.float32)
        for (lb, _, r0, r1) in rows:
            same(shard[:, :, lb * 32: lb * 32 + r1 - r0], full[:, :, r0:r1], f"rank {rank} band {lb}")
            sv[:, :, lb * 32: lb * 32 + r1 - r0], sg[:, :, lb * 32: lb * 32 + r1 - r0] = hv[:, :, r0:r1], gout[:, :, r0:r1]
        part, part_gb = bwd(sfs, torch.as_tensor(sv).cuda(), sg, iattr)
        for (lb, _, r0, r1) in rows:
            same(part_gb[:, :, lb * 32: lb * 32 + r1 - r0], whole_gb[:, :, r0:r1], f"gbary rank {rank} band {lb}")
        total += part
        sfs.close(), c.close()
    assert np.array_equal(total, whole) and (whole != 0).any()


# ------------------------------------------------------------------------------------------------------ autograd
def test_autograd(ctx, monkeypatch):
    import srz
    from srz.visibility import decode, interpolate, interpolate_bary_grad
    frames = pair(100, 70, 120)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    calls = []
    real = srz.FrameSet.interpolate_grad
    monkeypatch.setattr(srz.FrameSet, "interpolate_grad", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    for shape in ((121, 3, 6), (2, 121, 3, 6)):
        attr = torch.as_tensor(rand_attr(9, shape)).cuda().requires_grad_(True)
        out = interpolate(fs, vis, attr)
        assert out.shape == (2, 6, 70, 100) and out.requires_grad
        out.square().sum().backward()
        torch.cuda.synchronize()
        d = decode(vis)
        g = (2 * out.detach())  # float32: what the backward was handed
        wts = torch.stack([d.alpha, d.beta, d.gamma], 1)  # [n, 3, H, W]
        own = d.tri >= 0
        ref, mag = torch.zeros(shape, dtype=torch.float64, device="cuda"), torch.zeros(shape, dtype=torch.float64, device="cuda")
        cnt = torch.zeros(shape[:-2], dtype=torch.float64, device="cuda")
        for i in range(2):
            r, m, c = (ref[i], mag[i], cnt[i]) if len(shape) == 4 else (ref, mag, cnt)
            idx = d.tri[i][own[i]]
            prod = (wts[i][:, None] * g[i][None])[:, :, own[i]].to(torch.float64)  # [3, C, owned]: float32 products, widened
            r.index_add_(0, idx, prod.permute(2, 0, 1))
            m.index_add_(0, idx, prod.abs().permute(2, 0, 1))
            c.index_add_(0, idx, torch.ones_like(idx, dtype=torch.float64))
        nu = cnt[..., None, None] * 2.0 ** -24
        bound = nu / (1 - nu) * mag
        err = (attr.grad.to(torch.float64) - ref).abs()
        assert bool((err <= bound).all()), float((err - bound).max())
        # the raw call: the same shape and the same zero pattern
        raw = torch.zeros_like(attr)
        fs.interpolate_grad(vis.data_ptr(), g.contiguous().data_ptr(), None, 6, shape[0] if len(shape) == 4 else 1, 121, raw.data_ptr(), None, F, stream())
        torch.cuda.synchronize()
        assert raw.shape == attr.grad.shape and torch.equal(raw == 0, attr.grad == 0) and bool((attr.grad != 0).any())
        gb = interpolate_bary_grad(fs, vis, attr.detach(), g)
        assert gb.shape == (2, 2, 70, 100) and bool((gb[:, 0][~own] == 0).all()) and bool((gb[:, 1][~own] == 0).all()) and bool((gb != 0).any())
    n = len(calls)
    out = interpolate(fs, vis, attr.detach())
    assert not out.requires_grad and out.grad_fn is None and len(calls) == n  # no backward is there to launch
    fs.close()


# ------------------------------------------------------------------------------------------------------ misuse
def test_misuse(ctx):
    import srz
    L = srz.lib()
    t = soup(1, 60, 64, 64, ZS)
    fs = ctx.frameset([frame(t, 64, 64), frame(t[:50], 64, 64)])
    vis = visibility(fs)
    C, T = 4, 60
    attr = torch.zeros((2, T, 3, C), dtype=torch.float32, device="cuda")
    big = torch.full((2 * 8 * 64 * 64 + 8,), 5, dtype=torch.int32, device="cuda")  # outputs are carved from this
    gout = torch.zeros(fs.interpolate_shape(C), dtype=torch.float32, device="cuda")
    nb, h, e = fs.interpolate_bytes(C), ctx.h, abi.SRZ_E_INVALID
    v, a, o, g = vis.data_ptr(), attr.data_ptr(), big.data_ptr(), gout.data_ptr()
    o2 = o + 2 * 2 * 64 * 64 * 4 + 16  # a second output behind a gbary-sized first one
    assert fs.interpolate_bytes(0) == 0 and fs.interpolate_bytes(65) == 0 and nb == 2 * C * 64 * 64 * 4 and fs.interpolate_bytes(64) == 16 * nb

    def f(vis=v, attr=a, n_ch=C, af=2, at=T, out=o, ob=nb, flags=F, ctxh=h, fsh=fs.h):
        return L.srz_frameset_interpolate(ctxh, fsh, vis, attr, n_ch, af, at, out, ob, flags, None)

    def b(vis=v, gout=g, attr=a, n_ch=C, af=2, at=T, gattr=o2, gbary=o, flags=F, ctxh=h, fsh=fs.h):
        return L.srz_frameset_interpolate_grad(ctxh, fsh, vis, gout, attr, n_ch, af, at, gattr, gbary, flags, None)
    bad_f = [dict(ctxh=None), dict(fsh=None), dict(vis=None), dict(attr=None), dict(out=None), dict(n_ch=0), dict(n_ch=65), dict(af=0), dict(af=3),
             dict(at=59), dict(at=0), dict(vis=v + 4), dict(out=o + 4), dict(attr=a + 2), dict(ob=nb - 4), dict(out=v), dict(out=v + 64 * 64 * 4),
             dict(out=a), dict(attr=o + 16)]
    bad_b = [dict(ctxh=None), dict(fsh=None), dict(vis=None), dict(gout=None), dict(gattr=None, gbary=None), dict(attr=None), dict(n_ch=0),
             dict(n_ch=65), dict(af=0), dict(af=3), dict(at=59), dict(vis=v + 4), dict(gout=g + 4), dict(gbary=o + 4), dict(gattr=o2 + 2),
             dict(attr=a + 2), dict(gbary=v), dict(gattr=v + 32), dict(gbary=g), dict(gattr=g + 32), dict(gattr=a), dict(gbary=a), dict(gattr=o + 32)]
    for flag in (abi.UNIFIED, abi.ORDERED_RASTER, abi.NO_Z_READBACK, 16, F | abi.UNIFIED):
        bad_f.append(dict(flags=flag)), bad_b.append(dict(flags=flag))
    for kw in bad_f:
        assert f(**kw) == e, kw
    for kw in bad_b:
        assert b(**kw) == e, kw
    torch.cuda.synchronize()
    assert (big == 5).all() and (attr == 0).all() and (gout == 0).all()
    assert f() == 0 and b() == 0 and b(attr=None, gbary=None) == 0 and b(gattr=None) == 0 and f(af=1) == 0 and f(at=61, af=1) == 0
    torch.cuda.synchronize()
    fs.close()
