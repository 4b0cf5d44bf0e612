"""-m gpu: caller textures over a visibility buffer and their gradients (srz_frameset_texture / _texture_grad, k_tex, k_tex_grad).
The visibility buffer is the GPU's own render_visibility, except where a test writes one by hand; uv is the GPU's own interpolate of
the frames' uv, except where a test writes the planes by hand; the expected values are tests/texref.py's on those very buffers
(pinned on the CPU by tests/test_tex_ref.py).  Forward and guv: a NaN on one side must be a NaN on the other, every other word
matches bit for bit.  gtex: exact where every partial sum is representable (the dyadic cases) and where an element has one
contributing add, else within gamma_n * sum |w g|, gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing adds — one
rounding per add, the products being float32 products on both sides: derived, not measured."""
import numpy as np
import pytest
import torch

import interpref
import texref
from srz import abi, parallel
from support import SENTINEL, ccw, ctx, filled, frame, soup, stream, visibility, words  # noqa: F401
from texref import CLAMP, WRAP

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = texref.ZS
BACKDROP = ccw((-8, -8), (400, -8), (-8, 400), z=80.0, uv=((0.1, 0.2), (0.9, 0.3), (0.4, 0.95)))
SIZES = [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6), (1, 1, 3)]
CHANNELS = (1, 3, 4, 5, 17, 64)
TG_SLOTS = 2048  # the capacity of k_tex_grad's table of distinct texels per tile


def n_tris(f):
    return f if isinstance(f, int) else sum(len(t) for t in f.tris)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def interp_uv(fs, vis, frames):
    """the GPU's interpolate of the frames' own uv → the planes on the device [n, 2, rows, W] (zeros where nobody owns the pixel) and
    the attributes [n, T, 3, 2] they came from"""
    T = max(n_tris(f) for f in frames)
    a = np.zeros((len(frames), T, 3, 2), np.float32)
    for i, f in enumerate(frames):
        a[i, :n_tris(f)] = texref.frame_uv(f)
    out, a_dev = torch.zeros(fs.interpolate_shape(2), dtype=torch.float32, device="cuda"), dev(a)
    fs.interpolate(vis.data_ptr(), a_dev.data_ptr(), 2, len(frames), T, out.data_ptr(), fs.interpolate_bytes(2), F, stream())
    torch.cuda.synchronize()
    return out, a


def tex_dims(fs, tex):
    return (tex.shape[0] if tex.ndim == 4 else 1), tex.shape[-3], tex.shape[-2], tex.shape[-1]


def fwd(fs, vis, uv, tex, mode, flags=F, fill=0):
    """the forward pass into a buffer prefilled with the word `fill` → uint32 [n, C, rows, W]"""
    tf, h, w, C = tex_dims(fs, tex)
    out, t = filled(fs.interpolate_shape(C), fill), dev(tex)
    fs.texture(vis.data_ptr(), uv.data_ptr(), t.data_ptr(), w, h, C, tf, mode, out.data_ptr(), fs.interpolate_bytes(C), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def bwd(fs, vis, uv, gout, tex, mode, want_tex=True, want_uv=True, flags=F, fill=0, into=None):
    """the backward pass → (gtex float32 of tex's shape, added into `into` or zeros; guv uint32 [n, 2, rows, W] from `fill`)"""
    tf, h, w, C = tex_dims(fs, tex)
    t, g = dev(tex), dev(gout)
    assert tuple(g.shape) == tuple(fs.interpolate_shape(C))
    gt = (torch.zeros_like(t) if into is None else dev(into)) if want_tex else None
    gu = filled(fs.interpolate_shape(2), fill) if want_uv else None
    fs.texture_grad(vis.data_ptr(), uv.data_ptr(), g.data_ptr(), t.data_ptr(), w, h, C, tf, mode, gt.data_ptr() if want_tex else None,
                    gu.data_ptr() if want_uv else None, flags, stream())
    torch.cuda.synchronize()
    return (gt.cpu().numpy() if want_tex else None), (words(gu) if want_uv else None)


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def tex_of(t, i):
    return t[i] if t.ndim == 4 else t


def expect_fwd(tmp_path, frames, v, uvw, tex, mode, fused=True, fill=0):
    """v: the visibility buffer's words [n, 4, rows, W]; uvw: the uv planes float32 [n, 2, rows, W]"""
    out = []
    for i, f in enumerate(frames):
        pre = np.full((tex.shape[-1],) + v.shape[2:], fill, np.uint32)
        out.append(texref.forward(tmp_path, tex_of(tex, i), mode, n_tris(f), v[i, 1], uvw[i], fused, pre))
    return np.stack(out)


def expect_bwd(tmp_path, frames, v, uvw, gout, tex, mode, fused=True, fill=0):
    """(Grad per texture frame — one for a shared texture —, guv [n, 2, rows, W] float32)"""
    shared = tex.ndim == 3
    accs = [texref.Grad(tex.shape[-3:]) for _ in range(1 if shared else len(frames))]
    gu = []
    for i, f in enumerate(frames):
        pre = np.full((2,) + v.shape[2:], fill, np.uint32)
        gu.append(texref.grad(tmp_path, tex_of(tex, i), mode, n_tris(f), v[i, 1], uvw[i], gout[i], accs[0 if shared else i], True, fused, pre))
    return accs, np.stack(gu)


def check_gtex(got, accs, what, exact=False, init=None):
    """init: what the buffer held before the call (one more term of every element's sum)"""
    ref = np.stack([a.gtex for a in accs]).reshape(got.shape)
    mag = np.stack([a.gabs for a in accs]).reshape(got.shape)
    cnt = np.stack([np.broadcast_to(a.count[:, :, None], a.gtex.shape) for a in accs]).reshape(got.shape).astype(np.float64)
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
          f"max n {int(cnt.max())}, elements with one add {int((cnt == 1).sum())}, untouched {int((cnt == 0).sum())}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    one = cnt == 1
    same((got + np.float32(0))[one], (ref.astype(np.float32) + np.float32(0))[one], what + " (n = 1)")
    assert (got[cnt == 0] == 0).all()


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


# ------------------------------------------------------------------------------------------------------ forward and guv
@pytest.mark.parametrize("w,h,n", SIZES)
def test_forward_and_guv_sizes_and_channels(ctx, tmp_path, w, h, n):
    frames = pair(w, h, n)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    assert (v[:, 1] != 0).any(1).any(1).all()
    uv, _ = interp_uv(fs, vis, frames)
    uvw = uv.cpu().numpy()
    own = owners(v, frames)
    for mode in (CLAMP, WRAP):
        wide = texref.make_tex(1, 5, 7, 64, frames=2)
        gwide = rand_gout(mode, (2, 64, h, w), own)
        full = fwd(fs, vis, uv, wide, mode, F, SENTINEL)
        same(full, expect_fwd(tmp_path, frames, v, uvw, wide, mode, fill=SENTINEL), f"{w}x{h} C 64 mode {mode}")
        for C in CHANNELS:
            for t in (wide[..., :C], wide[0][..., :C]):  # per frame, shared
                got = fwd(fs, vis, uv, t, mode, F, SENTINEL)
                same(got, expect_fwd(tmp_path, frames, v, uvw, t, mode, fill=SENTINEL), f"{w}x{h} C {C} {t.ndim} mode {mode}")
                if t.ndim == 4:
                    assert np.array_equal(got, full[:, :C]), C  # every C is a slice of a wider call
                _, gu = bwd(fs, vis, uv, gwide[:, :C], t, mode, want_tex=False, fill=SENTINEL)
                same(gu, expect_bwd(tmp_path, frames, v, uvw, gwide[:, :C], t, mode, fill=SENTINEL)[1], f"guv {w}x{h} C {C} {t.ndim} mode {mode}")
    fs.close()


@pytest.mark.parametrize("name", texref.FRAME_CASES)
def test_frame_cases_every_texture_size_both_modes(ctx, tmp_path, name):
    """soup's uv, random_frame's beyond [0, 1], the hostile families' at, far beyond and not on the number line; textures 1 x 1 ..
    64 x 64, shared and per frame; forward and guv bit for bit, gtex within its bound"""
    f = texref.case_frame(name)
    frames = [f, f]
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    uv, _ = interp_uv(fs, vis, frames)
    uvw = uv.cpu().numpy()
    own = owners(v, frames)
    assert own.sum() >= 400
    if name in texref.NON_FINITE_CASES:
        assert (~np.isfinite(uvw).all(1) & own).sum() >= 40
    k = 0
    for (tw, th) in texref.TEX_SIZES:
        for mode in (CLAMP, WRAP):
            C = CHANNELS[k % len(CHANNELS)]
            tex = texref.make_tex(k, tw, th, C, frames=2)
            tex = tex if k % 2 else tex[0]
            k += 1
            what = f"{name} {tw}x{th} C {C} mode {mode} {tex.ndim}"
            got = fwd(fs, vis, uv, tex, mode, F, SENTINEL)
            same(got, expect_fwd(tmp_path, frames, v, uvw, tex, mode, fill=SENTINEL), what)
            assert (got[np.broadcast_to(~own[:, None], got.shape)] == 0).all()
            gout = rand_gout(k, got.shape, own)
            gt, gu = bwd(fs, vis, uv, gout, tex, mode, fill=SENTINEL)
            accs, want_gu = expect_bwd(tmp_path, frames, v, uvw, gout, tex, mode, fill=SENTINEL)
            same(gu, want_gu, what + " guv")
            assert np.isfinite(gt).all()
            check_gtex(gt, accs, what + " gtex")
            only_gu = bwd(fs, vis, uv, gout, tex, mode, want_tex=False, fill=SENTINEL)[1]
            assert np.array_equal(only_gu, gu)
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
    uv, _ = interp_uv(fs, vis, frames)
    uvw = uv.cpu().numpy()
    for tex in (texref.make_tex(4, 33, 9, 5, frames=9), texref.make_tex(4, 33, 9, 5)):
        got = fwd(fs, vis, uv, tex, WRAP, F, SENTINEL)
        same(got, expect_fwd(tmp_path, frames, v, uvw, tex, WRAP, fill=SENTINEL), "nine frames")
        gout = rand_gout(3, got.shape)
        gt, gu = bwd(fs, vis, uv, gout, tex, WRAP, fill=SENTINEL)
        accs, want_gu = expect_bwd(tmp_path, frames, v, uvw, gout, tex, WRAP, fill=SENTINEL)
        same(gu, want_gu, "nine frames guv")
        check_gtex(gt, accs, f"nine frames gtex {tex.ndim}")
    assert len({got[i].tobytes() for i in range(9)}) == 9
    fs.close()


def test_not_fused_hand_written_ids_and_uv(ctx, tmp_path):
    """frames that do not clear; ids out of range and bare class bits written into the buffer; uv planes written by hand: NaN, inf,
    3e38 and values on the borders under owners, NaN under nobody"""
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
    uvw = rng.uniform(-0.5, 1.5, (2, 2, 80, 96)).astype(np.float32)
    special = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, 1.0, -0.0, 0.5, 1.0 - 2.0 ** -24, 1e-40])
    hit = rng.random(uvw.shape) < 0.3
    uvw[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    uvw[np.broadcast_to(~own[:, None], uvw.shape)] = np.nan  # never read
    uv = dev(uvw)
    unsampled = own & ~np.isfinite(uvw).all(1)
    assert unsampled.sum() >= 200
    tex = texref.make_tex(6, 5, 7, 6)
    for mode in (CLAMP, WRAP):
        fused, kept = fwd(fs, vis, uv, tex, mode, F, SENTINEL), fwd(fs, vis, uv, tex, mode, 0, SENTINEL)
        same(fused, expect_fwd(tmp_path, frames, vw, uvw, tex, mode, True, SENTINEL), "fused")
        same(kept, expect_fwd(tmp_path, frames, vw, uvw, tex, mode, False, SENTINEL), "not fused")
        assert (fused[0][:, nobody] == 0).all() and (kept[0][:, nobody] == SENTINEL).all()  # exactly the owned words change
        assert (kept[0][:, own[0]] != SENTINEL).all() and (kept[:, :][np.broadcast_to(unsampled[:, None], kept.shape)] == 0).all()
        gout = rand_gout(5 + mode, fused.shape, own)
        for fl, fused_ in ((F, True), (0, False)):
            gt, gu = bwd(fs, vis, uv, gout, tex, mode, flags=fl, fill=SENTINEL)
            accs, want_gu = expect_bwd(tmp_path, frames, vw, uvw, gout, tex, mode, fused_, SENTINEL)
            same(gu, want_gu, f"guv fused {fused_}")
            assert (gu[0][:, nobody] == (0 if fused_ else SENTINEL)).all()
            check_gtex(gt, accs, f"gtex fused {fused_} mode {mode}")
    fs.close()


def test_non_finite_texels_and_gradients_propagate(ctx, tmp_path):
    frames = pair(64, 64, 90)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    uv, _ = interp_uv(fs, vis, frames)
    uvw = uv.cpu().numpy()
    tex = texref.make_tex(7, 5, 7, 4)
    tex[1, 2, 0], tex[3, 3, 1], tex[6, 0, 2] = np.nan, np.inf, -np.inf
    got = fwd(fs, vis, uv, tex, CLAMP)
    same(got, expect_fwd(tmp_path, frames, v, uvw, tex, CLAMP), "non-finite texels")
    assert np.isnan(got.view(np.float32)).any()
    gout = rand_gout(9, got.shape)
    _, gu = bwd(fs, vis, uv, gout, tex, CLAMP, want_tex=False)
    same(gu, expect_bwd(tmp_path, frames, v, uvw, gout, tex, CLAMP)[1], "non-finite texels guv")
    fs.close()


# ------------------------------------------------------------------------------------------------------ gtex, by construction
def hand_frames(w, h, n, tris):
    return [frame(soup(1, tris, w, h, ZS), w, h) for _ in range(n)]


def hand_vis(ids):
    """a visibility buffer [n, 4, h, w] float32 with these id words (z, alpha, beta: zeros — the texture passes read none of them)"""
    v = np.zeros((ids.shape[0], 4) + ids.shape[1:], np.float32)
    v[:, 1] = ids.view(np.float32)
    return v


def rand_ids(rng, n, h, w, tris, holes=True):
    ids = rng.integers(1, tris + 1, (n, h, w)).astype(np.uint32)
    ids |= (rng.random((n, h, w)) < 0.4).astype(np.uint32) << 31
    if holes:
        ids[rng.random((n, h, w)) < 0.1] = 0
    return ids


@pytest.mark.parametrize("mode", [CLAMP, WRAP])
@pytest.mark.parametrize("C", [1, 5, 8])
@pytest.mark.parametrize("w,h,n,tw,th", [(96, 96, 2, 16, 8), (50, 37, 2, 4, 4), (64, 64, 9, 32, 32)])
def test_gtex_exact_on_dyadic_inputs(ctx, tmp_path, mode, C, w, h, n, tw, th):
    """texture sizes powers of two and uv = (i + 0.5 + k / 8) / size: tx and ty are multiples of 1/8, the weights of 1/64; integer
    gout in [-16, 16], an integer buffer to add into: every partial sum is representable, any order of adds gives the same bits"""
    rng = np.random.default_rng([C, w, mode])
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    ids = rand_ids(rng, n, h, w, 20)
    v = hand_vis(ids)
    vis = torch.as_tensor(v).cuda()
    lo = -2 if mode == WRAP else 0  # (WRAP: whole periods away too; u - floorf(u) is exact on this grid)
    uvw = np.stack([(rng.integers(lo * tw, (1 - lo) * tw, (n, h, w)) + 0.5 + rng.integers(0, 8, (n, h, w)) / 8.0) / tw,
                    (rng.integers(lo * th, (1 - lo) * th, (n, h, w)) + 0.5 + rng.integers(0, 8, (n, h, w)) / 8.0) / th], 1).astype(np.float32)
    uv = dev(uvw)
    shared = n != 2
    tex = rng.integers(-8, 9, ((th, tw, C) if shared else (n, th, tw, C))).astype(np.float32)
    gout = rng.integers(-16, 17, (n, C, h, w)).astype(np.float32)
    init = rng.integers(-64, 65, tex.shape).astype(np.float32)
    gt, gu = bwd(fs, vis, uv, gout, tex, mode, fill=SENTINEL, into=init)
    accs, want_gu = expect_bwd(tmp_path, frames, v.view(np.uint32), uvw, gout, tex, mode, fill=SENTINEL)
    same(gu, want_gu, "dyadic guv")
    check_gtex(gt, accs, f"dyadic {w}x{h} tex {tw}x{th} C {C} mode {mode}", exact=True, init=init)
    assert (gt != init).any()
    same(fwd(fs, vis, uv, tex, mode), expect_fwd(tmp_path, frames, v.view(np.uint32), uvw, tex, mode), "dyadic forward")
    fs.close()


def regime(name):
    """(frame w, h, texture w, h, uv planes [2, h, w] float32, distinct texels the busiest tile touches) for the three regimes of
    k_tex_grad's table of TG_SLOTS distinct texels per 32 x 32 tile"""
    if name == "a handful of texels":  # the frames' pixels over one eighth of a 64 x 64 texture: a tile spans 4 x 4 texels, touches 6 x 6
        w = h = 64
        xs, ys = np.meshgrid(np.arange(w), np.arange(h))
        return w, h, 64, 64, np.stack([(xs + 0.37) / (8 * 64) + 0.25, (ys + 0.61) / (8 * 64) + 0.5]).astype(np.float32), 36
    if name == "at the capacity":  # a 64 x 32 texture under one tile: pixel (x, y) on the centre of texel (2 x, y), x1 = 2 x + 1, y1 = min(y + 1, 31)
        w = h = 32
        xs, ys = np.meshgrid(np.arange(w), np.arange(h))
        return w, h, 64, 32, np.stack([(2 * xs + 0.5) / 64, (ys + 0.5) / 32]).astype(np.float32), 64 * 32
    if name == "far over the capacity":  # a 256 x 256 texture minified across one tile: every pixel has four texels of its own
        w = h = 32
        xs, ys = np.meshgrid(np.arange(w), np.arange(h))
        return w, h, 256, 256, np.stack([(xs + 0.5) / 32, (ys + 0.5) / 32]).astype(np.float32), 4 * 32 * 32
    raise KeyError(name)


@pytest.mark.parametrize("name", ["a handful of texels", "at the capacity", "far over the capacity"])
def test_gtex_in_the_three_regimes_of_the_table(ctx, tmp_path, name):
    w, h, tw, th, uv1, distinct = regime(name)
    assert (distinct < TG_SLOTS // 8, distinct == TG_SLOTS, distinct >= 2 * TG_SLOTS) == \
        (name == "a handful of texels", name == "at the capacity", name == "far over the capacity")
    n, C = 2, 5
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    ids = rand_ids(np.random.default_rng(31), n, h, w, 20, holes=False)
    v = hand_vis(ids)
    vis = torch.as_tensor(v).cuda()
    uvw = np.stack([uv1] * n)
    uv = dev(uvw)
    # the busiest tile touches what the construction says (counted from the reference's own taps: each add names its texel)
    probe = texref.Grad((th, tw, 1))
    texref.grad(tmp_path, np.zeros((th, tw, 1), np.float32), CLAMP, 20, v.view(np.uint32)[0, 1][:32, :32], uvw[0][:, :32, :32],
                np.ones((1, 32, 32), np.float32), probe, False)
    assert int((probe.count > 0).sum()) == distinct and int(probe.count.sum()) == 4 * 32 * 32
    for tex in (texref.make_tex(8, tw, th, C), texref.make_tex(8, tw, th, C, frames=n)):
        gout = rand_gout(11, (n, C, h, w))
        gt, gu = bwd(fs, vis, uv, gout, tex, CLAMP, fill=SENTINEL)
        accs, want_gu = expect_bwd(tmp_path, frames, v.view(np.uint32), uvw, gout, tex, CLAMP, fill=SENTINEL)
        same(gu, want_gu, name + " guv")
        check_gtex(gt, accs, f"{name} {tex.ndim}")
        assert (gt != 0).any()
    fs.close()


@pytest.mark.parametrize("w,h,n", SIZES[:3])
def test_gtex_on_rendered_buffers_and_accumulation(ctx, tmp_path, w, h, n):
    frames = pair(w, h, n)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    uv, _ = interp_uv(fs, vis, frames)
    uvw = uv.cpu().numpy()
    own = owners(v, frames)
    for C in (3, 17):
        for tex in (texref.make_tex(C, 64, 64, C, frames=2), texref.make_tex(C, 2, 2, C)):
            gout = rand_gout(C, (2, C, h, w), own)
            gt, gu = bwd(fs, vis, uv, gout, tex, WRAP)
            accs, want_gu = expect_bwd(tmp_path, frames, v, uvw, gout, tex, WRAP)
            same(gu, want_gu, f"guv C {C}")
            check_gtex(gt, accs, f"{w}x{h} C {C} {tex.ndim}")
            only_gt = bwd(fs, vis, uv, gout, tex, WRAP, want_uv=False)[0]
            check_gtex(only_gt, accs, f"{w}x{h} C {C} {tex.ndim} gtex alone")
    # accumulation into a buffer that is not zero: one more term per element
    init = np.random.default_rng(4).normal(0, 5, tex.shape).astype(np.float32)
    gt2, _ = bwd(fs, vis, uv, gout, tex, WRAP, want_uv=False, into=init)
    check_gtex(gt2, accs, "into a non-zero buffer", init=init)
    assert (gt2 != init).any()
    fs.close()


# ------------------------------------------------------------------------------------------------------ sharded
def test_sharded_world_2(ctx, tmp_path):
    import srz
    w, h, tris = 64, 128, 50
    t = np.concatenate([soup(5, tris - 1, w, h, ZS, big=True), BACKDROP])
    frames = [frame(t, w, h), frame(t, w, h)]
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    uv, _ = interp_uv(fs, vis, frames)
    uvw = uv.cpu().numpy()
    tex = texref.make_tex(12, 5, 7, 5)
    gout = rand_gout(13, (2, 5, h, w))
    full = fwd(fs, vis, uv, tex, WRAP)
    same(full, expect_fwd(tmp_path, frames, v, uvw, tex, WRAP), "whole frame")
    whole_gu = bwd(fs, vis, uv, gout, tex, WRAP, want_tex=False)[1]
    accs, _ = expect_bwd(tmp_path, frames, v, uvw, gout, tex, WRAP)
    fs.close()
    total = np.zeros(tex.shape, np.float64)
    for rank in (0, 1):
        c = srz.Context(0, rank, 2)
        sfs = c.frameset(frames)
        svis = visibility(sfs)
        suv, _ = interp_uv(sfs, svis, frames)
        shard = fwd(sfs, svis, suv, tex, WRAP)
        rows = parallel.band_rows(h, rank, 2)
        assert len(rows) == 2
        sg = np.zeros(sfs.interpolate_shape(5), np.float32)
        for (lb, _, r0, r1) in rows:
            same(shard[:, :, lb * 32: lb * 32 + r1 - r0], full[:, :, r0:r1], f"rank {rank} band {lb}")
            sg[:, :, lb * 32: lb * 32 + r1 - r0] = gout[:, :, r0:r1]
        part, part_gu = bwd(sfs, svis, suv, sg, tex, WRAP)
        for (lb, _, r0, r1) in rows:
            same(part_gu[:, :, lb * 32: lb * 32 + r1 - r0], whole_gu[:, :, r0:r1], f"guv rank {rank} band {lb}")
        assert (part != 0).any()
        total += part.astype(np.float64)
        sfs.close(), c.close()
    # each rank's sums lie within the bound of its own adds; the two bounds add up to at most the whole frame's
    err = np.abs(total - accs[0].gtex)
    assert (err <= accs[0].bound()).all(), float((err - accs[0].bound()).max())


# ------------------------------------------------------------------------------------------------------ the chain, autograd
def test_guv_chains_into_interpolate_grad(ctx, tmp_path):
    frames = pair(100, 70, 120)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    uv, attr = interp_uv(fs, vis, frames)
    uvw = uv.cpu().numpy()
    tex = texref.make_tex(14, 33, 9, 4)
    gout = rand_gout(15, (2, 4, 70, 100), owners(v, frames))
    guv, g_dev, t_dev = filled(fs.interpolate_shape(2), SENTINEL), dev(gout), dev(tex)
    fs.texture_grad(vis.data_ptr(), uv.data_ptr(), g_dev.data_ptr(), t_dev.data_ptr(), 33, 9, 4, 1, WRAP, None, guv.data_ptr(), F, stream())
    want_gu = expect_bwd(tmp_path, frames, v, uvw, gout, tex, WRAP, fill=SENTINEL)[1]
    torch.cuda.synchronize()
    same(words(guv), want_gu, "guv")
    gattr = torch.zeros(attr.shape, dtype=torch.float32, device="cuda")
    fs.interpolate_grad(vis.data_ptr(), guv.data_ptr(), None, 2, 2, attr.shape[1], gattr.data_ptr(), None, F, stream())
    torch.cuda.synchronize()
    got = gattr.cpu().numpy()
    for i, f in enumerate(frames):
        acc = interpref.Grad(attr.shape[1:])
        interpref.grad(tmp_path, attr[i], n_tris(f), v[i], want_gu[i], into=acc, want_bary=False)
        err = np.abs(got[i].astype(np.float64) - acc.gattr)
        assert (err <= acc.bound()).all() and (got[i][acc.count == 0] == 0).all() and (acc.gattr != 0).sum() > 100
    fs.close()


def test_autograd(ctx, tmp_path, monkeypatch):
    import srz
    from srz.visibility import interpolate, texture, texture_grad
    frames = pair(100, 70, 120)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    uv, attr = interp_uv(fs, vis, frames)
    uvw = uv.cpu().numpy()
    calls = []
    real = srz.FrameSet.texture_grad
    monkeypatch.setattr(srz.FrameSet, "texture_grad", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    for wrap in (False, True):
        for shape in ((7, 5, 6), (2, 7, 5, 6)):
            texn = np.random.default_rng(16).normal(0, 3, shape).astype(np.float32)
            tex = dev(texn).requires_grad_(True)
            uvt = uv.clone().requires_grad_(True)
            out = texture(fs, vis, tex, uvt, wrap=wrap)
            assert out.shape == (2, 6, 70, 100) and out.requires_grad
            same(words(out.detach()), fwd(fs, vis, uv, texn, int(wrap)), "forward")
            out.square().sum().backward()
            torch.cuda.synchronize()
            g = (2 * out.detach()).contiguous()  # float32: what the backward was handed
            gt, gu = texture_grad(fs, vis, tex.detach(), uv, g, wrap=wrap)
            same(words(uvt.grad), words(gu), "uv.grad")
            accs, want_gu = expect_bwd(tmp_path, frames, v, uvw, g.cpu().numpy(), texn, int(wrap))
            same(words(gu), want_gu, "plain guv")
            check_gtex(tex.grad.cpu().numpy(), accs, "tex.grad")
            check_gtex(gt.cpu().numpy(), accs, "plain gtex")
    # through interpolate: the loss reaches the uv attributes
    a = dev(attr).requires_grad_(True)
    tex = dev(texn).requires_grad_(True)
    n = len(calls)
    out = texture(fs, vis, tex, interpolate(fs, vis, a), wrap=True)
    same(words(out.detach()), fwd(fs, vis, uv, texn, WRAP), "composed forward")
    out.square().sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == n + 1  # one call for both gradients
    g = (2 * out.detach()).contiguous().cpu().numpy()
    accs, want_gu = expect_bwd(tmp_path, frames, v, uvw, g, texn, WRAP)
    check_gtex(tex.grad.cpu().numpy(), accs, "composed tex.grad")
    got = a.grad.cpu().numpy()
    for i, f in enumerate(frames):
        acc = interpref.Grad(attr.shape[1:])
        interpref.grad(tmp_path, attr[i], n_tris(f), v[i], want_gu[i], into=acc, want_bary=False)
        assert (np.abs(got[i].astype(np.float64) - acc.gattr) <= acc.bound()).all() and (got[i] != 0).sum() > 100
    # nothing needs a gradient: no backward is there to launch; one input does: the call asks for that output alone
    n = len(calls)
    out = texture(fs, vis, tex.detach(), uv)
    assert not out.requires_grad and out.grad_fn is None and len(calls) == n
    uvt = uv.clone().requires_grad_(True)
    texture(fs, vis, tex.detach(), uvt).sum().backward()
    assert len(calls) == n + 1 and uvt.grad is not None
    fs.close()
