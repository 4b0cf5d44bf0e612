"""-m gpu: the Cook-Torrance pass over a visibility buffer and its gradients (srz_frameset_microfacet / _microfacet_grad, k_microfacet,
k_microfacet_grad, k_light_fold).  The visibility buffer is the GPU's own render_visibility, except where a test writes one by hand;
the normals are the GPU's own interpolate of the frames' normals, the positions a hand-written linear ramp, except where a test writes
the planes by hand; the expected values are tests/microfacetref.py's on those very buffers (pinned on the CPU by
tests/test_microfacet_ref.py).  Forward, gnrm, gpos, gbase, gmat: a NaN on one side must be a NaN on the other, every other word
matches bit for bit.  gpar: within gamma_n * sum |term| of the reference's double sums, gamma_n = n u / (1 - n u), u = 2^-24, n the
entry's contributing pixels — the bound of any summation tree, the terms being the rule's float32 terms on both sides: derived, not
measured —, bit-equal between two launches, and the float32 term itself where one pixel contributes."""
import numpy as np
import pytest
import torch

import microfacetref as mf
import vgkit
from srz import abi, parallel
from support import SENTINEL, ccw, ctx, filled, frame, scene_pair, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
BACKDROP = ccw((-8, -8), (400, -8), (-8, 400), z=80.0, uv=((0.1, 0.2), (0.9, 0.3), (0.4, 0.95)))
BACKDROP["nrm"] = np.float32([(0.3, -0.3, 0.9), (-0.4, 0.2, 0.8), (0.1, -0.2, 0.95)])
SIZES = [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6), (1, 1, 3)]
LIGHTS = (1, 3, 8)
ALL = (True, True, True, True, True)  # want: gnrm, gpos, gbase, gmat, gpar
PLANES_ONLY = (True, True, True, True, False)
GPAR_ONLY = (False, False, False, False, True)


def n_tris(f):
    return f if isinstance(f, int) else sum(len(t) for t in f.tris)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def interp_normals(fs, vis, frames):
    """the GPU's interpolate of the frames' own normals → the planes on the device [n, 3, rows, W] (zeros where nobody owns the pixel)"""
    T = max(n_tris(f) for f in frames)
    a = np.zeros((len(frames), T, 3, 3), np.float32)
    for i, f in enumerate(frames):
        a[i, :n_tris(f)] = np.concatenate([t["nrm"] for t in f.tris])
    out, a_dev = torch.zeros(fs.interpolate_shape(3), dtype=torch.float32, device="cuda"), dev(a)
    fs.interpolate(vis.data_ptr(), a_dev.data_ptr(), 3, len(frames), T, out.data_ptr(), fs.interpolate_bytes(3), F, stream())
    torch.cuda.synchronize()
    return out


def ramp(n, h, w):
    """positions by hand: a linear ramp over the frame, x and y in [-1, 1), z a tilted plane that differs per frame → [n, 3, h, w]"""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x, y = 2 * xs / max(w, 2) - 1, 2 * ys / max(h, 2) - 1
    return np.float32(np.stack([np.stack([x, y, 0.1 * x - 0.2 * y + 0.05 * i]) for i in range(n)]))


def rand_planes(seed, n, h, w, own=None):
    """(base in (0.1, 1) [n, 3, h, w], mat over [-0.1, 1.1] [n, 2, h, w], gout normal [n, 3, h, w]); nobody's words NaN: they may hold
    anything"""
    rng = np.random.default_rng([seed, 8])
    base, g = rng.uniform(0.1, 1.0, (n, 3, h, w)).astype(np.float32), rng.normal(0, 2, (n, 3, h, w)).astype(np.float32)
    mat = rng.uniform(-0.1, 1.1, (n, 2, h, w)).astype(np.float32)
    if own is not None:
        for t in (base, mat, g):
            t[np.broadcast_to(~own[:, None], t.shape)] = np.nan
    return base, mat, g


def owners(v, frames):
    return np.stack([((v[i, 1] & 0x7fffffff) - np.uint32(1)) < n_tris(f) for i, f in enumerate(frames)])


def pair(w, h, n, flags=F, k=2):
    t = np.concatenate([soup(1, n, w, h, ZS, big=w < 40), BACKDROP])
    return [frame(t, w, h, flags=flags) for _ in range(k)]


def hand_frames(w, h, n, tris):
    return [frame(soup(1, tris, w, h, ZS), w, h) for _ in range(n)]


def hand_vis(ids):
    v = np.zeros((ids.shape[0], 4) + ids.shape[1:], np.float32)
    v[:, 1] = ids.view(np.float32)
    return v


def par_dims(par):
    par = np.ascontiguousarray(par, np.float32)
    return par, (par.shape[-1] - 6) // 6, (par.shape[0] if par.ndim == 2 else 1)


def ptr(t):
    return None if t is None else t.data_ptr()


def fwd(fs, vis, nrm, pos, base, mat, par, flags=F, fill=0):
    """the forward pass into a buffer prefilled with the word `fill` → uint32 [n, 3, rows, W]; the planes: device tensors (base None)"""
    par, L, pf = par_dims(par)
    out, pt = filled(fs.interpolate_shape(3), fill), dev(par)
    fs.microfacet(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), ptr(base), mat.data_ptr(), pt.data_ptr(), L, pf, out.data_ptr(),
                  fs.interpolate_bytes(3), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def bwd(fs, vis, nrm, pos, base, mat, par, gout, want=ALL, flags=F, fill=0):
    """the backward pass → (gnrm, gpos, gbase [n, 3, rows, W], gmat [n, 2, rows, W] uint32 from `fill`, gpar float32 of par's shape
    from SENTINEL words); None where not wanted (gbase: and without base)"""
    par, L, pf = par_dims(par)
    pt, g = dev(par), dev(gout)
    want = list(want)
    want[2] = want[2] and base is not None
    planes = [filled(fs.interpolate_shape(2 if i == 3 else 3), fill) if w else None for i, w in enumerate(want[:4])]
    gpar = filled((pf, mf.par_len(L)), SENTINEL) if want[4] else None
    nbytes = fs.microfacet_work_bytes(L) if want[4] else 0
    work = filled((nbytes // 4,), SENTINEL) if want[4] else None
    fs.microfacet_grad(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), ptr(base), mat.data_ptr(), pt.data_ptr(), L, pf, g.data_ptr(),
                       *(ptr(t) for t in planes), ptr(gpar), ptr(work), nbytes, flags, stream())
    torch.cuda.synchronize()
    return tuple(None if t is None else words(t) for t in planes) + (None if gpar is None else words(gpar).view(np.float32),)


def par_of(par, i):
    return par[i] if par.ndim == 2 else par


def expect_fwd(tmp_path, frames, v, nw, pw, bw, mw, par, fused=True, fill=0):
    """v: the visibility buffer's words [n, 4, rows, W]; nw, pw, bw: the planes float32 [n, 3, rows, W] (bw None), mw [n, 2, rows, W]"""
    out = []
    for i, f in enumerate(frames):
        pre = np.full((3,) + v.shape[2:], fill, np.uint32)
        out.append(mf.forward(tmp_path, n_tris(f), v[i, 1], nw[i], pw[i], None if bw is None else bw[i], mw[i], par_of(par, i), fused, pre))
    return np.stack(out)


def expect_bwd(tmp_path, frames, v, nw, pw, bw, mw, par, gout, fused=True, fill=0):
    """(Grad per parameter frame — one for a shared block —, [gnrm, gpos, gbase, gmat] each [n, planes, rows, W] float32, gbase None
    without base)"""
    par = np.ascontiguousarray(par, np.float32)
    shared = par.ndim == 1
    L = (par.shape[-1] - 6) // 6
    accs = [mf.Grad(L) for _ in range(1 if shared else len(frames))]
    planes = []
    for i, f in enumerate(frames):
        pre = np.full((3,) + v.shape[2:], fill, np.uint32)
        planes.append(mf.grad(tmp_path, n_tris(f), v[i, 1], nw[i], pw[i], None if bw is None else bw[i], mw[i], par_of(par, i), gout[i],
                              accs[0 if shared else i], fused, pre))
    return accs, [None if planes[0][k] is None else np.stack([q[k] for q in planes]) for k in range(4)]


def check_gpar(got, accs, what, extra=0):
    ref, bound = np.stack([a.gsum for a in accs]), np.stack([a.bound(extra) for a in accs])
    cnt = np.stack([a.count for a in accs])
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(ref).all()
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    print(f"{what}: max err {err.max():.3e}, max err / bound {ratio:.3f}, max n {int(cnt.max())}, untouched {int((cnt == 0).sum())}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} entries beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    assert (got[cnt == 0] == 0).all()


def check_planes(got, want, what):
    for name, g, w in zip(("gnrm", "gpos", "gbase", "gmat"), got, want):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            same(g, w, f"{what} {name}")


def rendered(ctx, w, h, n, k=2):
    frames = pair(w, h, n, F, k)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    assert (v[:, 1] != 0).any(1).any(1).all()
    nrm = interp_normals(fs, vis, frames)
    return frames, fs, vis, v, nrm, nrm.cpu().numpy(), owners(v, frames)


# ------------------------------------------------------------------------------------------------------ forward and the planes
@pytest.mark.parametrize("w,h,n", SIZES)
def test_forward_and_plane_gradients(ctx, tmp_path, w, h, n):
    """every light count, base given and null, shared and per-frame parameters; at the three larger sizes gpar too: within its bound,
    the same words from a second launch, every entry overwritten"""
    frames, fs, vis, v, nrm, nw, own = rendered(ctx, w, h, n)
    pw = ramp(2, h, w)
    pos = dev(pw)
    bw, mw, gout = rand_planes(w, 2, h, w, own)
    base, mat = dev(bw), dev(mw)
    lit_any = False
    for L in LIGHTS:
        both = mf.make_params(w + L, L, frames=2)
        for par in (both, both[0]):
            for b_dev, b_np in ((base, bw), (None, None)):
                what = f"{w}x{h} L {L} par {par.ndim} base {b_np is not None}"
                got = fwd(fs, vis, nrm, pos, b_dev, mat, par, F, SENTINEL)
                same(got, expect_fwd(tmp_path, frames, v, nw, pw, b_np, mw, par, fill=SENTINEL), what)
                assert (got[np.broadcast_to(~own[:, None], got.shape)] == 0).all()
                lit_any |= bool((got != 0).any())
                want_par = w * h >= 1000
                res = bwd(fs, vis, nrm, pos, b_dev, mat, par, gout, (True, True, True, True, want_par), fill=SENTINEL)
                accs, planes = expect_bwd(tmp_path, frames, v, nw, pw, b_np, mw, par, gout, fill=SENTINEL)
                check_planes(res[:4], planes, what)
                if want_par:
                    assert not (res[4].view(np.uint32) == SENTINEL).any()  # written, every entry
                    check_gpar(res[4], accs, what + " gpar")
                    again = bwd(fs, vis, nrm, pos, b_dev, mat, par, gout, GPAR_ONLY)[4]
                    assert np.array_equal(again.view(np.uint32), res[4].view(np.uint32)), what + ": two launches differ"
    assert lit_any
    # each want flag alone gives the same words as all together
    par = mf.make_params(5, 3, frames=2)
    every = bwd(fs, vis, nrm, pos, base, mat, par, gout, fill=SENTINEL)
    for k in range(5):
        alone = bwd(fs, vis, nrm, pos, base, mat, par, gout, tuple(i == k for i in range(5)), fill=SENTINEL)
        assert all(alone[i] is None for i in range(5) if i != k)
        assert np.array_equal(alone[k].view(np.uint32), every[k].view(np.uint32)), k
    fs.close()


def test_nine_frames_wrap_the_frame_deal(ctx, tmp_path):
    """eight frames and more take the walk's other branch (workgroup b serves the frames f = b mod 8): with nine frames of four tiles
    the 40 workgroups stride 5 tiles, so a workgroup goes on from a tile of frame 0 to one of frame 8 — its LDS partials are reused"""
    t = np.concatenate([soup(11, 60, 64, 64, ZS), BACKDROP])
    frames = []
    for i in range(9):
        t2 = t.copy()
        t2["pos"][:-1, :, :2] += np.float32([1.5 * i, -1.0 * i])
        frames.append(frame(t2, 64, 64))
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    nrm = interp_normals(fs, vis, frames)
    nw, pw = nrm.cpu().numpy(), ramp(9, 64, 64)
    pos = dev(pw)
    bw, mw, gout = rand_planes(2, 9, 64, 64, owners(v, frames))
    base, mat = dev(bw), dev(mw)
    per = mf.make_params(4, 3, frames=9)
    rows = None
    for par in (per, per[0]):
        got = fwd(fs, vis, nrm, pos, base, mat, par, F, SENTINEL)
        same(got, expect_fwd(tmp_path, frames, v, nw, pw, bw, mw, par, fill=SENTINEL), "nine frames")
        res = bwd(fs, vis, nrm, pos, base, mat, par, gout, fill=SENTINEL)
        accs, planes = expect_bwd(tmp_path, frames, v, nw, pw, bw, mw, par, gout, fill=SENTINEL)
        check_planes(res[:4], planes, "nine frames")
        check_gpar(res[4], accs, f"nine frames gpar {par.ndim}")
        rows = res[4] if par.ndim == 2 else rows
    assert len({got[i].tobytes() for i in range(9)}) == 9 and len({rows[i].tobytes() for i in range(9)}) == 9
    fs.close()


def test_shared_parameters_are_the_frame_order_sum_of_the_per_frame_rows(ctx, tmp_path):
    """include/srz.h states it, so it is checkable bit for bit: one parameter frame for every frame gives, per entry, 0 + row 0 + row 1 +
    ... in float32 of the rows the call with that frame repeated per frame writes"""
    for k in (2, 9):
        frames, fs, vis, v, nrm, nw, own = rendered(ctx, 64, 64, 90, k=k)
        pos = dev(ramp(k, 64, 64))
        bw, mw, gout = rand_planes(3, k, 64, 64, own)
        base, mat = dev(bw), dev(mw)
        one = mf.make_params(9, 3)
        shared = bwd(fs, vis, nrm, pos, base, mat, one, gout, GPAR_ONLY)[4]
        rows = bwd(fs, vis, nrm, pos, base, mat, np.repeat(one[None], k, 0), gout, GPAR_ONLY)[4]
        s = np.zeros(rows.shape[1], np.float32)
        for i in range(k):
            s = s + rows[i]
        assert shared.shape == (1, rows.shape[1]) and np.array_equal(shared[0].view(np.uint32), s.view(np.uint32)) and (s != 0).all()
        fs.close()


# ------------------------------------------------------------------------------------------------------ hostile planes
def test_hostile_planes_under_a_hand_written_buffer(ctx, tmp_path):
    """planes written by hand (microfacetref.hostile_case) under a hand-written visibility buffer with holes: light's nine kinds, and
    roughness and metallic at and beyond each clamp edge, NaN, +-inf and subnormal, nv <= 0, N = Vd = Ld: every branch of the rule is
    met by at least 50 pixels (tests/test_microfacet_ref.py checks the count of these very inputs on the CPU), and every word matches"""
    n, h, w, tris = (mf.HOSTILE[k] for k in ("n", "h", "w", "tris"))
    ids, par, nw, pw, bw, mw, gout, kind = mf.hostile_case(**mf.HOSTILE)
    for name, m in mf.branches(tmp_path, tris, ids, nw, pw, bw, mw, gout, kind, par).items():
        assert int(m.sum()) >= 50, (name, int(m.sum()))
    frames = hand_frames(w, h, n, tris)
    fs = ctx.frameset(frames)
    v = hand_vis(ids)
    vw = v.view(np.uint32)
    vis = torch.as_tensor(v).cuda()
    own = owners(vw, frames)
    lit = np.stack([(mf.classify(tmp_path, tris, ids[i], nw[i], pw[i], mw[i], par)[0] & mf.LIT) != 0 for i in range(n)])
    nrm, pos, base, mat = dev(nw), dev(pw), dev(bw), dev(mw)
    for b_dev, b_np in ((base, bw), (None, None)):
        got = fwd(fs, vis, nrm, pos, b_dev, mat, par, F, SENTINEL)
        same(got, expect_fwd(tmp_path, frames, vw, nw, pw, b_np, mw, par, fill=SENTINEL), "hostile forward")
        assert (got[np.broadcast_to((own & ~lit)[:, None], got.shape)] == 0).all()
        res = bwd(fs, vis, nrm, pos, b_dev, mat, par, gout, PLANES_ONLY, fill=SENTINEL)
        _, planes = expect_bwd(tmp_path, frames, vw, nw, pw, b_np, mw, par, gout, fill=SENTINEL)
        check_planes(res[:4], planes, "hostile")
    assert np.isnan(got.view(np.float32)).any() or np.isnan(res[0].view(np.float32)).any()
    # gpar with base and gout made finite (a NaN term would make the whole entry a NaN on both sides: nothing to bound), per frame and
    # shared (3e38 is finite and overflows in the first product: it goes too); the material stays hostile: its clamps make it finite
    bf, gf = np.where(np.abs(bw) < 1e6, bw, np.float32(0.5)), np.where(np.abs(gout) < 1e6, gout, np.float32(-1.5))
    for bp in (par, np.stack([par, mf.hostile_params(3)])):
        res = bwd(fs, vis, nrm, pos, dev(bf), mat, bp, gf, fill=SENTINEL)
        accs, planes = expect_bwd(tmp_path, frames, vw, nw, pw, bf, mw, bp, gf, fill=SENTINEL)
        check_planes(res[:4], planes, "hostile finite")
        check_gpar(res[4], accs, f"hostile gpar {bp.ndim}")
    fs.close()


# ------------------------------------------------------------------------------------------------------ gpar
def test_gpar_of_one_pixel_is_its_float32_term(ctx, tmp_path):
    """exactly one owned pixel in the set (n = 1): every add of the tree adds +0, so each entry is the pixel's float32 term, bit for
    bit (+ 0.0f on both sides: a term of -0 comes out +0, as the header says); the entries of a light skipped there are +0"""
    w, h = 70, 40
    frames = hand_frames(w, h, 2, 20)
    fs = ctx.frameset(frames)
    for (fi, y, x) in ((0, 0, 0), (1, 37, 69), (0, 33, 31)):
        ids = np.zeros((2, h, w), np.uint32)
        ids[fi, y, x] = 5
        v = hand_vis(ids)
        nw, pw, bw, mw, gout = (np.stack([t, t]) for t in mf.make_planes(7, (h, w)))
        nw[fi, :, y, x] = (0.2, -0.4, 2.0)  # facing the lights and the eye: no term of the pixel is 0 by a branch
        mw[fi, :, y, x] = (0.4, 0.3)
        par = mf.make_params(3, 3)
        par[12:15] = pw[fi, :, y, x]  # light 1 exactly at the pixel: skipped
        res = bwd(fs, torch.as_tensor(v).cuda(), dev(nw), dev(pw), dev(bw), dev(mw), par, gout)
        acc = mf.Grad(3)
        terms = mf.grad(tmp_path, 20, ids[fi], nw[fi], pw[fi], bw[fi], mw[fi], par, gout[fi], into=acc, want_terms=True)[4]
        t = terms[:, y, x]
        assert (acc.count[np.r_[0:12, 18:24]] == 1).all() and not acc.count[12:18].any() and (t[np.r_[0:12, 18:24]] != 0).all()
        same(res[4][0] + np.float32(0), t + np.float32(0), f"one pixel {fi} {y} {x}")
        assert not res[4][0][12:18].view(np.uint32).any()
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
    par = mf.hostile_params(4)
    nw, pw, bw, mw, gout, _ = (np.stack(t) for t in zip(*(mf.hostile_planes(rng, (80, 96), par) for _ in range(2))))
    for t in (nw, pw, bw, mw, gout):
        t[np.broadcast_to(~own[:, None], t.shape)] = np.nan  # never read
    nrm, pos, base, mat = dev(nw), dev(pw), dev(bw), dev(mw)
    fused, kept = fwd(fs, vis, nrm, pos, base, mat, par, F, SENTINEL), fwd(fs, vis, nrm, pos, base, mat, par, 0, SENTINEL)
    same(fused, expect_fwd(tmp_path, frames, vw, nw, pw, bw, mw, par, True, SENTINEL), "fused")
    same(kept, expect_fwd(tmp_path, frames, vw, nw, pw, bw, mw, par, False, SENTINEL), "not fused")
    assert (fused[0][:, nobody] == 0).all() and (kept[0][:, nobody] == SENTINEL).all() and (kept[0][:, own[0]] != SENTINEL).all()
    for fl, fused_ in ((F, True), (0, False)):
        res = bwd(fs, vis, nrm, pos, base, mat, par, gout, PLANES_ONLY, flags=fl, fill=SENTINEL)
        _, planes = expect_bwd(tmp_path, frames, vw, nw, pw, bw, mw, par, gout, fused_, SENTINEL)
        check_planes(res[:4], planes, f"fused {fused_}")
        for q in res[:4]:
            assert (q[0][:, nobody] == (0 if fused_ else SENTINEL)).all()
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
    nrm = interp_normals(fs, vis, frames)
    nw, pw = nrm.cpu().numpy(), ramp(2, h, w)
    bw, mw, gout = rand_planes(13, 2, h, w)
    par = mf.make_params(12, 3)
    full = fwd(fs, vis, nrm, dev(pw), dev(bw), dev(mw), par)
    same(full, expect_fwd(tmp_path, frames, v, nw, pw, bw, mw, par), "whole frame")
    whole = bwd(fs, vis, nrm, dev(pw), dev(bw), dev(mw), par, gout)
    accs, planes = expect_bwd(tmp_path, frames, v, nw, pw, bw, mw, par, gout)
    check_planes(whole[:4], planes, "whole frame")
    check_gpar(whole[4], accs, "whole frame gpar")
    fs.close()
    total = np.zeros(whole[4].shape, np.float64)
    for rank in (0, 1):
        c = srz.Context(0, rank, 2)
        sfs = c.frameset(frames)
        svis = visibility(sfs)
        snrm = interp_normals(sfs, svis, frames)
        rows = parallel.band_rows(h, rank, 2)
        assert len(rows) == 2
        local = [np.zeros(sfs.interpolate_shape(k), np.float32) for k in (3, 3, 2, 3)]
        for (lb, _, r0, r1) in rows:
            for dst, src in zip(local, (pw, bw, mw, gout)):
                dst[:, :, lb * 32: lb * 32 + r1 - r0] = src[:, :, r0:r1]
        spos, sbase, smat, sg = local
        shard = fwd(sfs, svis, snrm, dev(spos), dev(sbase), dev(smat), par)
        part = bwd(sfs, svis, snrm, dev(spos), dev(sbase), dev(smat), par, sg)
        for (lb, _, r0, r1) in rows:
            same(shard[:, :, lb * 32: lb * 32 + r1 - r0], full[:, :, r0:r1], f"rank {rank} band {lb}")
            for k in range(4):
                same(part[k][:, :, lb * 32: lb * 32 + r1 - r0], whole[k][:, :, r0:r1], f"plane {k} rank {rank} band {lb}")
        assert (part[4] != 0).all()
        total += part[4].astype(np.float64)
        sfs.close(), c.close()
    # each rank's sums lie within the bound of its own pixels; the two bounds add up to at most the whole frame's
    err = np.abs(total - accs[0].gsum)
    assert (err <= accs[0].bound()).all(), float((err - accs[0].bound()).max())


def test_a_rank_without_bands_writes_every_row_of_gpar():
    """rank 1 of world 2 on a 32-row frame holds no band (its 32 local rows are padding): no tile, no kernel over tiles — and still
    d_gpar is WRITTEN, +0 in every entry (the caller adds the ranks' rows), with per-frame and with shared parameters; no word of
    the planes is touched"""
    import srz
    assert len(parallel.band_rows(32, 1, 2)) == 0 and len(parallel.band_rows(32, 0, 2)) == 1
    c = srz.Context(0, 1, 2)
    sfs = c.frameset(hand_frames(64, 32, 2, 20))
    shape = sfs.interpolate_shape(3)
    vis = torch.zeros(sfs.out_shape, dtype=torch.float32, device="cuda")
    nrm, pos, base, g = (torch.ones(shape, dtype=torch.float32, device="cuda") for _ in range(4))
    mat = torch.full(sfs.interpolate_shape(2), 0.5, dtype=torch.float32, device="cuda")
    outs = [filled(shape, SENTINEL) for _ in range(3)] + [filled(sfs.interpolate_shape(2), SENTINEL)]
    L = 3
    nbytes = sfs.microfacet_work_bytes(L)
    assert nbytes == 2 * mf.par_len(L) * 4  # no partials, a row per frame
    for pf in (2, 1):
        par = dev(mf.make_params(3, L, frames=2)[:pf])
        gpar, work = filled((pf, mf.par_len(L)), SENTINEL), filled((nbytes // 4,), SENTINEL)
        sfs.microfacet_grad(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), base.data_ptr(), mat.data_ptr(), par.data_ptr(), L, pf, g.data_ptr(),
                            *(t.data_ptr() for t in outs), gpar.data_ptr(), work.data_ptr(), nbytes, F, stream())
        torch.cuda.synchronize()
        assert not words(gpar).any(), (pf, words(gpar))
    # the forward and the planes-only backward have nothing to do there, and say so by succeeding
    sfs.microfacet(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), base.data_ptr(), mat.data_ptr(), par.data_ptr(), L, 1, outs[0].data_ptr(),
                   sfs.interpolate_bytes(3), F, stream())
    sfs.microfacet_grad(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), base.data_ptr(), mat.data_ptr(), par.data_ptr(), L, 1, g.data_ptr(),
                        outs[0].data_ptr(), None, None, None, None, None, 0, F, stream())
    torch.cuda.synchronize()
    assert all((words(t) == SENTINEL).all() for t in outs)
    sfs.close(), c.close()


# ------------------------------------------------------------------------------------------------------ autograd, the chain, a fit
def test_autograd(ctx, tmp_path, monkeypatch):
    import srz
    from srz.visibility import microfacet, microfacet_grad, microfacet_params
    frames, fs, vis, v, nrm, nw, own = rendered(ctx, 100, 70, 120)
    pw = ramp(2, 70, 100)
    bw, mw, _ = rand_planes(6, 2, 70, 100)
    pos, base, mat = dev(pw), dev(bw), dev(mw)
    calls = []
    real = srz.FrameSet.microfacet_grad
    monkeypatch.setattr(srz.FrameSet, "microfacet_grad", lambda self, *a, **k: (calls.append(a), real(self, *a, **k))[1])
    for per_frame in (False, True):
        parn = mf.make_params(16, 3, frames=2)
        parn[1, :6] = parn[0, :6]  # eye, amb shared; the lights per frame or shared
        parn = parn if per_frame else parn[0]
        row = parn[0] if per_frame else parn
        lights = dev(parn[..., 6:].reshape((2, 3, 6) if per_frame else (3, 6))).requires_grad_(True)
        eye, amb = (dev(row[i:i + 3]).requires_grad_(True) for i in (0, 3))
        nt, pt, bt, mt = (t.clone().requires_grad_(True) for t in (nrm, pos, base, mat))
        n0 = len(calls)
        out = microfacet(fs, vis, nt, pt, bt, mt, lights, eye, amb)
        assert out.shape == (2, 3, 70, 100) and out.requires_grad
        same(words(out.detach()), fwd(fs, vis, nrm, pos, base, mat, parn), "forward")
        out.square().sum().backward()
        torch.cuda.synchronize()
        assert len(calls) == n0 + 1  # one launch for every gradient
        g = (2 * out.detach()).contiguous()
        block = microfacet_params(fs, lights.detach(), eye.detach(), amb.detach())
        assert tuple(block.shape) == ((2, 24) if per_frame else (1, 24))
        gn, gp, gb, gm, gpar = microfacet_grad(fs, vis, nrm, pos, base, mat, block, g)
        for name, a, b in (("nrm", nt.grad, gn), ("pos", pt.grad, gp), ("base", bt.grad, gb), ("mat", mt.grad, gm)):
            same(words(a), words(b), name + ".grad against the plain call")
        accs, planes = expect_bwd(tmp_path, frames, v, nw, pw, bw, mw, parn, g.cpu().numpy())
        check_planes((words(gn), words(gp), words(gb), words(gm)), planes, "plain call")
        check_gpar(gpar.cpu().numpy(), accs, "plain gpar")
        # the pieces' gradients: slices of the block's (per-frame lights beside shared eye, amb: torch adds the two rows)
        lg = lights.grad.cpu().numpy().reshape(2 if per_frame else 1, 18)
        assert (np.abs(lg - np.stack([a.gsum[6:] for a in accs])) <= np.stack([a.bound()[6:] for a in accs])).all()
        tot, bnd = sum(a.gsum[:6] for a in accs), sum(a.bound(1)[:6] for a in accs)
        got6 = np.concatenate([t.grad.cpu().numpy() for t in (eye, amb)])
        assert (np.abs(got6 - tot) <= bnd).all() and (got6 != 0).all() and (lg != 0).all()
    # base None; nothing needs a gradient: no backward is there to launch; one input does: the call asks for that output alone
    n0 = len(calls)
    out = microfacet(fs, vis, nrm, pos, None, mat, lights.detach(), eye.detach(), amb.detach())
    assert not out.requires_grad and out.grad_fn is None
    same(words(out), fwd(fs, vis, nrm, pos, None, mat, parn), "base None")
    mt = mat.clone().requires_grad_(True)
    microfacet(fs, vis, nrm, pos, None, mt, lights.detach(), eye.detach(), amb.detach()).sum().backward()
    assert len(calls) == n0 + 1 and mt.grad is not None and bool((mt.grad != 0).any())
    # (the launch's output pointers after d_gout: gnrm, gpos, gbase, gmat, gpar, work — gmat alone was asked for)
    assert [bool(p) for p in calls[-1][9:15]] == [False, False, False, True, False, False]
    assert microfacet_grad(fs, vis, nrm, pos, None, mat, block, g, want_gpar=False)[2] is None
    assert microfacet_grad(fs, vis, nrm, pos, None, mat, block, g, want_gpar=False)[4] is None
    with pytest.raises(ValueError):
        microfacet(fs, vis, nrm[:, :2], pos, base, mat, lights.detach(), eye.detach(), amb.detach())
    with pytest.raises(ValueError):
        microfacet(fs, vis, nrm, pos, base, base, lights.detach(), eye.detach(), amb.detach())  # (a three-plane material)
    with pytest.raises(ValueError):
        microfacet(fs, vis, nrm, pos, base, None, lights.detach(), eye.detach(), amb.detach())
    with pytest.raises(ValueError):
        microfacet(fs, vis, nrm, pos, base, mat, dev(np.zeros((9, 6))), eye.detach(), amb.detach())
    with pytest.raises(ValueError):
        microfacet(fs, vis, nrm, pos, base, mat, dev(np.zeros((0, 6))), eye.detach(), amb.detach())
    with pytest.raises(ValueError):
        microfacet_grad(fs, vis, nrm, pos, None, mat, block, g, False, False, True, False, False)  # (gbase without base: nothing left)
    fs.close()


def test_the_chain_from_the_vertices_on_a_sceneset(ctx, tmp_path):
    """nrm = interpolate(corner_attr(mesh_normals(verts))), pos = interpolate(corner_attr(verts)), base = texture(tex, uv), mat =
    texture(mtex, uv) with a two-channel material texture, img = microfacet(...): finite, non-zero gradients reach the vertices, the
    lights and both textures, and microfacet's own share is the plain call's, bit for bit, on the planes the chain produced"""
    from srz import visibility as V
    W = H = 64
    SLOT = 3
    ident = np.eye(4, dtype=np.float32).reshape(16)
    posn, faces = vgkit.grid(16, 16, 3, extra=1)
    mvps = [vgkit.perspective(50.0, 46.0, 5.0, 6.0), vgkit.perspective(38.0, 52.0, 14.0, 3.0, w=1.5, wx=-0.2, wy=0.3, wz=0.25, sz=2.0, oz=4.0)]
    faces = vgkit.oriented(posn, faces, mvps[0])
    v8 = vgkit.verts8(posn)
    sframes, plain = [], []
    for i, m in enumerate(mvps):
        sf, f = scene_pair([(v8, faces, abi.SHADER_NORMAL, -1, m, ident)], W, H, (0.0, 0.0, 1.0), [], 1.75, 0.5, ctx=ctx if i == 0 else None,
                           slots=[SLOT])
        sframes.append(sf), plain.append(f)
    fs = ctx.frameset(sframes)
    T = max(f.n_tris for f in plain)
    vis = visibility(fs)
    v = words(vis)
    assert owners(v, [T, T]).sum() > 500
    rng = np.random.default_rng(19)
    verts = dev(posn).requires_grad_(True)
    tex = dev(rng.uniform(0.1, 1.0, (8, 8, 3))).requires_grad_(True)
    mtex = dev(rng.uniform(0.15, 0.85, (8, 8, 2))).requires_grad_(True)
    uv_attr = dev(rng.uniform(0.05, 0.95, (T, 3, 2)))
    centre = posn.mean(0)
    # one light on either side of the sheet: whichever way the mesh's normals face, one of them lights it; the eye on both sides in turn
    lights = dev([[*(centre + (0.3, 0.2, 1.5)), 9.0, 8.0, 7.0], [*(centre + (-0.4, 0.3, -1.2)), 3.0, 4.0, 5.0]]).requires_grad_(True)
    eye = dev(np.stack([centre + (0.1, -0.1, 2.0), centre + (0.1, -0.1, -2.0)])).requires_grad_(True)
    amb = dev((0.05, 0.06, 0.07)).requires_grad_(True)
    nrm = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: V.mesh_normals(ctx, SLOT, verts)}, pos_tris=T))
    pos = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: verts}, pos_tris=T))
    uv = V.interpolate(fs, vis, uv_attr)
    base, mat = V.texture(fs, vis, tex, uv), V.texture(fs, vis, mtex, uv)
    for t in (nrm, pos, base, mat):
        t.retain_grad()
    img = V.microfacet(fs, vis, nrm, pos, base, mat, lights, eye, amb)
    block = V.microfacet_params(fs, lights.detach(), eye.detach(), amb.detach())
    assert tuple(block.shape) == (2, 18)
    same(words(img.detach()), fwd(fs, vis, nrm.detach(), pos.detach(), base.detach(), mat.detach(), block.cpu().numpy()), "chain forward")
    same(words(img.detach()), expect_fwd(tmp_path, [T, T], v, nrm.detach().cpu().numpy(), pos.detach().cpu().numpy(),
                                         base.detach().cpu().numpy(), mat.detach().cpu().numpy(), block.cpu().numpy()),
         "chain forward against the reference")
    weight = dev(rng.normal(0, 1, tuple(img.shape)))
    (img * weight).sum().backward()
    torch.cuda.synchronize()
    for g in (verts.grad, lights.grad, tex.grad, mtex.grad, eye.grad, amb.grad):
        assert bool(torch.isfinite(g).all())
    for g in (verts.grad, lights.grad, tex.grad, mtex.grad, amb.grad):
        assert int((g != 0).sum()) > g.numel() // 20
    gn, gp, gb, gm, gpar = V.microfacet_grad(fs, vis, nrm.detach(), pos.detach(), base.detach(), mat.detach(), block, weight.contiguous())
    for name, a, b in (("nrm", nrm.grad, gn), ("pos", pos.grad, gp), ("base", base.grad, gb), ("mat", mat.grad, gm)):
        same(words(a), words(b), name + ".grad against the plain call")
    assert np.array_equal(words(eye.grad), words(gpar)[:, 0:3])
    fs.close()


def test_a_fit_of_roughness_and_metallic(ctx):
    """30 Adam steps on a per-pixel roughness and metallic plane against a target the same pass rendered from displaced values bring
    the loss below 10 % of its start.  The same run with the torch float64 rule on the CPU (microfacetref.torch_rule on fit_inputs' very
    planes: roughness and metallic displaced by 0.12 either way, lr 0.02) ends at 1.4 % of its start (lr 0.01: 0.8 %, 0.05: 2.3 %);
    chosen so that it stays under 5 %."""
    from srz.visibility import microfacet
    h, w = 48, 64
    frames = hand_frames(w, h, 1, 20)
    fs = ctx.frameset(frames)
    vis = torch.as_tensor(hand_vis(np.full((1, h, w), 3, np.uint32))).cuda()
    nrm, pos, base, true, start, lights, eye, amb = (dev(t) for t in fit_inputs(h, w))
    target = microfacet(fs, vis, nrm, pos, base, true, lights, eye, amb)
    x = start.clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=FIT_LR)
    losses = []
    for i in range(31):
        opt.zero_grad()
        loss = (microfacet(fs, vis, nrm, pos, base, x, lights, eye, amb) - target).square().mean()
        losses.append(float(loss.detach()))
        if i < 30:
            loss.backward()
            opt.step()
    print(f"loss {losses[0]:.4e} -> {losses[-1]:.4e}: {losses[-1] / losses[0]:.4f}")
    assert losses[0] > 0 and losses[-1] < 0.1 * losses[0]
    fs.close()


FIT_LR = 0.02


def fit_inputs(h, w):
    """(nrm, pos, base [1, 3, h, w], the true material and the displaced start [1, 2, h, w], lights [2, 6], eye, amb [3]) float32: the
    true roughness in (0.3, 0.7) and metallic in (0.2, 0.8), the start 0.12 off either way (inside the clamps)"""
    nrm, pos, base, _, _ = mf.make_planes(77, (h, w))
    rng = np.random.default_rng(78)
    true = rng.uniform([[[0.3]], [[0.2]]], [[[0.7]], [[0.8]]], (2, h, w)).astype(np.float32)
    start = (true + np.float32(0.12) * rng.choice(np.float32([-1, 1]), (2, h, w))).astype(np.float32)
    lights = np.float32([[0.5, -0.3, 4.0, 40.0, 32.0, 24.0], [-0.8, 0.6, 3.0, 20.0, 25.0, 30.0]])
    return nrm[None], pos[None], base[None], true[None], start[None], lights, np.float32([0.2, -0.1, 5.0]), np.float32([0.05, 0.05, 0.05])
