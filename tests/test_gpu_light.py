"""-m gpu: the Blinn-Phong lighting pass over a visibility buffer and its gradients (srz_frameset_light / _light_grad, k_light,
k_light_grad, k_light_fold).  The visibility buffer is the GPU's own render_visibility, except where a test writes one by hand; the
normals are the GPU's own interpolate of the frames' normals, the positions a hand-written linear ramp, except where a test writes
the planes by hand; the expected values are tests/lightref.py's on those very buffers (pinned on the CPU by tests/test_light_ref.py).
Forward, gnrm, gpos, gkd: a NaN on one side must be a NaN on the other, every other word matches bit for bit.  gpar: within
gamma_n * sum |term| of the reference's double sums, gamma_n = n u / (1 - n u), u = 2^-24, n the entry's contributing pixels — the
bound of any summation tree, the terms being the rule's float32 terms on both sides: derived, not measured —, bit-equal between two
launches, and the float32 term itself where one pixel contributes."""
import numpy as np
import pytest
import torch

import lightref
import vgkit
from srz import abi, parallel
from support import SENTINEL, ccw, ctx, filled, frame, scene_pair, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
BACKDROP = ccw((-8, -8), (400, -8), (-8, 400), z=80.0, uv=((0.1, 0.2), (0.9, 0.3), (0.4, 0.95)))
BACKDROP["nrm"] = np.float32([(0.3, -0.3, 0.9), (-0.4, 0.2, 0.8), (0.1, -0.2, 0.95)])
SIZES = [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6), (1, 1, 3)]
LIGHTS, EXPONENTS = (1, 3, 8), (1, 2, 5, 150, 256)


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


def rand_planes(seed, shape, own=None):
    """(kd in (0.1, 1), gout normal) [n, 3, rows, W]; nobody's words NaN: they may hold anything"""
    rng = np.random.default_rng([seed, 8])
    kd, g = rng.uniform(0.1, 1.0, shape).astype(np.float32), rng.normal(0, 2, shape).astype(np.float32)
    if own is not None:
        for t in (kd, g):
            t[np.broadcast_to(~own[:, None], t.shape)] = np.nan
    return kd, g


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


def rand_ids(rng, n, h, w, tris, holes=True):
    ids = rng.integers(1, tris + 1, (n, h, w)).astype(np.uint32)
    ids |= (rng.random((n, h, w)) < 0.4).astype(np.uint32) << 31
    if holes:
        ids[rng.random((n, h, w)) < 0.1] = 0
    return ids


def par_dims(par):
    par = np.ascontiguousarray(par, np.float32)
    return par, (par.shape[-1] - 9) // 6, (par.shape[0] if par.ndim == 2 else 1)


def fwd(fs, vis, nrm, pos, kd, par, p, flags=F, fill=0):
    """the forward pass into a buffer prefilled with the word `fill` → uint32 [n, 3, rows, W]; nrm, pos, kd: device tensors (kd None)"""
    par, L, pf = par_dims(par)
    out, pt = filled(fs.interpolate_shape(3), fill), dev(par)
    fs.light(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), None if kd is None else kd.data_ptr(), pt.data_ptr(), L, pf, p, out.data_ptr(),
             fs.interpolate_bytes(3), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def bwd(fs, vis, nrm, pos, kd, par, p, gout, want=(True, True, True, True), flags=F, fill=0):
    """the backward pass → (gnrm, gpos, gkd uint32 [n, 3, rows, W] from `fill`, gpar float32 of par's shape from SENTINEL words);
    None where not wanted (gkd: and without kd)"""
    par, L, pf = par_dims(par)
    pt, g = dev(par), dev(gout)
    want = list(want)
    want[2] = want[2] and kd is not None
    planes = [filled(fs.interpolate_shape(3), fill) if w else None for w in want[:3]]
    gpar = filled((pf, lightref.par_len(L)), SENTINEL) if want[3] else None
    nbytes = fs.light_work_bytes(L) if want[3] else 0
    work = filled((nbytes // 4,), SENTINEL) if want[3] else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    fs.light_grad(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), ptr(kd), pt.data_ptr(), L, pf, p, g.data_ptr(), *(ptr(t) for t in planes),
                  ptr(gpar), ptr(work), nbytes, flags, stream())
    torch.cuda.synchronize()
    return tuple(None if t is None else words(t) for t in planes) + (None if gpar is None else words(gpar).view(np.float32),)


def par_of(par, i):
    return par[i] if par.ndim == 2 else par


def expect_fwd(tmp_path, frames, v, nw, pw, kw, par, p, fused=True, fill=0):
    """v: the visibility buffer's words [n, 4, rows, W]; nw, pw, kw: the planes float32 [n, 3, rows, W] (kw None)"""
    out = []
    for i, f in enumerate(frames):
        pre = np.full((3,) + v.shape[2:], fill, np.uint32)
        out.append(lightref.forward(tmp_path, n_tris(f), v[i, 1], nw[i], pw[i], None if kw is None else kw[i], par_of(par, i), p, fused, pre))
    return np.stack(out)


def expect_bwd(tmp_path, frames, v, nw, pw, kw, par, p, gout, fused=True, fill=0):
    """(Grad per parameter frame — one for a shared block —, [gnrm, gpos, gkd] each [n, 3, rows, W] float32, gkd None without kd)"""
    par = np.ascontiguousarray(par, np.float32)
    shared = par.ndim == 1
    L = (par.shape[-1] - 9) // 6
    accs = [lightref.Grad(L) for _ in range(1 if shared else len(frames))]
    planes = []
    for i, f in enumerate(frames):
        pre = np.full((3,) + v.shape[2:], fill, np.uint32)
        planes.append(lightref.grad(tmp_path, n_tris(f), v[i, 1], nw[i], pw[i], None if kw is None else kw[i], par_of(par, i), p, gout[i],
                                    accs[0 if shared else i], fused, pre))
    return accs, [None if planes[0][k] is None else np.stack([q[k] for q in planes]) for k in range(3)]


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
    for name, g, w in zip(("gnrm", "gpos", "gkd"), got, want):
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
    """every light count and exponent, kd given and null, shared and per-frame parameters; at the three larger sizes gpar too: within
    its bound, the same words from a second launch, every entry overwritten"""
    frames, fs, vis, v, nrm, nw, own = rendered(ctx, w, h, n)
    pw = ramp(2, h, w)
    pos = dev(pw)
    kw, gout = rand_planes(w, (2, 3, h, w), own)
    kd = dev(kw)
    lit_any = False
    for L in LIGHTS:
        both = lightref.make_params(w + L, L, frames=2)
        for p in EXPONENTS:
            for par in (both, both[0]):
                for k_dev, k_np in ((kd, kw), (None, None)):
                    what = f"{w}x{h} L {L} p {p} par {par.ndim} kd {k_np is not None}"
                    got = fwd(fs, vis, nrm, pos, k_dev, par, p, F, SENTINEL)
                    same(got, expect_fwd(tmp_path, frames, v, nw, pw, k_np, par, p, fill=SENTINEL), what)
                    assert (got[np.broadcast_to(~own[:, None], got.shape)] == 0).all()
                    lit_any |= bool((got != 0).any())
                    want_par = w * h >= 1000
                    res = bwd(fs, vis, nrm, pos, k_dev, par, p, gout, (True, True, True, want_par), fill=SENTINEL)
                    accs, planes = expect_bwd(tmp_path, frames, v, nw, pw, k_np, par, p, gout, fill=SENTINEL)
                    check_planes(res[:3], planes, what)
                    if want_par:
                        assert not (res[3].view(np.uint32) == SENTINEL).any()  # written, every entry
                        check_gpar(res[3], accs, what + " gpar")
                        again = bwd(fs, vis, nrm, pos, k_dev, par, p, gout, (False, False, False, True))[3]
                        assert np.array_equal(again.view(np.uint32), res[3].view(np.uint32)), what + ": two launches differ"
    assert lit_any
    # each want flag alone gives the same words as all together
    par, p = lightref.make_params(5, 3, frames=2), 5
    every = bwd(fs, vis, nrm, pos, kd, par, p, gout, fill=SENTINEL)
    for k in range(4):
        alone = bwd(fs, vis, nrm, pos, kd, par, p, gout, tuple(i == k for i in range(4)), fill=SENTINEL)
        assert all(alone[i] is None for i in range(4) if i != k)
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
    kw, gout = rand_planes(2, (9, 3, 64, 64), owners(v, frames))
    kd = dev(kw)
    per = lightref.make_params(4, 3, frames=9)
    rows = None
    for par in (per, per[0]):
        got = fwd(fs, vis, nrm, pos, kd, par, 5, F, SENTINEL)
        same(got, expect_fwd(tmp_path, frames, v, nw, pw, kw, par, 5, fill=SENTINEL), "nine frames")
        res = bwd(fs, vis, nrm, pos, kd, par, 5, gout, fill=SENTINEL)
        accs, planes = expect_bwd(tmp_path, frames, v, nw, pw, kw, par, 5, gout, fill=SENTINEL)
        check_planes(res[:3], planes, "nine frames")
        check_gpar(res[3], accs, f"nine frames gpar {par.ndim}")
        rows = res[3] if par.ndim == 2 else rows
    assert len({got[i].tobytes() for i in range(9)}) == 9 and len({rows[i].tobytes() for i in range(9)}) == 9
    fs.close()


def test_shared_parameters_are_the_frame_order_sum_of_the_per_frame_rows(ctx, tmp_path):
    """include/srz.h states it, so it is checkable bit for bit: one parameter frame for every frame gives, per entry, 0 + row 0 + row 1 +
    ... in float32 of the rows the call with that frame repeated per frame writes"""
    for k in (2, 9):
        frames, fs, vis, v, nrm, nw, own = rendered(ctx, 64, 64, 90, k=k)
        pos = dev(ramp(k, 64, 64))
        kw, gout = rand_planes(3, (k, 3, 64, 64), own)
        kd = dev(kw)
        one = lightref.make_params(9, 3)
        shared = bwd(fs, vis, nrm, pos, kd, one, 5, gout, (False, False, False, True))[3]
        rows = bwd(fs, vis, nrm, pos, kd, np.repeat(one[None], k, 0), 5, gout, (False, False, False, True))[3]
        s = np.zeros(rows.shape[1], np.float32)
        for i in range(k):
            s = s + rows[i]
        assert shared.shape == (1, rows.shape[1]) and np.array_equal(shared[0].view(np.uint32), s.view(np.uint32)) and (s != 0).all()
        fs.close()


# ------------------------------------------------------------------------------------------------------ hostile planes
def test_hostile_planes_under_a_hand_written_buffer(ctx, tmp_path):
    """planes written by hand (lightref.hostile_planes) under a hand-written visibility buffer with holes: zero, NaN, inf and
    subnormal normals, a light and the eye exactly at P, Ld + Vd = 0, r2 overflowing, cosines exactly 0 and negative, non-finite kd
    and gout: every branch of the rule is met, and every word matches"""
    w, h, n, p = 96, 64, 2, 5
    rng = np.random.default_rng(41)
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    ids = rand_ids(rng, n, h, w, 20)
    v = hand_vis(ids)
    vw = v.view(np.uint32)
    vis = torch.as_tensor(v).cuda()
    par = lightref.hostile_params(2)
    nw, pw, kw, gout, kind = (np.stack(t) for t in zip(*(lightref.hostile_planes(rng, (h, w), par) for _ in range(n))))
    own = owners(vw, frames)
    cls, lcls = (np.stack(t) for t in zip(*(lightref.classify(tmp_path, 20, ids[i], nw[i], pw[i], par, p) for i in range(n))))
    lit = (cls & lightref.LIT) != 0
    reached = (lcls & lightref.REACHED) != 0
    on = reached & ((lcls & lightref.SKIPPED) == 0)
    branches = {"nobody": ~own, "not lit": own & ~lit, "lit": lit, "no view": lit & ((cls & lightref.VIEW) == 0),
                "skipped": reached & ~on, "not skipped": on, "diffuse off": on & ((lcls & lightref.DIFFUSE) == 0),
                "diffuse on": on & ((lcls & lightref.DIFFUSE) != 0), "specular disabled": on & ((lcls & lightref.SPEC_ENABLED) == 0),
                "Ld + Vd = 0": (on & ((lcls & lightref.SPEC_ENABLED) == 0))[:, 0] & ((cls & lightref.VIEW) != 0),
                "specular enabled, off": on & ((lcls & lightref.SPEC_ENABLED) != 0) & ((lcls & lightref.SPEC_ON) == 0),
                "specular on": (lcls & lightref.SPEC_ON) != 0, "cosine exactly 0": own & lit & (kind == 7),
                "r2 overflows": own & lit & (kind == 6), "non-finite kd": own & lit & ~np.isfinite(kw).all(1),
                "non-finite gout": own & lit & ~np.isfinite(gout).all(1)}
    for name, m in branches.items():
        assert int(m.sum()) >= 50, (name, int(m.sum()))
    nrm, pos, kd = dev(nw), dev(pw), dev(kw)
    for k_dev, k_np in ((kd, kw), (None, None)):
        got = fwd(fs, vis, nrm, pos, k_dev, par, p, F, SENTINEL)
        same(got, expect_fwd(tmp_path, frames, vw, nw, pw, k_np, par, p, fill=SENTINEL), "hostile forward")
        assert (got[np.broadcast_to((own & ~lit)[:, None], got.shape)] == 0).all()
        res = bwd(fs, vis, nrm, pos, k_dev, par, p, gout, (True, True, True, False), fill=SENTINEL)
        _, planes = expect_bwd(tmp_path, frames, vw, nw, pw, k_np, par, p, gout, fill=SENTINEL)
        check_planes(res[:3], planes, "hostile")
    assert np.isnan(got.view(np.float32)).any() or np.isnan(res[0].view(np.float32)).any()
    # gpar with kd and gout made finite (a NaN term would make the whole entry a NaN on both sides: nothing to bound), per frame and shared
    # (3e38 is finite and overflows in the first product: it goes too)
    kf, gf = np.where(np.abs(kw) < 1e6, kw, np.float32(0.5)), np.where(np.abs(gout) < 1e6, gout, np.float32(-1.5))
    for bp in (par, np.stack([par, lightref.hostile_params(3)])):
        res = bwd(fs, vis, nrm, pos, dev(kf), bp, p, gf, fill=SENTINEL)
        accs, planes = expect_bwd(tmp_path, frames, vw, nw, pw, kf, bp, p, gf, fill=SENTINEL)
        check_planes(res[:3], planes, "hostile finite")
        check_gpar(res[3], accs, f"hostile gpar {bp.ndim}")
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
        nw, pw, kw, gout = (np.stack([t, t]) for t in lightref.make_planes(7, (h, w)))
        nw[fi, :, y, x] = (0.2, -0.4, 2.0)  # facing the lights and the eye: no term of the pixel is 0 by a branch
        par = lightref.make_params(3, 3)
        par[15:18] = pw[fi, :, y, x]  # light 1 exactly at the pixel: skipped
        res = bwd(fs, torch.as_tensor(v).cuda(), dev(nw), dev(pw), dev(kw), par, 5, gout)
        acc = lightref.Grad(3)
        _, _, _, terms = lightref.grad(tmp_path, 20, ids[fi], nw[fi], pw[fi], kw[fi], par, 5, gout[fi], into=acc, want_terms=True)
        t = terms[:, y, x]
        assert (acc.count[np.r_[0:15, 21:27]] == 1).all() and not acc.count[15:21].any() and (t[np.r_[0:15, 21:27]] != 0).all()
        same(res[3][0] + np.float32(0), t + np.float32(0), f"one pixel {fi} {y} {x}")
        assert not res[3][0][15:21].view(np.uint32).any()
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
    par, p = lightref.hostile_params(4), 2
    nw, pw, kw, gout, _ = (np.stack(t) for t in zip(*(lightref.hostile_planes(rng, (80, 96), par) for _ in range(2))))
    for t in (nw, pw, kw, gout):
        t[np.broadcast_to(~own[:, None], t.shape)] = np.nan  # never read
    nrm, pos, kd = dev(nw), dev(pw), dev(kw)
    fused, kept = fwd(fs, vis, nrm, pos, kd, par, p, F, SENTINEL), fwd(fs, vis, nrm, pos, kd, par, p, 0, SENTINEL)
    same(fused, expect_fwd(tmp_path, frames, vw, nw, pw, kw, par, p, True, SENTINEL), "fused")
    same(kept, expect_fwd(tmp_path, frames, vw, nw, pw, kw, par, p, False, SENTINEL), "not fused")
    assert (fused[0][:, nobody] == 0).all() and (kept[0][:, nobody] == SENTINEL).all() and (kept[0][:, own[0]] != SENTINEL).all()
    for fl, fused_ in ((F, True), (0, False)):
        res = bwd(fs, vis, nrm, pos, kd, par, p, gout, (True, True, True, False), flags=fl, fill=SENTINEL)
        _, planes = expect_bwd(tmp_path, frames, vw, nw, pw, kw, par, p, gout, fused_, SENTINEL)
        check_planes(res[:3], planes, f"fused {fused_}")
        for q in res[:3]:
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
    kw, gout = rand_planes(13, (2, 3, h, w))
    par, p = lightref.make_params(12, 3), 5
    full = fwd(fs, vis, nrm, dev(pw), dev(kw), par, p)
    same(full, expect_fwd(tmp_path, frames, v, nw, pw, kw, par, p), "whole frame")
    whole = bwd(fs, vis, nrm, dev(pw), dev(kw), par, p, gout)
    accs, planes = expect_bwd(tmp_path, frames, v, nw, pw, kw, par, p, gout)
    check_planes(whole[:3], planes, "whole frame")
    check_gpar(whole[3], accs, "whole frame gpar")
    fs.close()
    total = np.zeros(whole[3].shape, np.float64)
    for rank in (0, 1):
        c = srz.Context(0, rank, 2)
        sfs = c.frameset(frames)
        svis = visibility(sfs)
        snrm = interp_normals(sfs, svis, frames)
        rows = parallel.band_rows(h, rank, 2)
        assert len(rows) == 2
        local = [np.zeros(sfs.interpolate_shape(3), np.float32) for _ in range(3)]
        for (lb, _, r0, r1) in rows:
            for dst, src in zip(local, (pw, kw, gout)):
                dst[:, :, lb * 32: lb * 32 + r1 - r0] = src[:, :, r0:r1]
        spos, skd, sg = local
        shard = fwd(sfs, svis, snrm, dev(spos), dev(skd), par, p)
        part = bwd(sfs, svis, snrm, dev(spos), dev(skd), par, p, sg)
        for (lb, _, r0, r1) in rows:
            same(shard[:, :, lb * 32: lb * 32 + r1 - r0], full[:, :, r0:r1], f"rank {rank} band {lb}")
            for k in range(3):
                same(part[k][:, :, lb * 32: lb * 32 + r1 - r0], whole[k][:, :, r0:r1], f"plane {k} rank {rank} band {lb}")
        assert (part[3] != 0).all()
        total += part[3].astype(np.float64)
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
    nrm, pos, kd, g = (torch.ones(shape, dtype=torch.float32, device="cuda") for _ in range(4))
    outs = [filled(shape, SENTINEL) for _ in range(3)]
    L, p = 3, 5
    nbytes = sfs.light_work_bytes(L)
    assert nbytes == 2 * lightref.par_len(L) * 4  # no partials, a row per frame
    for pf in (2, 1):
        par = dev(lightref.make_params(3, L, frames=2)[:pf])
        gpar, work = filled((pf, lightref.par_len(L)), SENTINEL), filled((nbytes // 4,), SENTINEL)
        sfs.light_grad(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), kd.data_ptr(), par.data_ptr(), L, pf, p, g.data_ptr(),
                       *(t.data_ptr() for t in outs), gpar.data_ptr(), work.data_ptr(), nbytes, F, stream())
        torch.cuda.synchronize()
        assert not words(gpar).any(), (pf, words(gpar))
    # the forward and the planes-only backward have nothing to do there, and say so by succeeding
    sfs.light(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), kd.data_ptr(), par.data_ptr(), L, 1, p, outs[0].data_ptr(),
              sfs.interpolate_bytes(3), F, stream())
    sfs.light_grad(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), kd.data_ptr(), par.data_ptr(), L, 1, p, g.data_ptr(), outs[0].data_ptr(), None,
                   None, None, None, 0, F, stream())
    torch.cuda.synchronize()
    assert all((words(t) == SENTINEL).all() for t in outs)
    sfs.close(), c.close()


# ------------------------------------------------------------------------------------------------------ autograd, the chain, a fit
def test_autograd(ctx, tmp_path, monkeypatch):
    import srz
    from srz.visibility import light, light_grad, light_params
    frames, fs, vis, v, nrm, nw, own = rendered(ctx, 100, 70, 120)
    pw = ramp(2, 70, 100)
    kw, _ = rand_planes(6, (2, 3, 70, 100))
    pos, kd = dev(pw), dev(kw)
    calls = []
    real = srz.FrameSet.light_grad
    monkeypatch.setattr(srz.FrameSet, "light_grad", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    p = 5
    for per_frame in (False, True):
        parn = lightref.make_params(16, 3, frames=2)
        parn[1, :9] = parn[0, :9]  # eye, ka, ks shared; the lights per frame or shared
        parn = parn if per_frame else parn[0]
        row = parn[0] if per_frame else parn
        lights = dev(parn[..., 9:].reshape((2, 3, 6) if per_frame else (3, 6))).requires_grad_(True)
        eye, ka, ks = (dev(row[i:i + 3]).requires_grad_(True) for i in (0, 3, 6))
        nt, pt, kt = (t.clone().requires_grad_(True) for t in (nrm, pos, kd))
        n0 = len(calls)
        out = light(fs, vis, nt, pt, kt, lights, eye, ka, ks, p)
        assert out.shape == (2, 3, 70, 100) and out.requires_grad
        same(words(out.detach()), fwd(fs, vis, nrm, pos, kd, parn, p), "forward")
        out.square().sum().backward()
        torch.cuda.synchronize()
        assert len(calls) == n0 + 1  # one launch for every gradient
        g = (2 * out.detach()).contiguous()
        block = light_params(fs, lights.detach(), eye.detach(), ka.detach(), ks.detach())
        assert tuple(block.shape) == ((2, 27) if per_frame else (1, 27))
        gn, gp, gk, gpar = light_grad(fs, vis, nrm, pos, kd, block, p, g)
        for name, a, b in (("nrm", nt.grad, gn), ("pos", pt.grad, gp), ("kd", kt.grad, gk)):
            same(words(a), words(b), name + ".grad against the plain call")
        accs, planes = expect_bwd(tmp_path, frames, v, nw, pw, kw, parn, p, g.cpu().numpy())
        check_planes((words(gn), words(gp), words(gk)), planes, "plain call")
        check_gpar(gpar.cpu().numpy(), accs, "plain gpar")
        # the pieces' gradients: slices of the block's (per-frame lights beside shared eye, ka, ks: torch adds the two rows)
        lg = lights.grad.cpu().numpy().reshape(2 if per_frame else 1, 18)
        assert (np.abs(lg - np.stack([a.gsum[9:] for a in accs])) <= np.stack([a.bound()[9:] for a in accs])).all()
        tot, bnd = sum(a.gsum[:9] for a in accs), sum(a.bound(1)[:9] for a in accs)
        got9 = np.concatenate([t.grad.cpu().numpy() for t in (eye, ka, ks)])
        assert (np.abs(got9 - tot) <= bnd).all() and (got9 != 0).all() and (lg != 0).all()
    # kd None; nothing needs a gradient: no backward is there to launch; one input does: the call asks for that output alone
    n0 = len(calls)
    out = light(fs, vis, nrm, pos, None, lights.detach(), eye.detach(), ka.detach(), ks.detach(), p)
    assert not out.requires_grad and out.grad_fn is None
    same(words(out), fwd(fs, vis, nrm, pos, None, parn, p), "kd None")
    lt = lights.detach().clone().requires_grad_(True)
    light(fs, vis, nrm, pos, None, lt, eye.detach(), ka.detach(), ks.detach(), p).sum().backward()
    assert len(calls) == n0 + 1 and lt.grad is not None and bool((lt.grad != 0).all())
    assert light_grad(fs, vis, nrm, pos, None, block, p, g, want_gpar=False)[2:] == (None, None)
    for bad in (dict(p=0), dict(p=257), dict(p=2.5)):
        with pytest.raises(ValueError):
            light(fs, vis, nrm, pos, kd, lights.detach(), eye.detach(), ka.detach(), ks.detach(), bad["p"])
    with pytest.raises(ValueError):
        light(fs, vis, nrm[:, :2], pos, kd, lights.detach(), eye.detach(), ka.detach(), ks.detach(), p)
    with pytest.raises(ValueError):
        light(fs, vis, nrm, pos, kd, dev(np.zeros((9, 6))), eye.detach(), ka.detach(), ks.detach(), p)
    fs.close()


def test_the_chain_from_the_vertices_on_a_sceneset(ctx, tmp_path):
    """nrm = interpolate(corner_attr(mesh_normals(verts))), pos = interpolate(corner_attr(verts)), kd = texture(tex, interpolate(uv)),
    img = light(...): finite, non-zero gradients reach the vertices (through the normals and the positions), the lights and the
    texture, and light's own share is the plain call's, bit for bit, on the planes the chain produced"""
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
    uv_attr = dev(rng.uniform(0.05, 0.95, (T, 3, 2)))
    centre = posn.mean(0)
    # one light on either side of the sheet: whichever way the mesh's normals face, one of them lights it
    lights = dev([[*(centre + (0.3, 0.2, 1.5)), 9.0, 8.0, 7.0], [*(centre + (-0.4, 0.3, -1.2)), 3.0, 4.0, 5.0]]).requires_grad_(True)
    eye, ka, ks = (dev(t).requires_grad_(True) for t in (centre + (0.1, -0.1, 2.0), (0.05, 0.06, 0.07), (0.5, 0.4, 0.3)))
    nrm = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: V.mesh_normals(ctx, SLOT, verts)}, pos_tris=T))
    pos = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: verts}, pos_tris=T))
    kd = V.texture(fs, vis, tex, V.interpolate(fs, vis, uv_attr))
    for t in (nrm, pos, kd):
        t.retain_grad()
    img = V.light(fs, vis, nrm, pos, kd, lights, eye, ka, ks, 7)
    block = V.light_params(fs, lights.detach(), eye.detach(), ka.detach(), ks.detach())
    same(words(img.detach()), fwd(fs, vis, nrm.detach(), pos.detach(), kd.detach(), block.cpu().numpy()[0], 7), "chain forward")
    same(words(img.detach()), expect_fwd(tmp_path, [T, T], v, nrm.detach().cpu().numpy(), pos.detach().cpu().numpy(),
                                         kd.detach().cpu().numpy(), block.cpu().numpy()[0], 7), "chain forward against the reference")
    weight = dev(rng.normal(0, 1, tuple(img.shape)))
    (img * weight).sum().backward()
    torch.cuda.synchronize()
    for g in (verts.grad, lights.grad, tex.grad, eye.grad, ka.grad, ks.grad):
        assert bool(torch.isfinite(g).all())
    for g in (verts.grad, lights.grad, tex.grad, ka.grad):
        assert int((g != 0).sum()) > g.numel() // 20
    gn, gp, gk, gpar = V.light_grad(fs, vis, nrm.detach(), pos.detach(), kd.detach(), block, 7, weight.contiguous())
    for name, a, b in (("nrm", nrm.grad, gn), ("pos", pos.grad, gp), ("kd", kd.grad, gk)):
        same(words(a), words(b), name + ".grad against the plain call")
    assert np.array_equal(words(lights.grad).reshape(-1), words(gpar)[0, 9:])
    # the vertices hear from both paths: the chain with the positions detached gives another, non-zero gradient
    verts2 = dev(posn).requires_grad_(True)
    nrm2 = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: V.mesh_normals(ctx, SLOT, verts2)}, pos_tris=T))
    (V.light(fs, vis, nrm2, pos.detach(), kd.detach(), lights.detach(), eye.detach(), ka.detach(), ks.detach(), 7) * weight).sum().backward()
    assert bool((verts2.grad != 0).any()) and not torch.equal(verts2.grad, verts.grad)
    fs.close()


def test_a_fit_of_one_light(ctx):
    """30 Adam steps on one light's position and intensity against a target the same pass rendered from displaced values bring the
    loss below 10 % of its start.  The same run with the torch float64 rule on the CPU (lightref.torch_rule, the same seeded planes,
    displacement (0.5, -0.4, 0) and x 1.1, lr 0.05) ends at 3.5 % of its start; chosen so that it stays under 5 %."""
    from srz.visibility import light
    h, w = 48, 64
    frames = hand_frames(w, h, 1, 20)
    fs = ctx.frameset(frames)
    vis = torch.as_tensor(hand_vis(np.full((1, h, w), 3, np.uint32))).cuda()
    nrm, pos, kd = (dev(t[None]) for t in lightref.make_planes(77, (h, w))[:3])
    eye, ka, ks = dev([0.2, -0.1, 5.0]), dev([0.05, 0.05, 0.05]), dev([0.6, 0.6, 0.6])
    true = dev([[0.5, -0.3, 4.0, 10.0, 8.0, 6.0]])
    target = light(fs, vis, nrm, pos, kd, true, eye, ka, ks, 5)
    x = (true + dev([[0.5, -0.4, 0.0, 0.0, 0.0, 0.0]])) * dev([[1, 1, 1, 1.1, 1.1, 1.1]])
    x = x.clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=0.05)
    losses = []
    for i in range(31):
        opt.zero_grad()
        loss = (light(fs, vis, nrm, pos, kd, x, eye, ka, ks, 5) - target).square().mean()
        losses.append(float(loss.detach()))
        if i < 30:
            loss.backward()
            opt.step()
    print(f"loss {losses[0]:.4e} -> {losses[-1]:.4e}: {losses[-1] / losses[0]:.4f}")
    assert losses[0] > 0 and losses[-1] < 0.1 * losses[0]
    fs.close()
