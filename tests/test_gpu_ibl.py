"""-m gpu: the image-based-lighting passes over a visibility buffer and their gradients (srz_frameset_reflect / _reflect_grad,
srz_brdf_table, srz_frameset_ibl / _ibl_grad; k_reflect, k_reflect_grad, k_brdf_table, k_ibl, k_ibl_grad).  The visibility buffers
and the planes are written by hand; the expected values are tests/iblref.py's on those very buffers (pinned on the CPU by
tests/test_ibl_ref.py).  Every plane and the table: a NaN on one side must be a NaN on the other, every other word matches bit for
bit.  d_gtab: within gamma_n * sum |term| of the reference's double sums, gamma_n = n u / (1 - n u), u = 2^-24, n the word's
contributing pixels + 1 — the bound of any summation tree, srz_frameset_texture_grad's own: derived, not measured —, and the float32
term itself where one pixel contributes."""
import types

import numpy as np
import pytest
import torch

import iblref as ib
import srz
from srz import abi, parallel
from support import SENTINEL, ctx, filled, frame, soup, stream, words  # noqa: F401

pytestmark = pytest.mark.gpu

F, E = abi.FUSED_CLEAR, abi.SRZ_E_INVALID
ZS = np.float32([1, 2, 3, 4])
TRIS = 20
SIZES = [(64, 64, 1, False), (96, 40, 3, True)]  # w, h, frames, holes
TABLES = (2, 3, 17, 64)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def hand_set(ctx, w, h, n, flags=0):
    """a set of n frames of TRIS triangles whose frames do not ask for the fused clear themselves: the call's flags decide"""
    return ctx.frameset([frame(soup(1, TRIS, w, h, ZS), w, h, flags=flags) for _ in range(n)])


def hand_vis(ids):
    v = np.zeros((ids.shape[0], 4) + ids.shape[1:], np.float32)
    v[:, 1] = ids.view(np.float32)
    return torch.as_tensor(v).cuda()


def owners(ids):
    return ((ids & 0x7fffffff) - np.uint32(1)) < TRIS


def eye_of(eye, i):
    return eye[i] if eye.ndim == 2 else eye


# ------------------------------------------------------------------------------------------------ the calls and what they should give
def g_reflect(fs, vis, nrm, pos, eye, flags=F):
    e = dev(eye).reshape(-1, 3)
    out = filled(fs.interpolate_shape(4), SENTINEL)
    fs.reflect(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), e.data_ptr(), e.shape[0], out.data_ptr(), fs.interpolate_bytes(4), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def g_reflect_grad(fs, vis, nrm, pos, eye, gout, want=(True, True), flags=F):
    e, g = dev(eye).reshape(-1, 3), dev(gout)
    outs = [filled(fs.interpolate_shape(3), SENTINEL) if w else None for w in want]
    fs.reflect_grad(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), e.data_ptr(), e.shape[0], g.data_ptr(), ptr(outs[0]), ptr(outs[1]), flags, stream())
    torch.cuda.synchronize()
    return tuple(None if t is None else words(t) for t in outs)


def x_reflect(tmp, ids, nw, pw, eye, fused=True):
    pre = np.full((4,) + ids.shape[1:], SENTINEL, np.uint32)
    return np.stack([ib.reflect(tmp, TRIS, ids[i], nw[i], pw[i], eye_of(eye, i), fused, pre) for i in range(len(ids))])


def x_reflect_grad(tmp, ids, nw, pw, eye, gout, fused=True):
    pre = np.full((3,) + ids.shape[1:], SENTINEL, np.uint32)
    res = [ib.reflect_grad(tmp, TRIS, ids[i], nw[i], pw[i], eye_of(eye, i), gout[i], fused, pre) for i in range(len(ids))]
    return tuple(np.stack([r[k] for r in res]) for k in range(2))


IBL_OUTS = ("gbase", "gmat", "gnv", "girr", "gspec", "gtab")
IBL_PLANES = (3, 2, 1, 3, 3)


def g_ibl(fs, vis, base, mat, nv, irr, spec, tab, flags=F):
    out = filled(fs.interpolate_shape(3), SENTINEL)
    fs.ibl(vis.data_ptr(), ptr(base), mat.data_ptr(), nv.data_ptr(), irr.data_ptr(), spec.data_ptr(), tab.data_ptr(), tab.shape[0], out.data_ptr(),
           fs.interpolate_bytes(3), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def g_ibl_grad(fs, vis, base, mat, nv, irr, spec, tab, gout, want=(True,) * 6, flags=F, gtab0=None):
    """→ (gbase, gmat, gnv, girr, gspec as uint32 words from SENTINEL, gtab float32 added into gtab0 (zeros)); None where not wanted"""
    want = list(want)
    want[0] = want[0] and base is not None
    g = dev(gout)
    outs = [filled(fs.interpolate_shape(k), SENTINEL) if w else None for k, w in zip(IBL_PLANES, want)]
    gtab = (torch.zeros_like(tab) if gtab0 is None else dev(gtab0)) if want[5] else None
    fs.ibl_grad(vis.data_ptr(), ptr(base), mat.data_ptr(), nv.data_ptr(), irr.data_ptr(), spec.data_ptr(), tab.data_ptr(), tab.shape[0], g.data_ptr(),
                *(ptr(t) for t in outs), ptr(gtab), flags, stream())
    torch.cuda.synchronize()
    return tuple(None if t is None else words(t) for t in outs) + (None if gtab is None else gtab.cpu().numpy(),)


def x_ibl(tmp, ids, bw, mw, vw, iw, sw, tab, fused=True):
    pre = np.full((3,) + ids.shape[1:], SENTINEL, np.uint32)
    return np.stack([ib.ibl(tmp, TRIS, ids[i], None if bw is None else bw[i], mw[i], vw[i], iw[i], sw[i], tab, fused, pre) for i in range(len(ids))])


def x_ibl_grad(tmp, ids, bw, mw, vw, iw, sw, tab, gout, fused=True):
    """(the five planes stacked over the frames — gbase None without base —, the TabGrad of all frames)"""
    pre = np.full((3,) + ids.shape[1:], SENTINEL, np.uint32)
    acc = ib.TabGrad(tab.shape[0])
    res = [ib.ibl_grad(tmp, TRIS, ids[i], None if bw is None else bw[i], mw[i], vw[i], iw[i], sw[i], tab, gout[i], acc, fused, pre)
           for i in range(len(ids))]
    return tuple(None if res[0][k] is None else np.stack([r[k] for r in res]) for k in range(5)), acc


def check_gtab(got, acc, what, extra=1, start=None):
    ref = acc.gsum if start is None else acc.gsum + np.float64(start)
    bound = acc.bound(extra) if start is None else acc.bound(extra) + np.abs(ref) * 2.0 ** -24
    assert np.isfinite(ref).all(), what
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    print(f"{what}: max err {err.max():.3e}, max err / bound {ratio:.3f}, max n {int(acc.count.max())}, untouched {int((acc.count == 0).sum())}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} words beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    if start is None:
        assert (got[acc.count == 0] == 0).all()


def reflect_inputs(seed, n, h, w, holes, per_frame_eye):
    rng = np.random.default_rng([seed, n, h, w])
    ids = ib.rand_ids(rng, n, h, w, TRIS, holes)
    nw, pw, gout = (np.stack(t) for t in zip(*(ib.reflect_planes(seed + i, (h, w)) for i in range(n))))
    for t in (nw, pw, gout):
        t[np.broadcast_to(~owners(ids)[:, None], t.shape)] = np.nan  # nobody's words never reach a result
    return ids, nw, pw, gout, ib.make_eye(seed, n if per_frame_eye else None)


def ibl_inputs(seed, n, h, w, holes, t):
    rng = np.random.default_rng([seed, n, h, w, t])
    ids = ib.rand_ids(rng, n, h, w, TRIS, holes)
    planes = [np.stack(a) for a in zip(*(ib.ibl_planes(seed + i, (h, w), t) for i in range(n)))]
    for a in planes:
        a[np.broadcast_to(~owners(ids)[:, None], a.shape)] = np.nan
    return (ids, ib.smooth_table(t)) + tuple(planes)  # ids, tab, base, mat, nv, irr, spec, gout


# ------------------------------------------------------------------------------------------------ reflect
@pytest.mark.parametrize("w,h,n,holes", SIZES)
def test_reflect_and_its_gradients(ctx, tmp_path, w, h, n, holes):
    """shared and per-frame eye, with and without the fused clear, either output alone"""
    fs = hand_set(ctx, w, h, n)
    for per_frame in (False, True):
        ids, nw, pw, gout, eye = reflect_inputs(7, n, h, w, holes, per_frame)
        own, vis, nrm, pos = owners(ids), hand_vis(ids), dev(nw), dev(pw)
        for flags, fused in ((F, True), (0, False)):
            what = f"{w}x{h}x{n} eye {eye.ndim} fused {fused}"
            got = g_reflect(fs, vis, nrm, pos, eye, flags)
            same(got, x_reflect(tmp_path, ids, nw, pw, eye, fused), what)
            nobody = np.broadcast_to(~own[:, None], got.shape)
            assert (got[nobody] == (0 if fused else SENTINEL)).all() and (got[~nobody] != SENTINEL).all() and (got[~nobody] != 0).any()
            want = x_reflect_grad(tmp_path, ids, nw, pw, eye, gout, fused)
            both = g_reflect_grad(fs, vis, nrm, pos, eye, gout, (True, True), flags)
            for k, name in enumerate(("gnrm", "gpos")):
                same(both[k], want[k], f"{what} {name}")
                alone = g_reflect_grad(fs, vis, nrm, pos, eye, gout, tuple(i == k for i in range(2)), flags)
                assert alone[1 - k] is None and np.array_equal(alone[k], both[k]), (what, name)
    fs.close()


def test_nine_frames_wrap_the_frame_deal(ctx, tmp_path):
    """eight frames and more take the walk's other branch; per-frame eyes: every frame reads its own"""
    fs = hand_set(ctx, 64, 64, 9)
    ids, nw, pw, gout, eye = reflect_inputs(5, 9, 64, 64, True, True)
    vis, nrm, pos = hand_vis(ids), dev(nw), dev(pw)
    got = g_reflect(fs, vis, nrm, pos, eye)
    same(got, x_reflect(tmp_path, ids, nw, pw, eye), "nine frames")
    res = g_reflect_grad(fs, vis, nrm, pos, eye, gout)
    for a, b in zip(res, x_reflect_grad(tmp_path, ids, nw, pw, eye, gout)):
        same(a, b, "nine frames grad")
    # ibl over the same walk; its table build strides several tiles per workgroup whatever the frame count
    ids, tab, bw, mw, vw, iw, sw, gout = ibl_inputs(6, 9, 64, 64, True, 8)
    vis = hand_vis(ids)
    args = [dev(a) for a in (bw, mw, vw, iw, sw, tab)]
    same(g_ibl(fs, vis, *args), x_ibl(tmp_path, ids, bw, mw, vw, iw, sw, tab), "nine frames ibl")
    res = g_ibl_grad(fs, vis, *args, gout)
    planes, acc = x_ibl_grad(tmp_path, ids, bw, mw, vw, iw, sw, tab, gout)
    for name, a, b in zip(IBL_OUTS, res[:5], planes):
        same(a, b, "nine frames ibl " + name)
    check_gtab(res[5], acc, "nine frames gtab")
    fs.close()


def test_reflect_hostile_planes(ctx, tmp_path):
    """iblref.hostile_reflect: every branch of the rule is met by at least 50 pixels, and every word matches"""
    case = ib.hostile_reflect(**ib.HOSTILE)
    for name, m in ib.reflect_branches(tmp_path, ib.HOSTILE["tris"], *case).items():
        assert int(m.sum()) >= 50, (name, int(m.sum()))
    ids, eye, nw, pw, gout, _ = case
    assert ib.HOSTILE["tris"] == TRIS
    fs = hand_set(ctx, ib.HOSTILE["w"], ib.HOSTILE["h"], ib.HOSTILE["n"])
    vis, nrm, pos = hand_vis(ids), dev(nw), dev(pw)
    got = g_reflect(fs, vis, nrm, pos, eye)
    same(got, x_reflect(tmp_path, ids, nw, pw, eye), "hostile reflect")
    res = g_reflect_grad(fs, vis, nrm, pos, eye, gout)
    for a, b, name in zip(res, x_reflect_grad(tmp_path, ids, nw, pw, eye, gout), ("gnrm", "gpos")):
        same(a, b, "hostile reflect " + name)
    # (a non-finite normal or position leaves the pixel unlit or without a view: the forward holds no NaN; a non-finite gout does reach
    # the gradients)
    assert np.isfinite(got.view(np.float32)).all() and np.isnan(res[0].view(np.float32)).any() and np.isnan(res[1].view(np.float32)).any()
    fs.close()


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("n,m", [(n, m) for n in (2, 3, 8) for m in (1, 4, 16, 64)] + [(64, 8)])
def test_brdf_table_is_the_reference_bit_for_bit(ctx, tmp_path, n, m):
    tab = filled((n, n, 2), SENTINEL)
    guard = filled((16,), SENTINEL)
    ctx.brdf_table(tab.data_ptr(), n * n * 8, n, m, stream())
    torch.cuda.synchronize()
    got = words(tab)
    same(got, ib.table(tmp_path, n, m), f"table {n} {m}")
    assert (got != SENTINEL).all() and (words(guard) == SENTINEL).all() and np.isfinite(got.view(np.float32)).all()
    again = filled((n, n, 2), 0)
    ctx.brdf_table(again.data_ptr(), n * n * 8, n, m, stream())
    torch.cuda.synchronize()
    assert np.array_equal(words(again), got)


def test_brdf_table_wrapper(ctx, tmp_path):
    from srz.visibility import brdf_table
    tab = brdf_table(ctx, 8)
    same(words(tab), ib.table(tmp_path, 8, 64), "brdf_table(ctx, 8)")
    t = tab.cpu().numpy()
    assert abs(t[7, 0, 0] - 1) < 5e-3 and abs(t[7, 0, 1]) < 5e-3 and (t >= 0).all() and (t.sum(-1) < 1.01).all()


# ------------------------------------------------------------------------------------------------ ibl
@pytest.mark.parametrize("w,h,n,holes", SIZES)
def test_ibl_and_its_gradients(ctx, tmp_path, w, h, n, holes):
    """tables of 2, 3, 17 and 64, base given and null, with and without the fused clear; d_gtab within its bound"""
    fs = hand_set(ctx, w, h, n)
    for t in TABLES:
        ids, tab, bw, mw, vw, iw, sw, gout = ibl_inputs(3, n, h, w, holes, t)
        own, vis = owners(ids), hand_vis(ids)
        base, mat, nv, irr, spec, tt = (dev(a) for a in (bw, mw, vw, iw, sw, tab))
        for b_dev, b_np in ((base, bw), (None, None)):
            for flags, fused in ((F, True), (0, False)):
                what = f"{w}x{h}x{n} table {t} base {b_np is not None} fused {fused}"
                got = g_ibl(fs, vis, b_dev, mat, nv, irr, spec, tt, flags)
                same(got, x_ibl(tmp_path, ids, b_np, mw, vw, iw, sw, tab, fused), what)
                nobody = np.broadcast_to(~own[:, None], got.shape)
                assert (got[nobody] == (0 if fused else SENTINEL)).all() and (got[~nobody] != SENTINEL).all()
                res = g_ibl_grad(fs, vis, b_dev, mat, nv, irr, spec, tt, gout, flags=flags)
                planes, acc = x_ibl_grad(tmp_path, ids, b_np, mw, vw, iw, sw, tab, gout, fused)
                for name, a, b in zip(IBL_OUTS, res[:5], planes):
                    assert (a is None) == (b is None), (what, name)
                    if a is not None:
                        same(a, b, f"{what} {name}")
                check_gtab(res[5], acc, what + " gtab")
    fs.close()


def test_ibl_every_output_alone(ctx, tmp_path):
    """each output pointer alone gives the words all together give; gtab alone, and added into what the caller's table holds"""
    w, h, n, t = 96, 40, 3, 17
    fs = hand_set(ctx, w, h, n)
    ids, tab, bw, mw, vw, iw, sw, gout = ibl_inputs(9, n, h, w, True, t)
    vis = hand_vis(ids)
    args = [dev(a) for a in (bw, mw, vw, iw, sw, tab)]
    every = g_ibl_grad(fs, vis, *args, gout)
    _, acc = x_ibl_grad(tmp_path, ids, bw, mw, vw, iw, sw, tab, gout)
    for k in range(6):
        alone = g_ibl_grad(fs, vis, *args, gout, tuple(i == k for i in range(6)))
        assert all(alone[i] is None for i in range(6) if i != k)
        if k < 5:
            assert np.array_equal(alone[k], every[k]), IBL_OUTS[k]
        else:
            check_gtab(alone[5], acc, "gtab alone")
    start = np.random.default_rng(4).normal(0, 3, (t, t, 2)).astype(np.float32)
    added = g_ibl_grad(fs, vis, *args, gout, (False,) * 5 + (True,), gtab0=start)[5]
    check_gtab(added, acc, "gtab added into", start=start)
    fs.close()


def test_gtab_of_one_pixel_is_its_float32_term(ctx, tmp_path):
    """exactly one owned pixel in the set: every other add adds nothing, so each of its eight words is the pixel's float32 term, bit
    for bit (+ 0.0f on both sides: a term of -0 comes out +0), and every other word stays +0"""
    w, h, t = 70, 40, 8
    fs = hand_set(ctx, w, h, 2)
    for (fi, y, x) in ((0, 0, 0), (1, 37, 69), (0, 33, 31)):
        ids = np.zeros((2, h, w), np.uint32)
        ids[fi, y, x] = 5
        _, tab, bw, mw, vw, iw, sw, gout = ibl_inputs(11 + y, 2, h, w, False, t)
        mw[fi, :, y, x], vw[fi, 0, y, x] = (0.43, 0.3), 0.61
        for a in (bw, iw, sw, gout):
            a[fi, :, y, x] = np.abs(np.nan_to_num(a[fi, :, y, x], nan=0.5)) + 0.25
        got = g_ibl_grad(fs, hand_vis(ids), *(dev(a) for a in (bw, mw, vw, iw, sw, tab)), gout, (False,) * 5 + (True,))[5]
        terms, cell = ib.ibl_grad(tmp_path, TRIS, ids[fi], bw[fi], mw[fi], vw[fi], iw[fi], sw[fi], tab, gout[fi], want_terms=True)[5:7]
        x0, y0 = cell[:, y, x]
        want = np.zeros((t, t, 2), np.float32)
        for q, (dx, dy) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            want[x0 + dx, y0 + dy] = terms[q, y, x], terms[4 + q, y, x]
        assert (x0, y0) == (4, 2) and (want[x0:x0 + 2, y0:y0 + 2] != 0).all()
        same(got + np.float32(0), want + np.float32(0), f"one pixel {fi} {y} {x}")
    fs.close()


def test_ibl_hostile_planes(ctx, tmp_path):
    """iblref.hostile_ibl: NaN, inf, subnormal and 3e38 words in every plane and in the table, nv and roughness on and beyond every clamp
    edge and on cell boundaries; every branch is met by at least 50 pixels, every word matches, and nothing is read outside the table
    (a guard of NaN-free sentinel words around it would not show a read: the words matching the reference's do)"""
    case = ib.hostile_ibl(**ib.HOSTILE)
    for name, m in ib.ibl_branches(tmp_path, ib.HOSTILE["tris"], *case).items():
        assert int(m.sum()) >= 50, (name, int(m.sum()))
    ids, tab, bw, mw, vw, iw, sw, gout, _ = case
    fs = hand_set(ctx, ib.HOSTILE["w"], ib.HOSTILE["h"], ib.HOSTILE["n"])
    vis = hand_vis(ids)
    base, mat, nv, irr, spec, tt = (dev(a) for a in (bw, mw, vw, iw, sw, tab))
    for b_dev, b_np in ((base, bw), (None, None)):
        got = g_ibl(fs, vis, b_dev, mat, nv, irr, spec, tt)
        same(got, x_ibl(tmp_path, ids, b_np, mw, vw, iw, sw, tab), "hostile ibl")
        res = g_ibl_grad(fs, vis, b_dev, mat, nv, irr, spec, tt, gout, (True,) * 5 + (False,))
        planes, _ = x_ibl_grad(tmp_path, ids, b_np, mw, vw, iw, sw, tab, gout)
        for name, a, b in zip(IBL_OUTS, res[:5], planes):
            if b is not None:
                same(a, b, "hostile ibl " + name)
    assert np.isnan(got.view(np.float32)).any() and np.isnan(res[1].view(np.float32)).any()
    # gtab with the colour planes, gout and the table made finite (a NaN term would make the whole word a NaN on both sides: nothing to
    # bound); the coordinates stay hostile: their clamps make them finite
    fin = lambda a, v: np.where(np.abs(a) < 1e6, a, np.float32(v)).astype(np.float32)  # noqa: E731
    bf, jf, sf, gf, tf = fin(bw, 0.5), fin(iw, 0.25), fin(sw, 0.75), fin(gout, -1.5), fin(tab, 0.3)
    res = g_ibl_grad(fs, vis, dev(bf), mat, nv, dev(jf), dev(sf), dev(tf), gf)
    planes, acc = x_ibl_grad(tmp_path, ids, bf, mw, vw, jf, sf, tf, gf)
    for name, a, b in zip(IBL_OUTS, res[:5], planes):
        same(a, b, "hostile finite " + name)
    check_gtab(res[5], acc, "hostile gtab")
    fs.close()


def test_sharded_world_2(ctx, tmp_path):
    """each rank's bands of reflect, ibl and their gradient planes are the whole frame's words; the ranks' tables add up"""
    w, h, n, t = 64, 128, 2, 8
    ids, tab, bw, mw, vw, iw, sw, gout = ibl_inputs(14, n, h, w, True, t)
    nw, pw, gr = (np.stack(a) for a in zip(*(ib.reflect_planes(13 + i, (h, w)) for i in range(n))))
    eye = ib.make_eye(13, n)
    frames = [frame(soup(1, TRIS, w, h, ZS), w, h, flags=0) for _ in range(n)]
    v = np.zeros((n, 4, h, w), np.float32)
    v[:, 1] = ids.view(np.float32)
    full = (x_reflect(tmp_path, ids, nw, pw, eye),) + x_reflect_grad(tmp_path, ids, nw, pw, eye, gr)
    planes, acc = x_ibl_grad(tmp_path, ids, bw, mw, vw, iw, sw, tab, gout)
    full_ibl = (x_ibl(tmp_path, ids, bw, mw, vw, iw, sw, tab),) + planes
    total = np.zeros((t, t, 2), np.float64)
    for rank in (0, 1):
        c = srz.Context(0, rank, 2)
        sfs = c.frameset(frames)
        rows = parallel.band_rows(h, rank, 2)
        assert len(rows) == 2

        def local(a):
            out = np.zeros((a.shape[0], a.shape[1], sfs.interpolate_shape(1)[2], w), np.float32)
            for (lb, _, r0, r1) in rows:
                out[:, :, lb * 32: lb * 32 + r1 - r0] = a[:, :, r0:r1]
            return out
        vis = torch.as_tensor(local(v)).cuda()
        shard = (g_reflect(sfs, vis, dev(local(nw)), dev(local(pw)), eye),) + g_reflect_grad(sfs, vis, dev(local(nw)), dev(local(pw)), eye, local(gr))
        args = [dev(local(a)) for a in (bw, mw, vw, iw, sw)] + [dev(tab)]
        res = g_ibl_grad(sfs, vis, *args, local(gout))
        shard_ibl = (g_ibl(sfs, vis, *args),) + res[:5]
        for (lb, _, r0, r1) in rows:
            for k, (a, b) in enumerate(zip(shard + shard_ibl, full + full_ibl)):
                same(a[:, :, lb * 32: lb * 32 + r1 - r0], b[:, :, r0:r1], f"rank {rank} band {lb} output {k}")
        total += res[5].astype(np.float64)
        sfs.close(), c.close()
    err = np.abs(total - acc.gsum)
    assert (err <= acc.bound(2)).all(), float((err - acc.bound(2)).max())


# ------------------------------------------------------------------------------------------------ refusals
W, H, N, T = 64, 64, 2, 8
P4, P3, P2, P1 = (N * k * H * W * 4 for k in (4, 3, 2, 1))
TAB = T * T * 2 * 4
ONLY_FUSED = "only SRZ_FUSED_CLEAR is accepted in flags"
PAR_FRAMES = "par_frames must be 1 or the set's frame count"
TAB_N = "n must be 2 .. SRZ_BRDF_TABLE_MAX"
OUT_IN, OUT_OUT = "an output overlaps an input", "two outputs overlap"
ENTRIES = {
    "frameset_reflect": dict(vis=("vis", 0), nrm=("a", 0), pos=("b", 0), eye=("eye", 0), par_frames=1, out=("o1", 0), out_bytes=P4, flags=F),
    "frameset_reflect_grad": dict(vis=("vis", 0), nrm=("a", 0), pos=("b", 0), eye=("eye", 0), par_frames=1, gout=("g", 0), gnrm=("o1", 0),
                                  gpos=("o2", 0), flags=F),
    "brdf_table": dict(tab=("o1", 0), tab_bytes=TAB, n=T, m=16),
    "frameset_ibl": dict(vis=("vis", 0), base=("a", 0), mat=("b", 0), nv=("c", 0), irr=("d", 0), spec=("e", 0), tab=("tab", 0), n=T, out=("o1", 0),
                         out_bytes=P3, flags=F),
    "frameset_ibl_grad": dict(vis=("vis", 0), base=("a", 0), mat=("b", 0), nv=("c", 0), irr=("d", 0), spec=("e", 0), tab=("tab", 0), n=T,
                              gout=("g", 0), gbase=("o1", 0), gmat=("o2", 0), gnv=("o3", 0), girr=("o4", 0), gspec=("o5", 0), gtab=("o6", 0),
                              flags=F),
}
RF, RG, BT, IF, IG = ENTRIES
RF16 = "the plane buffers (d_vis, d_nrm, d_pos, d_out) must be 16-byte aligned"
RG16 = "the plane buffers (d_vis, d_nrm, d_pos, d_gout, d_gnrm, d_gpos) must be 16-byte aligned"
IF16 = "the plane buffers (d_vis, d_base, d_mat, d_nv, d_irr, d_spec, d_out) must be 16-byte aligned"
IG16 = "the plane buffers (d_vis, d_base, d_mat, d_nv, d_irr, d_spec, d_gout, d_gbase, d_gmat, d_gnv, d_girr, d_gspec) must be 16-byte aligned"
WRONG_SHARD = "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)"
# what an entry point's overlap refusals name in front of their text: the outputs against the inputs
AGAINST = {RF: " (d_out against d_vis, d_nrm, d_pos, d_eye)", RG: " (d_gnrm, d_gpos against d_vis, d_nrm, d_pos, d_eye, d_gout)",
           IF: " (d_out against d_vis, d_base, d_mat, d_nv, d_irr, d_spec, d_tab)",
           IG: " (d_gbase, d_gmat, d_gnv, d_girr, d_gspec, d_gtab against d_vis, d_base, d_mat, d_nv, d_irr, d_spec, d_tab, d_gout)"}
# (entry point, the faulty argument(s), text after "srz_<entry point>"; WRONG_SHARD stands alone; None: no text is set)
CASES = [
    (RF, dict(ctx=None), None), (RF, dict(fs=None), ": null frameset"), (RF, dict(vis=None), ": null d_vis"), (RF, dict(nrm=None), ": null d_nrm"),
    (RF, dict(pos=None), ": null d_pos"), (RF, dict(eye=None), ": null d_eye"), (RF, dict(out=None), ": null d_out"),
    (RF, dict(par_frames=0), ": " + PAR_FRAMES), (RF, dict(par_frames=3), ": " + PAR_FRAMES),
    (RF, dict(out_bytes=P4 - 1), ": out_bytes is too small for d_out"), (RF, dict(flags=abi.UNIFIED), ": " + ONLY_FUSED),
    (RF, dict(flags=F | 16), ": " + ONLY_FUSED), (RF, dict(vis=("vis", 4)), ": " + RF16), (RF, dict(nrm=("a", 8)), ": " + RF16),
    (RF, dict(pos=("b", 4)), ": " + RF16), (RF, dict(out=("o1", 4)), ": " + RF16), (RF, dict(eye=("eye", 2)), ": d_eye must be 4-byte aligned"),
    (RF, dict(out=("vis", 0)), ": " + OUT_IN), (RF, dict(out=("a", 0)), ": " + OUT_IN), (RF, dict(pos=("o1", P4 - 16)), ": " + OUT_IN),
    (RF, dict(eye=("o1", 8)), ": " + OUT_IN), (RF, dict(ctx="sharded"), WRONG_SHARD),
    (RG, dict(ctx=None), None), (RG, dict(fs=None), ": null frameset"), (RG, dict(vis=None), ": null d_vis"), (RG, dict(nrm=None), ": null d_nrm"),
    (RG, dict(pos=None), ": null d_pos"), (RG, dict(eye=None), ": null d_eye"), (RG, dict(gout=None), ": null d_gout"),
    (RG, dict(gnrm=None, gpos=None), ": neither d_gnrm nor d_gpos is asked for"), (RG, dict(par_frames=3), ": " + PAR_FRAMES),
    (RG, dict(flags=4), ": " + ONLY_FUSED), (RG, dict(gout=("g", 8)), ": " + RG16), (RG, dict(gnrm=("o1", 4)), ": " + RG16),
    (RG, dict(gpos=("o2", 12)), ": " + RG16), (RG, dict(eye=("eye", 1)), ": d_eye must be 4-byte aligned"),
    (RG, dict(gnrm=("g", 0)), ": " + OUT_IN), (RG, dict(gpos=("vis", 16)), ": " + OUT_IN), (RG, dict(gpos=("o1", P3 - 16)), ": " + OUT_OUT),
    (RG, dict(ctx="sharded"), WRONG_SHARD),
    (BT, dict(ctx=None), None), (BT, dict(tab=None), ": null d_tab"), (BT, dict(n=1), ": " + TAB_N), (BT, dict(n=0), ": " + TAB_N),
    (BT, dict(n=65, tab_bytes=1 << 20), ": " + TAB_N), (BT, dict(m=0), ": m must be 1 .. 256"), (BT, dict(m=257), ": m must be 1 .. 256"),
    (BT, dict(tab_bytes=TAB - 1), ": tab_bytes is too small for d_tab"), (BT, dict(tab=("o1", 2)), ": d_tab must be 4-byte aligned"),
    (IF, dict(ctx=None), None), (IF, dict(fs=None), ": null frameset"), (IF, dict(vis=None), ": null d_vis"), (IF, dict(mat=None), ": null d_mat"),
    (IF, dict(nv=None), ": null d_nv"), (IF, dict(irr=None), ": null d_irr"), (IF, dict(spec=None), ": null d_spec"), (IF, dict(tab=None), ": null d_tab"),
    (IF, dict(out=None), ": null d_out"), (IF, dict(n=1), ": " + TAB_N), (IF, dict(n=65), ": " + TAB_N),
    (IF, dict(out_bytes=P3 - 1), ": out_bytes is too small for d_out"), (IF, dict(flags=abi.ORDERED_RASTER), ": " + ONLY_FUSED),
    (IF, dict(base=("a", 4)), ": " + IF16), (IF, dict(mat=("b", 8)), ": " + IF16), (IF, dict(nv=("c", 4)), ": " + IF16), (IF, dict(irr=("d", 4)), ": " + IF16),
    (IF, dict(spec=("e", 4)), ": " + IF16), (IF, dict(out=("o1", 4)), ": " + IF16), (IF, dict(tab=("tab", 2)), ": d_tab must be 4-byte aligned"),
    (IF, dict(out=("vis", 0)), ": " + OUT_IN), (IF, dict(out=("a", 0)), ": " + OUT_IN), (IF, dict(out=("c", 0)), ": " + OUT_IN),
    (IF, dict(tab=("o1", 4)), ": " + OUT_IN), (IF, dict(nv=("o1", P3 - 16)), ": " + OUT_IN), (IF, dict(ctx="sharded"), WRONG_SHARD),
    (IG, dict(ctx=None), None), (IG, dict(fs=None), ": null frameset"), (IG, dict(vis=None), ": null d_vis"), (IG, dict(mat=None), ": null d_mat"),
    (IG, dict(nv=None), ": null d_nv"), (IG, dict(irr=None), ": null d_irr"), (IG, dict(spec=None), ": null d_spec"), (IG, dict(tab=None), ": null d_tab"),
    (IG, dict(gout=None), ": null d_gout"),
    (IG, dict(gbase=None, gmat=None, gnv=None, girr=None, gspec=None, gtab=None), ": none of d_gbase, d_gmat, d_gnv, d_girr, d_gspec, d_gtab is asked for"),
    (IG, dict(base=None), ": d_gbase needs d_base"), (IG, dict(n=1), ": " + TAB_N), (IG, dict(n=65), ": " + TAB_N), (IG, dict(flags=1), ": " + ONLY_FUSED),
    (IG, dict(gout=("g", 4)), ": " + IG16), (IG, dict(gbase=("o1", 4)), ": " + IG16), (IG, dict(gmat=("o2", 8)), ": " + IG16),
    (IG, dict(gnv=("o3", 4)), ": " + IG16), (IG, dict(girr=("o4", 4)), ": " + IG16), (IG, dict(gspec=("o5", 12)), ": " + IG16),
    (IG, dict(gtab=("o6", 2)), ": d_tab and d_gtab must be 4-byte aligned"), (IG, dict(tab=("tab", 1)), ": d_tab and d_gtab must be 4-byte aligned"),
    (IG, dict(gbase=("g", 0)), ": " + OUT_IN), (IG, dict(gtab=("tab", TAB - 4)), ": " + OUT_IN), (IG, dict(gnv=("vis", 0)), ": " + OUT_IN),
    (IG, dict(gtab=("e", 64)), ": " + OUT_IN), (IG, dict(gmat=("o1", P3 - 16)), ": " + OUT_OUT), (IG, dict(gtab=("o5", 4)), ": " + OUT_OUT),
    (IG, dict(ctx="sharded"), WRONG_SHARD),
]


def case_id(case):
    entry, fault, _ = case
    return entry + "-" + "-".join(f"{k}={v[0] + '+' + str(v[1]) if isinstance(v, tuple) else v}" for k, v in fault.items())


assert len({case_id(c) for c in CASES}) == len(CASES)


@pytest.fixture(scope="module")
def kit():
    """the contexts, the set and the buffers every case draws its arguments from"""
    tris = soup(3, TRIS, W, H, (10.0, 20.0, 30.0))
    main, sharded = srz.Context(0), srz.Context(0, 0, 2)
    k = types.SimpleNamespace(ctx={"main": main, "sharded": sharded})
    k.fs = main.frameset([frame(tris, W, H), frame(tris[::-1].copy(), W, H)])
    vis = torch.zeros(k.fs.out_shape, dtype=torch.float32, device="cuda")
    assert vis.numel() * 4 == P4 == k.fs.out_bytes and [k.fs.interpolate_bytes(c) for c in (3, 2, 1)] == [P3, P2, P1]
    k.fs.render_visibility(vis.data_ptr(), P4, F, stream())
    torch.cuda.synchronize()
    half = lambda nbytes: torch.full((nbytes // 4,), 0.5, dtype=torch.float32, device="cuda")  # noqa: E731
    out = lambda: torch.full((P4 // 4 + 64,), 0x5eed5eed, dtype=torch.int32, device="cuda")  # noqa: E731
    k.buf = {"vis": vis, **{name: half(P4) for name in "abcdeg"}, "eye": half(64), "tab": half(2 * TAB), **{f"o{i}": out() for i in range(1, 7)}}
    k.before = {name: t.clone() for name, t in k.buf.items()}
    yield k
    k.fs.close()
    main.close(), sharded.close()


def call(kit, entry, fault):
    args = dict(ctx="main", fs="main", **ENTRIES[entry])
    assert set(fault) <= set(args), (entry, fault)
    args.update(fault)
    h = kit.ctx[args.pop("ctx")].h if args["ctx"] is not None else args.pop("ctx")
    fs = kit.fs.h if args.pop("fs") is not None else None
    values = [kit.buf[v[0]].data_ptr() + v[1] if isinstance(v, tuple) else v for v in args.values()]
    head = (h,) if entry == BT else (h, fs)
    return getattr(srz.lib(), "srz_" + entry)(*head, *values, None), h


def untouched(kit):
    torch.cuda.synchronize()
    for name, t in kit.buf.items():
        assert torch.equal(t, kit.before[name]), f"{name} was written"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_refusal(kit, case):
    entry, fault, text = case
    lib = srz.lib()
    marker = "srz_frameset_render: null frameset / output"
    for c in kit.ctx.values():
        assert lib.srz_frameset_render(c.h, None, None, 0, 0, None) == E and lib.srz_last_error(c.h).decode() == marker
    rc, h = call(kit, entry, fault)
    assert rc == E, (rc, lib.srz_last_error(h))
    if text is None:
        assert h is None and all(lib.srz_last_error(c.h).decode() == marker for c in kit.ctx.values())
    else:
        if text in (": " + OUT_IN, ": " + OUT_OUT):
            text = AGAINST[entry] + text
        assert lib.srz_last_error(h).decode() == (text if text is WRONG_SHARD else f"srz_{entry}{text}")
    untouched(kit)


def test_the_valid_calls_are_accepted(kit):
    """ENTRIES' arguments are a valid call of each entry point, and so are the calls that leave out what may be left out"""
    kit.buf["o6"].zero_()  # (added into: the sentinel as a float would swallow the adds)
    for entry, fault in ((RF, {}), (RF, dict(par_frames=2)), (RG, {}), (RG, dict(gnrm=None)), (RG, dict(gpos=None)), (BT, {}), (BT, dict(n=2, m=1)),
                         (IF, {}), (IF, dict(base=None)), (IF, dict(n=2)), (IG, {}), (IG, dict(base=None, gbase=None)),
                         (IG, dict(gbase=None, gmat=None, gnv=None, girr=None, gspec=None)), (IG, dict(gtab=None))):
        rc, h = call(kit, entry, fault)
        assert rc == 0, (entry, fault, srz.lib().srz_last_error(h))
    torch.cuda.synchronize()
    for name in ("o1", "o2", "o3", "o4", "o5"):
        assert not torch.equal(kit.buf[name], kit.before[name]), name
    assert bool(kit.buf["o6"].any())
    for name, t in kit.buf.items():
        t.copy_(kit.before[name])
