"""-m gpu: SH9 lighting — srz_frameset_sh / _sh_grad (k_sh, k_sh_grad, k_light_fold) and srz_cube_sh / _cube_sh_grad (k_cube_sh,
k_cube_sh_finish, k_cube_sh_q, k_cube_sh_grad).  The visibility buffer is the GPU's own render_visibility, except where a test
writes one by hand; the normals are the GPU's own interpolate of the frames' normals, except where a test writes them by hand; the
expected values are tests/shref.py's on those very buffers (pinned on the CPU by tests/test_sh_ref.py).
Forward, gnrm, the cube's sh, den and gsrc: a NaN on one side must be a NaN on the other, every other word matches bit for bit.
gsh: within gamma_n * sum |term| of the reference's double sums, gamma_n = n u / (1 - n u), u = 2^-24, n the entry's contributing
pixels — the bound of any summation tree, the terms being the rule's float32 terms on both sides: derived, not measured —, bit-equal
between two launches, the float32 term itself where one pixel contributes, +0 where nobody does."""
import numpy as np
import pytest
import torch

import shref
from srz import abi, parallel
from support import SENTINEL, ccw, ctx, filled, frame, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
BACKDROP = ccw((-8, -8), (400, -8), (-8, 400), z=80.0, uv=((0.1, 0.2), (0.9, 0.3), (0.4, 0.95)))
BACKDROP["nrm"] = np.float32([(0.3, -0.3, 0.9), (-0.4, 0.2, 0.8), (0.1, -0.2, 0.95)])
SIZES = [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6), (1, 1, 3)]
CHANNELS, KINDS = (1, 3, 7), (shref.IRRADIANCE, shref.RADIANCE)


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


def rand_ids(rng, n, h, w, tris):
    ids = rng.integers(1, tris + 1, (n, h, w)).astype(np.uint32)
    ids |= (rng.random((n, h, w)) < 0.4).astype(np.uint32) << 31
    ids[rng.random((n, h, w)) < 0.1] = 0
    return ids


def sh_dims(sh):
    sh = np.ascontiguousarray(sh, np.float32)
    return sh, sh.shape[-1], (sh.shape[0] if sh.ndim == 3 else 1)


def fwd(fs, vis, nrm, sh, kind, flags=F, fill=0):
    """the forward pass into a buffer prefilled with the word `fill` → uint32 [n, C, rows, W]; nrm: a device tensor"""
    sh, C, sf = sh_dims(sh)
    out, st = filled(fs.interpolate_shape(C), fill), dev(sh)
    fs.sh(vis.data_ptr(), nrm.data_ptr(), st.data_ptr(), C, sf, kind, out.data_ptr(), fs.interpolate_bytes(C), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def bwd(fs, vis, nrm, sh, kind, gout, want=(True, True), flags=F, fill=0):
    """the backward pass → (gnrm uint32 [n, 3, rows, W] from `fill`, gsh float32 of sh's shape [sf, 9, C] from SENTINEL words); None
    where not wanted"""
    sh, C, sf = sh_dims(sh)
    st, g = dev(sh), dev(gout)
    gnrm = filled(fs.interpolate_shape(3), fill) if want[0] else None
    gsh = filled((sf, 9, C), SENTINEL) if want[1] else None
    nbytes = fs.sh_work_bytes(C) if want[1] else 0
    work = filled((nbytes // 4,), SENTINEL) if want[1] else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    fs.sh_grad(vis.data_ptr(), nrm.data_ptr(), st.data_ptr(), C, sf, kind, g.data_ptr(), ptr(gnrm), ptr(gsh), ptr(work), nbytes, flags, stream())
    torch.cuda.synchronize()
    return (None if gnrm is None else words(gnrm)), (None if gsh is None else words(gsh).view(np.float32))


def sh_of(sh, i):
    return sh[i] if sh.ndim == 3 else sh


def expect_fwd(tmp_path, frames, v, nw, sh, kind, fused=True, fill=0):
    """v: the visibility buffer's words [n, 4, rows, W]; nw: the normals float32 [n, 3, rows, W]"""
    C = sh.shape[-1]
    return np.stack([shref.forward(tmp_path, n_tris(f), v[i, 1], nw[i], sh_of(sh, i), kind, fused, np.full((C,) + v.shape[2:], fill, np.uint32))
                     for i, f in enumerate(frames)])


def expect_bwd(tmp_path, frames, v, nw, sh, kind, gout, fused=True, fill=0):
    """(Grad per coefficient frame — one for shared coefficients —, gnrm [n, 3, rows, W] float32)"""
    sh = np.ascontiguousarray(sh, np.float32)
    shared = sh.ndim == 2
    accs = [shref.Grad(sh.shape[-1]) for _ in range(1 if shared else len(frames))]
    planes = [shref.grad(tmp_path, n_tris(f), v[i, 1], nw[i], sh_of(sh, i), kind, gout[i], accs[0 if shared else i], fused,
                         np.full((3,) + v.shape[2:], fill, np.uint32)) for i, f in enumerate(frames)]
    return accs, np.stack(planes)


RATIOS = []


def check_gsh(got, accs, what, extra=0):
    ref, bound = np.stack([a.gsum for a in accs]), np.stack([a.bound(extra) for a in accs])
    cnt = np.stack([a.count for a in accs])
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(ref).all()
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    RATIOS.append(ratio)
    print(f"{what}: max err {err.max():.3e}, max err / bound {ratio:.3f} (largest so far {max(RATIOS):.3f}), max n {int(cnt.max())}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} entries beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    assert not got[cnt == 0].view(np.uint32).any()  # +0 where nobody contributes


def rendered(ctx, w, h, n, k=2):
    frames = pair(w, h, n, F, k)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    assert (v[:, 1] != 0).any(1).any(1).all()
    nrm = interp_normals(fs, vis, frames)
    return frames, fs, vis, v, nrm, nrm.cpu().numpy(), owners(v, frames)


def rand_gout(seed, shape, own):
    """gout normal [n, C, rows, W]; nobody's words NaN: they may hold anything"""
    g = np.random.default_rng([seed, 9]).normal(0, 2, shape).astype(np.float32)
    g[np.broadcast_to(~own[:, None], g.shape)] = np.nan
    return g


# ------------------------------------------------------------------------------------------------------ the pixel pass
@pytest.mark.parametrize("w,h,n", SIZES)
def test_forward_and_gradients(ctx, tmp_path, w, h, n):
    """every channel count and kind, shared and per-frame coefficients, over a sentinel prefill: the forward and gnrm bit for bit; gsh
    within its bound, the same words from a second launch, every entry overwritten; each output alone gives the same words"""
    frames, fs, vis, v, nrm, nw, own = rendered(ctx, w, h, n)
    for C in CHANNELS:
        both = shref.make_sh(w + C, C, frames=2)
        gout = rand_gout(w + C, (2, C, h, w), own)
        for kind in KINDS:
            for sh in (both, both[0]):
                what = f"{w}x{h} C {C} kind {kind} sh {sh.ndim}"
                got = fwd(fs, vis, nrm, sh, kind, F, SENTINEL)
                same(got, expect_fwd(tmp_path, frames, v, nw, sh, kind, fill=SENTINEL), what)
                assert (got[np.broadcast_to(~own[:, None], got.shape)] == 0).all() and (got != 0).any()
                gn, gsh = bwd(fs, vis, nrm, sh, kind, gout, fill=SENTINEL)
                accs, plane = expect_bwd(tmp_path, frames, v, nw, sh, kind, gout, fill=SENTINEL)
                same(gn, plane, what + " gnrm")
                assert not (gsh.view(np.uint32) == SENTINEL).any()  # written, every entry
                check_gsh(gsh, accs, what + " gsh")
                alone = bwd(fs, vis, nrm, sh, kind, gout, (False, True))
                assert alone[0] is None and np.array_equal(alone[1].view(np.uint32), gsh.view(np.uint32)), what + ": two launches differ"
                only = bwd(fs, vis, nrm, sh, kind, gout, (True, False), fill=SENTINEL)
                assert only[1] is None and np.array_equal(only[0], gn), what + ": gnrm alone differs"
    fs.close()


def test_not_fused_keeps_nobodys_words(ctx, tmp_path):
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
    C, kind = 3, shref.IRRADIANCE
    sh = shref.make_sh(5, C)
    nw, gout = (np.stack(t) for t in zip(*(shref.hostile_planes(rng, (80, 96), C) for _ in range(2))))
    for t in (nw, gout):
        t[np.broadcast_to(~own[:, None], t.shape)] = np.nan  # never read
    nrm = dev(nw)
    fused, kept = fwd(fs, vis, nrm, sh, kind, F, SENTINEL), fwd(fs, vis, nrm, sh, kind, 0, SENTINEL)
    same(fused, expect_fwd(tmp_path, frames, vw, nw, sh, kind, True, SENTINEL), "fused")
    same(kept, expect_fwd(tmp_path, frames, vw, nw, sh, kind, False, SENTINEL), "not fused")
    assert (fused[0][:, nobody] == 0).all() and (kept[0][:, nobody] == SENTINEL).all() and (kept[0][:, own[0]] != SENTINEL).all()
    for fl, fused_ in ((F, True), (0, False)):
        gn, _ = bwd(fs, vis, nrm, sh, kind, gout, (True, False), flags=fl, fill=SENTINEL)
        _, plane = expect_bwd(tmp_path, frames, vw, nw, sh, kind, gout, fused_, SENTINEL)
        same(gn, plane, f"fused {fused_}")
        assert (gn[0][:, nobody] == (0 if fused_ else SENTINEL)).all()
    fs.close()


def test_hostile_normals_under_a_hand_written_buffer(ctx, tmp_path):
    """normals written by hand (shref.hostile_planes: zero, subnormal, huge, inf, NaN, the axes) under a hand-written visibility
    buffer with holes, non-finite gout: lit or not as the rule says, and every word matches; gsh with gout made finite"""
    w, h, n = 96, 64, 2
    rng = np.random.default_rng(41)
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    ids = rand_ids(rng, n, h, w, 20)
    v = hand_vis(ids)
    vw = v.view(np.uint32)
    vis = torch.as_tensor(v).cuda()
    own = owners(vw, frames)
    for C in (3, 7):
        sh = shref.make_sh(6, C, frames=2)
        nw, gout = (np.stack(t) for t in zip(*(shref.hostile_planes(rng, (h, w), C) for _ in range(n))))
        lit = np.stack([(shref.classify(tmp_path, 20, ids[i], nw[i]) & shref.LIT) != 0 for i in range(n)])
        for name, m in (("nobody", ~own), ("not lit", own & ~lit), ("lit", lit), ("non-finite gout", lit & ~np.isfinite(gout).all(1)),
                        ("a NaN normal", own & np.isnan(nw).any(1)), ("an infinite normal", own & np.isinf(nw).any(1))):
            assert int(m.sum()) >= 50, (name, int(m.sum()))
        nrm = dev(nw)
        for kind in KINDS:
            got = fwd(fs, vis, nrm, sh, kind, F, SENTINEL)
            same(got, expect_fwd(tmp_path, frames, vw, nw, sh, kind, fill=SENTINEL), "hostile forward")
            assert (got[np.broadcast_to((own & ~lit)[:, None], got.shape)] == 0).all()
            assert np.isfinite(got.view(np.float32)).all()  # a normal that is not finite is not lit: no NaN comes out of it
            gn, _ = bwd(fs, vis, nrm, sh, kind, gout, (True, False), fill=SENTINEL)
            _, plane = expect_bwd(tmp_path, frames, vw, nw, sh, kind, gout, fill=SENTINEL)
            same(gn, plane, "hostile gnrm")
            assert np.isnan(gn.view(np.float32)).any()  # a NaN gout of a lit pixel is a NaN on both sides
            gf = np.where(np.abs(gout) < 1e6, gout, np.float32(-1.5))
            for s in (sh, sh[1]):
                gn, gsh = bwd(fs, vis, nrm, s, kind, gf, fill=SENTINEL)
                accs, plane = expect_bwd(tmp_path, frames, vw, nw, s, kind, gf, fill=SENTINEL)
                same(gn, plane, "hostile finite gnrm")
                check_gsh(gsh, accs, f"hostile gsh C {C} kind {kind} sh {s.ndim}")
    fs.close()


def test_gsh_of_one_pixel_is_its_float32_term(ctx, tmp_path):
    """exactly one owned pixel in the set: every add of the tree adds +0, so each entry is the pixel's float32 term, bit for bit
    (+ 0.0f on both sides: a term of -0 comes out +0, as the header says); the other frame's row, to which nobody contributes, is
    +0 in every entry"""
    w, h, C = 70, 40, 3
    frames = hand_frames(w, h, 2, 20)
    fs = ctx.frameset(frames)
    sh = shref.make_sh(8, C, frames=2)
    for (fi, y, x) in ((0, 0, 0), (1, 37, 69), (0, 33, 31)):
        ids = np.zeros((2, h, w), np.uint32)
        ids[fi, y, x] = 5
        nw, gout = (np.stack([t, t]) for t in shref.make_planes(7, (h, w), C))
        for kind in KINDS:
            _, gsh = bwd(fs, torch.as_tensor(hand_vis(ids)).cuda(), dev(nw), sh, kind, gout, (False, True))
            acc = shref.Grad(C)
            _, terms = shref.grad(tmp_path, 20, ids[fi], nw[fi], sh[fi], kind, gout[fi], into=acc, want_terms=True)
            t = terms[:, :, y, x]
            assert (acc.count == 1).all() and (t != 0).all()
            same(gsh[fi] + np.float32(0), t + np.float32(0), f"one pixel {fi} {y} {x}")
            assert not gsh[1 - fi].view(np.uint32).any()
            # shared coefficients: the one row is 0 + row 0 + row 1 in float32
            _, one = bwd(fs, torch.as_tensor(hand_vis(ids)).cuda(), dev(nw), sh[fi], kind, gout, (False, True))
            same(one[0] + np.float32(0), t + np.float32(0), "one pixel, shared")
    fs.close()


def test_shared_coefficients_are_the_frame_order_sum_of_the_per_frame_rows(ctx):
    """include/srz.h states it, so it is checkable bit for bit: one set of coefficients for every frame gives, per entry, 0 + row 0 +
    row 1 + ... in float32 of the rows the call with those coefficients repeated per frame writes; nine frames take the walk's other
    branch (workgroup b serves the frames f = b mod 8), so a workgroup's LDS partials are reused across frames"""
    for k in (2, 9):
        frames, fs, vis, v, nrm, nw, own = rendered(ctx, 64, 64, 90, k=k)
        gout = rand_gout(3, (k, 7, 64, 64), own)
        one = shref.make_sh(9, 7)
        shared = bwd(fs, vis, nrm, one, shref.IRRADIANCE, gout, (False, True))[1]
        rows = bwd(fs, vis, nrm, np.repeat(one[None], k, 0), shref.IRRADIANCE, gout, (False, True))[1]
        s = np.zeros(rows.shape[1:], np.float32)
        for i in range(k):
            s = s + rows[i]
        assert shared.shape == (1, 9, 7) and np.array_equal(shared[0].view(np.uint32), s.view(np.uint32)) and (s != 0).all()
        fs.close()


def test_a_rank_without_bands_writes_every_row_of_gsh():
    """rank 1 of world 2 on a 32-row frame holds no band: no tile, no kernel over tiles — and still d_gsh is WRITTEN, +0 in every
    entry, with per-frame and with shared coefficients; no word of the planes is touched"""
    import srz
    assert len(parallel.band_rows(32, 1, 2)) == 0
    c = srz.Context(0, 1, 2)
    sfs = c.frameset(hand_frames(64, 32, 2, 20))
    C = 3
    vis = torch.zeros(sfs.out_shape, dtype=torch.float32, device="cuda")
    nrm = torch.ones(sfs.interpolate_shape(3), dtype=torch.float32, device="cuda")
    g = torch.ones(sfs.interpolate_shape(C), dtype=torch.float32, device="cuda")
    gn, out = filled(sfs.interpolate_shape(3), SENTINEL), filled(sfs.interpolate_shape(C), SENTINEL)
    nbytes = sfs.sh_work_bytes(C)
    assert nbytes == 2 * 9 * C * 4  # no partials, a row per frame
    for sf in (2, 1):
        sh = dev(shref.make_sh(3, C, frames=2)[:sf])
        gsh, work = filled((sf, 9, C), SENTINEL), filled((nbytes // 4,), SENTINEL)
        sfs.sh_grad(vis.data_ptr(), nrm.data_ptr(), sh.data_ptr(), C, sf, 0, g.data_ptr(), gn.data_ptr(), gsh.data_ptr(), work.data_ptr(), nbytes,
                    F, stream())
        torch.cuda.synchronize()
        assert not words(gsh).any(), (sf, words(gsh))
    sfs.sh(vis.data_ptr(), nrm.data_ptr(), sh.data_ptr(), C, 1, 0, out.data_ptr(), sfs.interpolate_bytes(C), F, stream())
    torch.cuda.synchronize()
    assert (words(gn) == SENTINEL).all() and (words(out) == SENTINEL).all()
    sfs.close(), c.close()


# ------------------------------------------------------------------------------------------------------ the cube pass
def cube_calls(ctx, cube):
    """→ (sh [frames, 9, C], den [1], a closure gsh → gsrc), float32 numpy, every output from SENTINEL words"""
    frames, _, n, _, C = cube.shape
    src = dev(cube)
    sh, den = filled((frames, 9, C), SENTINEL), filled((1,), SENTINEL)
    nbytes = ctx.cube_sh_work_bytes(n, C, frames)
    work = filled((nbytes // 4,), SENTINEL)
    ctx.cube_sh(src.data_ptr(), n, C, frames, sh.data_ptr(), den.data_ptr(), work.data_ptr(), nbytes, stream())
    torch.cuda.synchronize()

    def back(gsh):
        g, gsrc = dev(gsh), filled(cube.shape, SENTINEL)
        ctx.cube_sh_grad(g.data_ptr(), den.data_ptr(), n, C, frames, gsrc.data_ptr(), work.data_ptr(), nbytes, stream())
        torch.cuda.synchronize()
        return words(gsrc)
    return words(sh), words(den), back


@pytest.mark.parametrize("n", [1, 2, 3, 8, 63, 64, 65, 130])
def test_cube_sh_is_the_reference_bit_for_bit(ctx, tmp_path, n):
    """every channel count, one and two frames: sh, den and gsrc are the reference's words (65 and 130 make lanes take two and three
    columns; 7 channels take two register groups); a second launch gives the same words; without d_den the same sh"""
    for C in CHANNELS:
        for frames in (1, 2):
            cube = shref.make_cube(n + C, n, C, frames)
            sh, den, back = cube_calls(ctx, cube)
            want_sh, want_den = shref.cube_sh(tmp_path, cube)
            what = f"n {n} C {C} frames {frames}"
            same(sh, want_sh, what + " sh")
            same(den, want_den, what + " den")
            gsh = np.random.default_rng([n, C]).normal(0, 1, (frames, 9, C)).astype(np.float32)
            gsrc = back(gsh)
            same(gsrc, shref.cube_sh_grad(tmp_path, gsh, want_den, n), what + " gsrc")
            sh2, den2, back2 = cube_calls(ctx, cube)
            assert np.array_equal(sh2, sh) and np.array_equal(den2, den) and np.array_equal(back2(gsh), gsrc), what + ": two launches differ"
    src, out = dev(cube), filled((frames, 9, C), SENTINEL)
    nbytes = ctx.cube_sh_work_bytes(n, C, frames)
    work = filled((nbytes // 4,), SENTINEL)
    ctx.cube_sh(src.data_ptr(), n, C, frames, out.data_ptr(), None, work.data_ptr(), nbytes, stream())
    torch.cuda.synchronize()
    assert np.array_equal(words(out), sh)


@pytest.mark.parametrize("n", [3, 65])
def test_a_nan_texel_reaches_its_own_channel_and_frame_only(ctx, tmp_path, n):
    cube = shref.make_cube(14, n, 3, 2)
    cube[1, 2, n // 2, n - 1, 1] = np.nan
    sh, den, _ = cube_calls(ctx, cube)
    want, _ = shref.cube_sh(tmp_path, cube)
    same(sh, want, "a NaN texel")
    nan = np.isnan(sh.view(np.float32))
    expect = np.zeros_like(nan)
    expect[1, :, 1] = True
    assert np.array_equal(nan, expect) and np.isfinite(den.view(np.float32)).all()
