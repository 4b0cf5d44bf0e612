"""-m gpu: gradients to vertex positions from a visibility buffer (srz_frameset_position_grad, k_pos_grad).  The visibility buffer is
the GPU's own render_visibility, except where a test writes one by hand; the expected values are tests/posgradref.py's on that
buffer (pinned on the CPU by tests/test_posgrad_ref.py).  gpix: a NaN on one side must be a NaN on the other, every other word
matches bit for bit.  gpos: exact where every partial sum is representable (the dyadic cases), else within gamma_n * sum |term|,
gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing pixels — one rounding per add, the terms being float32 terms
on both sides: derived, not measured."""
import numpy as np
import pytest
import torch

import interpref
import posgradref
from srz import abi, parallel
from support import SENTINEL, ccw, ctx, filled, frame, padded_positions, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
BACKDROP = ccw((-8, -8), (400, -8), (-8, 400), z=(80.0, 60.0, 70.0))
SIZES = [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6), (1, 1, 3)]
INPUTS = ((True, False), (False, True), (True, True))  # (gbary, gz)
OUTPUTS = ((True, False), (False, True), (True, True))  # (gpos, gpix)


def call(fs, vis, gbary, gz, T, want_pos=True, want_pix=True, flags=F, fill=0, into=None):
    """one srz_frameset_position_grad → (gpos float32 [n, T, 3, 3], added into `into` or zeros; gpix uint32 [n, 2, rows, W] from `fill`)"""
    gb = None if gbary is None else torch.as_tensor(np.ascontiguousarray(gbary, np.float32)).cuda()
    g = None if gz is None else torch.as_tensor(np.ascontiguousarray(gz, np.float32)).cuda()
    assert gb is None or tuple(gb.shape) == tuple(fs.interpolate_shape(2))
    assert g is None or tuple(g.shape) == tuple(fs.interpolate_shape(1))
    gp = (torch.zeros((fs.n_frames, T, 3, 3), dtype=torch.float32, device="cuda") if into is None else torch.as_tensor(into).cuda()) if want_pos else None
    gx = filled(fs.interpolate_shape(2), fill) if want_pix else None
    fs.position_grad(vis.data_ptr(), gb.data_ptr() if gb is not None else None, g.data_ptr() if g is not None else None, T,
                     gp.data_ptr() if want_pos else None, gx.data_ptr() if want_pix else None, flags, stream())
    torch.cuda.synchronize()
    return (gp.cpu().numpy() if want_pos else None), (words(gx) if want_pix else None)


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def expect(tmp_path, frames, v, gbary, gz, T, fused=True, fill=0):
    """(a posgradref.Grad per frame, gpix [n, 2, rows, W] float32)"""
    pos = padded_positions(frames, T)
    accs, gx = [posgradref.Grad(T) for _ in frames], []
    for i, f in enumerate(frames):
        pre = np.full((2,) + v.shape[2:], fill, np.uint32)
        gx.append(posgradref.grad(tmp_path, pos[i], f.n_tris, v[i], None if gbary is None else gbary[i],
                                  None if gz is None else gz[i], accs[i], True, fused, pre))
    return accs, np.stack(gx)


def check_gpos(got, accs, what, exact=False, calls=1):
    """finite elements: within the bound (0 when exact), bit for bit where n = 1, exactly 0 where n = 0; an element some term of which
    is not finite: NaN where the reference has NaN, the reference's infinity where it has one"""
    ref = calls * np.stack([a.gpos for a in accs])
    mag = np.stack([a.gabs for a in accs])
    bound = np.stack([a.bound(calls) for a in accs])
    cnt = np.stack([np.broadcast_to(a.count[:, None, None], a.gpos.shape) for a in accs])
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(mag)
    assert np.isfinite(ref[fin]).all()
    if exact:
        assert fin.all() and (ref.astype(np.float32).astype(np.float64) == ref).all(), "the case is not dyadic"
        bound = np.zeros_like(bound)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - ref)
    ratio = err[fin & (bound > 0)] / bound[fin & (bound > 0)]
    print(f"{what}: max err {err[fin].max():.3e}, max err / bound {ratio.max() if ratio.size else 0:.3f}, max n {int(cnt.max())}")
    bad = fin & ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    assert np.array_equal(np.isnan(got[~fin]), np.isnan(ref[~fin])), what + ": NaN elements"
    inf = ~fin & np.isinf(ref)
    assert np.array_equal(got[inf].astype(np.float64), ref[inf]), what + ": infinite elements"
    if calls == 1:
        one = fin & (cnt == 1)
        same((got + np.float32(0))[one], (ref.astype(np.float32) + np.float32(0))[one], what + " (n = 1)")
    assert (got[cnt == 0] == 0).all()


def pair(w, h, n, flags=F, k=2):
    t = np.concatenate([soup(2, n, w, h, ZS, big=w < 40), BACKDROP])
    return [frame(t, w, h, flags=flags) for _ in range(k)]


def rand_grads(seed, fs, own=None, sigma=2.0):
    """(gbary [n, 2, rows, W], gz [n, 1, rows, W]) float32; with `own` [n, rows, W] the words at nobody's pixels are NaN"""
    rng = np.random.default_rng([seed, 77])
    gb = rng.normal(0, sigma, fs.interpolate_shape(2)).astype(np.float32)
    gz = rng.normal(0, sigma, fs.interpolate_shape(1)).astype(np.float32)
    if own is not None:
        gb[np.broadcast_to(~own[:, None], gb.shape)] = np.nan
        gz[np.broadcast_to(~own[:, None], gz.shape)] = np.nan
    return gb, gz


def owned(v, frames):
    return np.stack([((v[i, 1] & 0x7fffffff) - np.uint32(1)) < f.n_tris for i, f in enumerate(frames)])


# ------------------------------------------------------------------------------------------------------ sizes and edges
@pytest.mark.parametrize("w,h,n", SIZES)
def test_sizes_inputs_and_outputs(ctx, tmp_path, w, h, n):
    frames = pair(w, h, n)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    own = owned(v, frames)
    assert own.any(1).any(1).all()
    T = n + 3  # (the frames have n + 1 triangles)
    gb, gz = rand_grads(w, fs, own)
    for use_b, use_z in INPUTS:
        b, z = gb if use_b else None, gz if use_z else None
        accs, want_px = expect(tmp_path, frames, v, b, z, T, fill=SENTINEL)
        for want_pos, want_pix in OUTPUTS:
            what = f"{w}x{h} gbary {use_b} gz {use_z} gpos {want_pos} gpix {want_pix}"
            gp, gx = call(fs, vis, b, z, T, want_pos, want_pix, fill=SENTINEL)
            if want_pix:
                same(gx, want_px, what)
                assert (gx[:, 0][~own] == 0).all() and (gx[:, 1][~own] == 0).all()
            if want_pos:
                assert np.isfinite(gp).all()
                check_gpos(gp, accs, what)
                assert (gp[..., 2] != 0).any() == use_z  # without gz the z slots receive no add
    fs.close()


def test_nine_frames_wrap_the_frame_deal(ctx, tmp_path):
    """nine frames; frame 4 has fewer triangles than pos_tris, frame 5 too and its buffer holds ids beyond its count: nobody"""
    t = np.concatenate([soup(12, 60, 64, 64, ZS), BACKDROP])
    frames = []
    for i in range(9):
        t2 = t.copy()
        t2["pos"][:-1, :, :2] += np.float32([1.5 * i, -1.0 * i])
        frames.append(frame(t2[:40] if i in (4, 5) else t2, 64, 64))
    fs = ctx.frameset(frames)
    hv = visibility(fs).cpu().numpy()
    hv[5] = hv[0]  # ids up to 61 in a frame of 40 triangles
    vis = torch.as_tensor(hv).cuda()
    v = hv.view(np.uint32)
    own = owned(v, frames)
    assert ((v[5, 1] & 0x7fffffff) > 40).sum() > 100 and own[5].sum() > 100 and (~own[5]).sum() > (~own[0]).sum()
    T = 63
    gb, gz = rand_grads(9, fs, own)
    gp, gx = call(fs, vis, gb, gz, T, fill=SENTINEL)
    accs, want_px = expect(tmp_path, frames, v, gb, gz, T, fill=SENTINEL)
    same(gx, want_px, "nine frames gpix")
    check_gpos(gp, accs, "nine frames gpos")
    assert len({gp[i].tobytes() for i in range(9)}) == 9 and (gp[4:6, 40:] == 0).all() and (gp[0, 40:61] != 0).any()
    fs.close()


# ------------------------------------------------------------------------------------------------------ exact
def run_ids(rng, n, h, w, tris, max_run, holes=True):
    """[n, h, w] id words: runs of 1 .. max_run pixels of one owner over the raster (they straddle quads, the 8-lane rows of a wave,
    tiles and bands), either class, some pixels nobody's"""
    total = n * h * w
    lens = rng.integers(1, max_run + 1, total)
    owner = rng.integers(1, tris + 1, total).astype(np.uint32)
    ids = np.repeat(owner, lens)[:total]
    ids |= (rng.random(total) < 0.4).astype(np.uint32) << 31
    if holes:
        ids[rng.random(total) < 0.1] = 0
    return ids.reshape(n, h, w)


def table_hash(key):
    """the slot k_pos_grad's table tries first for key = triangle index + 1 (a multiplicative hash into 128 slots)"""
    return ((key * 0x9e3779b1) & 0xffffffff) >> 25


def dyadic_case(name):
    """(w, h, frames, triangles, ids [n, h, w])"""
    rng = np.random.default_rng([len(name), 5])
    if name == "one owner filling a tile":
        return 32, 32, 1, 5, np.full((1, 32, 32), 3, np.uint32)
    if name == "one owner, many tiles, nine frames":
        return 64, 64, 9, 5, np.full((9, 64, 64), 3, np.uint32) | (rng.random((9, 64, 64)) < 0.3).astype(np.uint32) << 31
    if name == "runs across quads and rows":
        return 96, 96, 2, 300, run_ids(rng, 2, 96, 96, 300, 13)
    if name == "long runs":
        return 96, 96, 2, 7, run_ids(rng, 2, 96, 96, 7, 150)
    if name == "four owners in a quad":
        ys, xs = np.mgrid[0:64, 0:64]
        return 64, 64, 1, 37, (1 + (xs + 7 * ys) % 37).astype(np.uint32)[None]
    if name == "1024 owners in a tile":
        return 32, 32, 1, 1024, (rng.permutation(1024).astype(np.uint32) + 1).reshape(1, 32, 32)
    if name == "colliding owners":
        keys = np.arange(1, 2001)
        clash = keys[table_hash(keys) == table_hash(7)][:12]  # twelve owners that try one slot first: four probes serve four
        assert len(clash) == 12
        ids = np.repeat(rng.choice(clash, 2 * 64 * 64 // 3 + 1), 3)[:2 * 64 * 64].astype(np.uint32)
        return 64, 64, 2, 2000, ids.reshape(2, 64, 64)
    if name == "partial tiles":
        return 50, 37, 2, 40, run_ids(rng, 2, 37, 50, 40, 9)
    raise KeyError(name)


DYADIC = ("one owner filling a tile", "one owner, many tiles, nine frames", "runs across quads and rows", "long runs", "four owners in a quad",
          "1024 owners in a tile", "colliding owners", "partial tiles")


def dyadic_tris(rng, n):
    """n right triangles with legs 2, 4 or 8 along the axes at integer places, either winding: area a power of two (8 .. 64, either
    sign), every edge difference an integer, integer depths"""
    t = np.zeros(n, abi.TRI_DTYPE)
    a = rng.integers(-20, 60, (n, 2)).astype(np.float32)
    lx, ly = 2.0 ** rng.integers(1, 4, n), 2.0 ** rng.integers(2, 4, n)
    b, c = a + np.stack([lx, 0 * lx], 1), a + np.stack([0 * ly, ly], 1)
    flip = rng.random(n) < 0.5
    t["pos"][:, 0, :2], t["pos"][:, 1, :2], t["pos"][:, 2, :2] = a, np.where(flip[:, None], c, b), np.where(flip[:, None], b, c)
    t["pos"][:, :, 2] = rng.integers(1, 4, (n, 3))
    t["nrm"] = [0, 0, -1]
    return t


@pytest.mark.parametrize("name", DYADIC)
def test_exact_on_dyadic_inputs(ctx, tmp_path, name):
    """triangles of power-of-two area and integer edges, alpha and beta multiples of 1/16, integer gradients: every term and every
    partial sum is representable, any order of adds gives the same bits"""
    w, h, n, tris, ids = dyadic_case(name)
    rng = np.random.default_rng([len(name), 17])
    frames = [frame(dyadic_tris(rng, tris), w, h) for _ in range(n)]
    fs = ctx.frameset(frames)
    al = rng.integers(0, 17, ids.shape)
    be = (rng.integers(0, 17, ids.shape) * (16 - al)) // 16
    hv = np.zeros((n, 4, h, w), np.float32)
    hv[:, 1], hv[:, 2], hv[:, 3] = ids.view(np.float32), al / 16.0, be / 16.0
    vis = torch.as_tensor(hv).cuda()
    v = hv.view(np.uint32)
    gb = rng.integers(-4, 5, (n, 2, h, w)).astype(np.float32)
    gz = rng.integers(-2, 3, (n, 1, h, w)).astype(np.float32)
    T = tris + 1
    for use_b, use_z in INPUTS:
        b, z = gb if use_b else None, gz if use_z else None
        gp, gx = call(fs, vis, b, z, T, fill=SENTINEL)
        accs, want_px = expect(tmp_path, frames, v, b, z, T, fill=SENTINEL)
        same(gx, want_px, name + " gpix")
        check_gpos(gp, accs, f"{name} gbary {use_b} gz {use_z}", exact=True)
        assert (gp != 0).any()
    fs.close()


# ------------------------------------------------------------------------------------------------------ not fused, hostile
def test_not_fused_hostile_ids_and_non_finite_values(ctx, tmp_path):
    """frames that do not clear; ids out of range and bare class bits written into the buffer; NaN at every nobody pixel of the
    gradient planes; NaN / inf gradients at owned pixels; accumulation into a gpos that is not zero"""
    t = soup(4, 40, 96, 80, ZS)
    frames = [frame(t, 96, 80, flags=0), frame(t, 96, 80, flags=0)]
    fs = ctx.frameset(frames)
    hv = visibility(fs).cpu().numpy()
    ids = hv[0, 1].view(np.uint32)
    ids[0, :16], ids[1, :16], ids[2, :16], ids[3, :16], ids[4, :16] = len(t) + 1, 0x7fffffff, 0xffffffff, (len(t) + 1) | 0x80000000, 0x80000000
    ids[5, :16] = 0
    vis = torch.as_tensor(hv).cuda()
    v = hv.view(np.uint32)
    own = owned(v, frames)
    assert (~own[0, :6, :16]).all() and (~own).sum() > 500 and own.sum() > 400
    T = len(t)
    gb, gz = rand_grads(4, fs, own)
    for fl, fused in ((F, True), (0, False)):
        gp, gx = call(fs, vis, gb, gz, T, flags=fl, fill=SENTINEL)
        accs, want_px = expect(tmp_path, frames, v, gb, gz, T, fused, SENTINEL)
        same(gx, want_px, f"fused {fused}")
        assert np.isfinite(gp).all() and not np.isnan(gx.view(np.float32)[:, 0][own]).any()
        check_gpos(gp, accs, f"fused {fused}")
        for p in (0, 1):
            assert (gx[:, p][~own] == (0 if fused else SENTINEL)).all() and (fused or (gx[:, p][own] != SENTINEL).all())
    # accumulation: a second call into the first one's result is twice one call (the bound of 2 n adds on twice the sums)
    gp2, _ = call(fs, vis, gb, gz, T, want_pix=False, into=gp)
    check_gpos(gp2, accs, "two calls", calls=2)
    assert (gp2 != gp).any()
    # non-finite gradients at owned pixels propagate as the reference has them, and to their owners only
    ys, xs = np.nonzero(own[1])
    for j, val in enumerate((np.nan, np.inf, -np.inf)):
        gb[1, 0][ys[j::11][:12], xs[j::11][:12]] = val
        gz[1, 0][ys[j + 5::11][:12], xs[j + 5::11][:12]] = val
    gp, gx = call(fs, vis, gb, gz, T, flags=0, fill=SENTINEL)
    accs, want_px = expect(tmp_path, frames, v, gb, gz, T, False, SENTINEL)
    same(gx, want_px, "non-finite gpix")
    check_gpos(gp, accs, "non-finite gpos")
    assert np.isnan(gp[1]).any() and np.isfinite(gp[0]).all() and np.isfinite(gp[1]).any()
    fs.close()


# ------------------------------------------------------------------------------------------------------ a sceneset
def test_sceneset_equals_the_frameset_of_its_stream(ctx, tmp_path):
    from srz import scenes as pscenes
    wl = pscenes.spot_bunny_1080p()
    wl.upload_meshes(ctx)
    frames = [wl.frame(3), wl.frame(4)]
    fs, ss = ctx.frameset(frames), ctx.frameset([wl.scene_frame(3), wl.scene_frame(4)])
    vis_f, vis_s = visibility(fs), visibility(ss)
    assert torch.equal(vis_f.view(torch.int32), vis_s.view(torch.int32))
    v = words(vis_f)
    T = max(f.n_tris for f in frames)
    gb, gz = rand_grads(8, fs, owned(v, frames))
    accs, want_px = expect(tmp_path, frames, v, gb, gz, T)
    for name, s, vis in (("frameset", fs, vis_f), ("sceneset", ss, vis_s)):
        gp, gx = call(s, vis, gb, gz, T)
        same(gx, want_px, name)
        check_gpos(gp, accs, name)
        assert (gx[0, 0] != 0).sum() > 10000 and (gp != 0).sum() > 10000
    fs.close(), ss.close()


# ------------------------------------------------------------------------------------------------------ sharded
def test_sharded_world_2(ctx, tmp_path):
    import srz
    w, h, tris = 64, 128, 50
    t = np.concatenate([soup(8, tris - 1, w, h, ZS, big=True), BACKDROP])
    frames = [frame(t, w, h), frame(t, w, h)]
    fs = ctx.frameset(frames)
    v = words(visibility(fs))
    gb, gz = rand_grads(6, fs, owned(v, frames))
    accs, want_px = expect(tmp_path, frames, v, gb, gz, tris)
    fs.close()
    total = np.zeros((2, tris, 3, 3), np.float64)
    for rank in (0, 1):
        c = srz.Context(0, rank, 2)
        sfs = c.frameset(frames)
        svis = visibility(sfs)
        rows = parallel.band_rows(h, rank, 2)
        assert len(rows) == 2
        sb, sz = np.full(sfs.interpolate_shape(2), np.nan, np.float32), np.full(sfs.interpolate_shape(1), np.nan, np.float32)
        for (lb, _, r0, r1) in rows:
            assert np.array_equal(words(svis)[:, :, lb * 32: lb * 32 + r1 - r0], v[:, :, r0:r1])
            sb[:, :, lb * 32: lb * 32 + r1 - r0], sz[:, :, lb * 32: lb * 32 + r1 - r0] = gb[:, :, r0:r1], gz[:, :, r0:r1]
        part, part_px = call(sfs, svis, sb, sz, tris)
        for (lb, _, r0, r1) in rows:
            same(part_px[:, :, lb * 32: lb * 32 + r1 - r0], want_px[:, :, r0:r1], f"gpix rank {rank} band {lb}")
        assert np.isfinite(part).all() and (part != 0).any()
        total += part
        sfs.close(), c.close()
    # (two float32 partial sums add exactly in float64; together they hold one rounding per contributing pixel)
    err = np.abs(total - np.stack([a.gpos for a in accs]))
    assert (err <= np.stack([a.bound() for a in accs])).all(), float(err.max())


# ------------------------------------------------------------------------------------------------------ cross-checks
def test_cross_checks_against_the_attribute_gradient(ctx, tmp_path):
    from srz.visibility import interpolate_bary_grad, position_grad
    frames = pair(100, 70, 120)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    T = frames[0].n_tris
    # ---- gz all ones: the z slots are the sums of w per corner, which interpolate_grad's gattr is for one channel of gout = 1
    ones = torch.ones(fs.interpolate_shape(1), dtype=torch.float32, device="cuda")
    gp = position_grad(fs, vis, gz=ones)
    assert gp.shape == (2, T, 3, 3)
    ga = torch.zeros((2, T, 3, 1), dtype=torch.float32, device="cuda")
    fs.interpolate_grad(vis.data_ptr(), ones.data_ptr(), None, 1, 2, T, ga.data_ptr(), None, F, stream())
    torch.cuda.synchronize()
    accs, _ = expect(tmp_path, frames, v, None, ones.cpu().numpy(), T)
    zb = np.stack([a.bound() for a in accs])[..., 2]
    iacc = [interpref.Grad((T, 3, 1)) for _ in frames]
    for i, f in enumerate(frames):
        interpref.grad(tmp_path, np.zeros((T, 3, 1), np.float32), f.n_tris, v[i], np.ones((1,) + v.shape[2:], np.float32), iacc[i], False)
    ib = np.stack([a.bound() for a in iacc])[..., 0]
    diff = np.abs(gp.cpu().numpy()[..., 2].astype(np.float64) - ga.cpu().numpy()[..., 0])
    assert (diff <= zb + ib).all() and (ga != 0).sum() > 100
    # ---- positions as three attribute channels, gout = (0, 0, gz): interpolate_bary_grad's planes are gz's share of dalpha, dbeta
    pos = torch.as_tensor(padded_positions(frames, T).reshape(2, T, 3, 3)).cuda()
    _, gz = rand_grads(3, fs)
    gout = torch.zeros(fs.interpolate_shape(3), dtype=torch.float32, device="cuda")
    gout[:, 2] = torch.as_tensor(gz[:, 0]).cuda()
    gbary = interpolate_bary_grad(fs, vis, pos, gout)
    via_b, px_b = position_grad(fs, vis, gbary=gbary, want_pix=True)
    via_z, px_z = position_grad(fs, vis, gz=torch.as_tensor(gz).cuda(), want_pix=True)
    same(px_b.cpu().numpy(), px_z.cpu().numpy(), "gpix through gbary and through gz")
    accs, _ = expect(tmp_path, frames, v, None, gz, T)
    xy = np.stack([a.bound() for a in accs])[..., :2]
    diff = np.abs(via_b.cpu().numpy()[..., :2].astype(np.float64) - via_z.cpu().numpy()[..., :2])
    assert (diff <= 2 * xy).all() and (via_b[..., 2] == 0).all() and (via_z[..., 2] != 0).any() and (via_b[..., :2] != 0).sum() > 100
    fs.close()


# ------------------------------------------------------------------------------------------------------ autograd
def test_autograd(ctx, tmp_path, monkeypatch):
    import srz
    from srz.visibility import depth, interpolate, interpolate_bary_grad, interpolate_geo, position_grad
    frames = pair(100, 70, 120)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    T = frames[0].n_tris
    calls = []
    for name in ("interpolate_grad", "position_grad"):
        real = getattr(srz.FrameSet, name)
        monkeypatch.setattr(srz.FrameSet, name, lambda self, *a, _real=real, _name=name, **k: (calls.append(_name), _real(self, *a, **k))[1])
    pos = torch.as_tensor(padded_positions(frames, T).reshape(2, T, 3, 3)).cuda().requires_grad_(True)
    attr = torch.as_tensor(np.random.default_rng(9).normal(0, 3, (T, 3, 6)).astype(np.float32)).cuda().requires_grad_(True)
    # ---- interpolate_geo: one interpolate_grad call for both gradients, one position_grad call
    out = interpolate_geo(fs, vis, attr, pos)
    assert out.shape == (2, 6, 70, 100) and out.requires_grad
    out.square().sum().backward()
    torch.cuda.synchronize()
    assert calls == ["interpolate_grad", "position_grad"]
    g = 2 * out.detach()
    gbary = interpolate_bary_grad(fs, vis, attr.detach(), g)
    two_calls = position_grad(fs, vis, gbary=gbary, pos_tris=T)
    accs, _ = expect(tmp_path, frames, v, gbary.cpu().numpy(), None, T)
    bound = np.stack([a.bound() for a in accs])
    ref = np.stack([a.gpos for a in accs])
    for got in (pos.grad, two_calls):
        assert (np.abs(got.cpu().numpy().astype(np.float64) - ref) <= bound).all()
    assert pos.grad.shape == pos.shape and (pos.grad[..., 2] == 0).all() and (pos.grad != 0).sum() > 100
    plain = attr.detach().clone().requires_grad_(True)
    interpolate(fs, vis, plain).square().sum().backward()
    iacc = interpref.Grad((T, 3, 6))
    for i, f in enumerate(frames):
        interpref.grad(tmp_path, attr.detach().cpu().numpy(), f.n_tris, v[i], g[i].cpu().numpy(), iacc, False)
    for got in (attr.grad, plain.grad):
        assert (np.abs(got.cpu().numpy().astype(np.float64) - iacc.gattr) <= iacc.bound()).all()
    # ---- only pos asks for a gradient: still one call each; nobody asks: none
    n = len(calls)
    pos2 = pos.detach().clone().requires_grad_(True)
    interpolate_geo(fs, vis, attr.detach(), pos2).square().sum().backward()
    assert calls[n:] == ["interpolate_grad", "position_grad"] and (np.abs(pos2.grad.cpu().numpy().astype(np.float64) - ref) <= bound).all()
    n = len(calls)
    assert not interpolate_geo(fs, vis, attr.detach(), pos.detach()).requires_grad and len(calls) == n
    # ---- depth: plane 0, backward through gz
    pos3 = pos.detach().clone().requires_grad_(True)
    z = depth(fs, vis, pos3)
    own = torch.as_tensor(owned(v, frames)).cuda()
    assert z.shape == (2, 1, 70, 100) and torch.equal(z[:, 0], vis[:, 0])
    wz = torch.as_tensor(np.random.default_rng(10).normal(0, 2, (2, 1, 70, 100)).astype(np.float32)).cuda()
    torch.where(own[:, None], z * wz, torch.zeros_like(z)).sum().backward()
    torch.cuda.synchronize()
    assert calls[n:] == ["position_grad"]
    gz = torch.where(own[:, None], wz, torch.zeros_like(wz))
    accs, _ = expect(tmp_path, frames, v, None, gz.cpu().numpy(), T)
    err = np.abs(pos3.grad.cpu().numpy().astype(np.float64) - np.stack([a.gpos for a in accs]))
    assert (err <= np.stack([a.bound() for a in accs])).all() and (pos3.grad[..., 2] != 0).sum() > 100
    fs.close()


# ------------------------------------------------------------------------------------------------------ misuse
def test_misuse(ctx):
    import srz
    L = srz.lib()
    t = soup(1, 60, 64, 64, ZS)
    fs = ctx.frameset([frame(t, 64, 64), frame(t[:50], 64, 64)])
    vis = visibility(fs)
    T = 60
    big = torch.full((2 * 4 * 64 * 64 + 2 * T * 9 + 64,), 5, dtype=torch.int32, device="cuda")  # outputs are carved from this
    gbary = torch.zeros(fs.interpolate_shape(2), dtype=torch.float32, device="cuda")
    gz = torch.zeros(fs.interpolate_shape(1), dtype=torch.float32, device="cuda")
    two, h, e = fs.interpolate_bytes(2), ctx.h, abi.SRZ_E_INVALID
    v, b, z, x = vis.data_ptr(), gbary.data_ptr(), gz.data_ptr(), big.data_ptr()
    p = x + two + 16  # gpos behind a gpix-sized first output
    assert two == 2 * 2 * 64 * 64 * 4

    def f(vis=v, gbary=b, gz=z, pt=T, gpos=p, gpix=x, flags=F, ctxh=h, fsh=fs.h):
        return L.srz_frameset_position_grad(ctxh, fsh, vis, gbary, gz, pt, gpos, gpix, flags, None)
    bad = [dict(ctxh=None), dict(fsh=None), dict(vis=None), dict(gbary=None, gz=None), dict(gpos=None, gpix=None), dict(pt=59), dict(pt=0),
           dict(vis=v + 4), dict(gbary=b + 4), dict(gz=z + 8), dict(gpix=x + 4), dict(gpos=p + 2), dict(gpix=v), dict(gpix=v + 64 * 64 * 4),
           dict(gpos=v + 32), dict(gpix=b), dict(gpos=b + 32), dict(gpix=z), dict(gpos=z + 32), dict(gpos=x + 32), dict(gpos=x + two - 4),
           dict(gbary=x + 16, gpos=None), dict(gz=p + 4 * 9 * T, gpix=None)]
    for flag in (abi.UNIFIED, abi.ORDERED_RASTER, abi.NO_Z_READBACK, 16, F | abi.UNIFIED):
        bad.append(dict(flags=flag))
    for kw in bad:
        assert f(**kw) == e, kw
    torch.cuda.synchronize()
    assert (big == 5).all() and (gbary == 0).all() and (gz == 0).all()
    assert f() == 0 and f(gbary=None) == 0 and f(gz=None) == 0 and f(gpos=None) == 0 and f(gpix=None) == 0 and f(pt=61) == 0 and f(flags=0) == 0
    torch.cuda.synchronize()
    fs.close()
