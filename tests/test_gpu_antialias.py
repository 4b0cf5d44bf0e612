"""-m gpu: silhouette antialiasing of a visibility buffer (srz_frameset_antialias / _antialias_grad, k_antialias / k_antialias_grad).
The visibility buffer is the GPU's own render_visibility, except where a test writes one by hand; the planes and their gradients are
seeded normals; the expected values are tests/antialiasref.py's on that buffer (pinned on the CPU by tests/test_antialias_ref.py).
out and gin: a NaN on one side must be a NaN on the other, every other word matches bit for bit.  gpos: within gamma_n * sum |term|,
gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing pairs — one rounding per add, the terms being float32 terms on
both sides: derived, not measured —, bit for bit where n = 1, exactly 0 where n = 0, exact where every partial sum is representable."""
import numpy as np
import pytest
import torch

import antialiasref as ref
import posgradref
from srz import abi
from support import ctx, filled, frame, padded_positions, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
OUTPUTS = ((True, False), (False, True), (True, True))  # (gin, gpos)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def forward(fs, vis, c):
    """one srz_frameset_antialias into a sentinel-filled buffer → uint32 words [n, C, rows, W]"""
    d = dev(c)
    out = filled(d.shape)
    fs.antialias(vis.data_ptr(), d.data_ptr(), d.shape[1], out.data_ptr(), fs.interpolate_bytes(d.shape[1]), F, stream())
    torch.cuda.synchronize()
    return words(out)


def backward(fs, vis, c, g, T, want_gin=True, want_gpos=True, into=None):
    """one srz_frameset_antialias_grad → (gin uint32 words from a sentinel fill, gpos float32 [n, T, 3, 3] added into `into` or zeros)"""
    d, dg = dev(c), dev(g)
    gin = filled(d.shape) if want_gin else None
    gp = (torch.zeros((fs.n_frames, T, 3, 3), dtype=torch.float32, device="cuda") if into is None else torch.as_tensor(into).cuda()) if want_gpos else None
    fs.antialias_grad(vis.data_ptr(), d.data_ptr(), dg.data_ptr(), d.shape[1], gin.data_ptr() if want_gin else None, T,
                      gp.data_ptr() if want_gpos else None, F, stream())
    torch.cuda.synchronize()
    return (words(gin) if want_gin else None), (gp.cpu().numpy() if want_gpos else None)


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def expect(tmp_path, frames, v, c, g, T, pos=None):
    """(out [n, C, rows, W], gin likewise, an antialiasref.Grad per frame)"""
    pos = padded_positions(frames, T) if pos is None else pos
    accs, out, gin = [ref.Grad(T) for _ in frames], [], []
    for i, f in enumerate(frames):
        out.append(ref.forward(tmp_path, pos[i], f.n_tris, v[i], c[i]))
        gin.append(ref.backward(tmp_path, pos[i], f.n_tris, v[i], c[i], g[i], accs[i]))
    return np.stack(out), np.stack(gin), accs


def check_gpos(got, accs, what, exact=False, calls=1):
    """finite elements: within the bound (0 when exact), bit for bit where n = 1, exactly 0 where n = 0; an element some term of which
    is not finite: NaN where the reference has NaN, the reference's infinity where it has one"""
    ref_ = calls * np.stack([a.gpos for a in accs])
    mag = np.stack([a.gabs for a in accs])
    bound = np.stack([a.bound(calls) for a in accs])
    cnt = np.stack([a.count for a in accs])
    assert got.shape == ref_.shape, (got.shape, ref_.shape)
    fin = np.isfinite(mag)
    assert np.isfinite(ref_[fin]).all()
    if exact:
        assert fin.all() and (ref_.astype(np.float32).astype(np.float64) == ref_).all(), "the case is not dyadic"
        bound = np.zeros_like(bound)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - ref_)
    ratio = err[fin & (bound > 0)] / bound[fin & (bound > 0)]
    print(f"{what}: max err {err[fin].max():.3e}, max err / bound {ratio.max() if ratio.size else 0:.3f}, max n {int(cnt.max())}")
    bad = fin & ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    assert np.array_equal(np.isnan(got[~fin]), np.isnan(ref_[~fin])), what + ": NaN elements"
    inf = ~fin & np.isinf(ref_)
    assert np.array_equal(got[inf].astype(np.float64), ref_[inf]), what + ": infinite elements"
    if calls == 1:
        one = fin & (cnt == 1)
        same((got + np.float32(0))[one], (ref_.astype(np.float32) + np.float32(0))[one], what + " (n = 1)")
    assert (got[cnt == 0] == 0).all(), what + ": an element without a contributing pair is not 0"


def planes(seed, fs, n_ch, sigma=1.0):
    rng = np.random.default_rng([seed, n_ch, 31])
    return (rng.normal(0, sigma, fs.interpolate_shape(n_ch)).astype(np.float32), rng.normal(0, sigma, fs.interpolate_shape(n_ch)).astype(np.float32))


def run_all(tmp_path, fs, frames, vis, v, T, n_chs, what, pos=None):
    """forward and every combination of the backward's outputs at each channel count, against the reference"""
    accs = None
    for n_ch in n_chs:
        c, g = planes(len(what), fs, n_ch)
        want_out, want_gin, accs = expect(tmp_path, frames, v, c, g, T, pos)
        same(forward(fs, vis, c), want_out, f"{what} C {n_ch} out")
        for want_i, want_p in OUTPUTS:
            gin, gp = backward(fs, vis, c, g, T, want_i, want_p)
            if want_i:
                same(gin, want_gin, f"{what} C {n_ch} gin (gpos {want_p})")
            if want_p:
                check_gpos(gp, accs, f"{what} C {n_ch} gpos (gin {want_i})")
                assert (gp[..., 2] == 0).all()
    return accs


# ------------------------------------------------------------------------------------------------------ sizes and channels
@pytest.mark.parametrize("backdrop", (True, False))
@pytest.mark.parametrize("w,h,n", ref.SIZES)
def test_sizes_channels_and_outputs(ctx, tmp_path, w, h, n, backdrop):
    """two frames of the scene tests/test_antialias_ref.py counts the pairs of; every out and gin word is written (the sentinel is
    no float the reference produces: `same` would see it)"""
    t = ref.scene_tris(w, h, n, backdrop)
    frames = [frame(t, w, h), frame(t, w, h)]
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    T = len(t) + 2
    accs = run_all(tmp_path, fs, frames, vis, v, T, (1, 3, 4, 5) + ((64,) if (w, h) == (64, 64) else ()), f"{w}x{h} backdrop {backdrop}")
    for a in accs:
        for name in ref.relied_on(w, h, backdrop):
            assert a.counters[name] > 0, (name, a.counters)
    fs.close()


def test_nine_frames_wrap_the_frame_deal(ctx, tmp_path):
    """nine frames; frames 4 and 5 have fewer triangles than pos_tris, and frame 5's buffer holds ids beyond its count, copied in
    from frame 0: nobody there — the frame deal and the guard of the position gather"""
    t = ref.scene_tris(64, 64, 60, False)
    frames = []
    for i in range(9):
        t2 = t.copy()
        t2["pos"][:, :, :2] += np.float32([1.5 * i, -1.0 * i])
        frames.append(frame(t2[:40] if i in (4, 5) else t2, 64, 64))
    fs = ctx.frameset(frames)
    hv = visibility(fs).cpu().numpy()
    hv[5] = hv[0]
    vis = torch.as_tensor(hv).cuda()
    v = hv.view(np.uint32)
    assert ((v[5, 1] & 0x7fffffff) > 40).sum() > 100
    T = len(t) + 1
    accs = run_all(tmp_path, fs, frames, vis, v, T, (3,), "nine frames")
    assert all(a.counters["target_n"] + a.counters["target_f"] > 0 for a in accs)
    fs.close()


# ------------------------------------------------------------------------------------------------------ hand-written buffers
def run_ids(rng, n, h, w, tris, max_run):
    """[n, h, w] id words: runs of 1 .. max_run pixels of one owner over the raster, either class, some pixels nobody's"""
    total = n * h * w
    lens = rng.integers(1, max_run + 1, total)
    owner = rng.integers(1, tris + 1, total).astype(np.uint32)
    ids = np.repeat(owner, lens)[:total]
    ids |= (rng.random(total) < 0.4).astype(np.uint32) << 31
    ids[rng.random(total) < 0.1] = 0
    return ids.reshape(n, h, w)


def id_case(name):
    """(w, h, frames, triangles, ids [n, h, w]): the id planes of tests/test_gpu_posgrad.py's cases of these names, restated"""
    rng = np.random.default_rng([len(name), 5])
    if name == "four owners in a quad":
        ys, xs = np.mgrid[0:64, 0:64]
        return 64, 64, 1, 37, (1 + (xs + 7 * ys) % 37).astype(np.uint32)[None]
    if name == "1024 owners in a tile":
        return 32, 32, 1, 1024, (rng.permutation(1024).astype(np.uint32) + 1).reshape(1, 32, 32)
    if name == "runs across quads and rows":
        return 96, 96, 2, 300, run_ids(rng, 2, 96, 96, 300, 13)
    if name == "partial tiles":
        return 50, 37, 2, 40, run_ids(rng, 2, 37, 50, 40, 9)
    raise KeyError(name)


def dyadic_tris(rng, n, w, h):
    """n right triangles with legs 2 .. 16 along the axes at quarter-pixel places inside the frame, either winding, integer depths"""
    t = np.zeros(n, abi.TRI_DTYPE)
    a = rng.integers(-8, 4 * max(w, h), (n, 2)).astype(np.float32) / 4
    lx, ly = 2.0 ** rng.integers(1, 5, n), 2.0 ** rng.integers(1, 5, n)
    b, c = a + np.stack([lx, 0 * lx], 1), a + np.stack([0 * ly, ly], 1)
    flip = rng.random(n) < 0.5
    t["pos"][:, 0, :2], t["pos"][:, 1, :2], t["pos"][:, 2, :2] = a, np.where(flip[:, None], c, b), np.where(flip[:, None], b, c)
    t["pos"][:, :, 2] = rng.integers(1, 4, (n, 3))
    t["nrm"] = [0, 0, -1]
    return t


@pytest.mark.parametrize("name", ("four owners in a quad", "1024 owners in a tile", "runs across quads and rows", "partial tiles"))
def test_hand_written_id_planes(ctx, tmp_path, name):
    """ids no rasteriser would write, over triangles that lie anywhere; z planes with ties, +-0, NaN and +inf; hostile ids —
    0x7fffffff, 0xffffffff, bare class bits, count + 1 — are nobody"""
    w, h, n, tris, ids = id_case(name)
    rng = np.random.default_rng([len(name), 17])
    frames = [frame(dyadic_tris(rng, tris, w, h), w, h) for _ in range(n)]
    fs = ctx.frameset(frames)
    ids = ids.copy()
    for r, word in enumerate((0x7fffffff, 0xffffffff, 0x80000000, tris + 1, (tris + 1) | 0x80000000)):
        ids[:, 3 + 2 * r, 5:21] = word
    hv = np.zeros((n, 4, h, w), np.float32)
    hv[:, 0] = rng.choice(np.float32([1, 2, 2, 3, 0.0, -0.0, np.nan, np.inf]), ids.shape)
    hv[:, 1] = ids.view(np.float32)
    vis = torch.as_tensor(hv).cuda()
    v = hv.view(np.uint32)
    accs = run_all(tmp_path, fs, frames, vis, v, tris + 1, (3,), name)
    assert sum(a.counters["differ"] for a in accs) > 500
    fs.close()


def test_exact_on_a_dyadic_edge(ctx, tmp_path):
    """one side at x = 20.25 from y = -64 to y = 192 across the 64 rows of a 64 x 64 frame, integer colours and gradients: k = (64 +
    y) / 256, every term a multiple of 2^-8 below 2^13: every partial sum is representable, gpos is the same in any order of adds"""
    t = np.zeros(1, abi.TRI_DTYPE)
    t["pos"][0] = [[20.25, -64, 5], [20.25, 192, 5], [-1000, 64, 5]]
    t["nrm"] = [0, 0, -1]
    frames = [frame(t, 64, 64)]
    fs = ctx.frameset(frames)
    hv = np.zeros((1, 4, 64, 64), np.float32)
    hv[0, 0] = np.inf
    hv[0, 0, :, :21], hv[0, 1, :, :21] = 5.0, np.uint32([1]).view(np.float32)[0]
    vis = torch.as_tensor(hv).cuda()
    v = hv.view(np.uint32)
    rng = np.random.default_rng(3)
    c = rng.integers(-8, 9, (1, 3, 64, 64)).astype(np.float32)
    g = rng.integers(-4, 5, (1, 3, 64, 64)).astype(np.float32)
    want_out, want_gin, accs = expect(tmp_path, frames, v, c, g, 1)
    same(forward(fs, vis, c), want_out, "dyadic out")
    gin, gp = backward(fs, vis, c, g, 1)
    same(gin, want_gin, "dyadic gin")
    check_gpos(gp, accs, "dyadic gpos", exact=True)
    assert accs[0].counters["target_n"] == 64 and (accs[0].count[0, :2, 0] == 64).all() and (gp[0, 0, :2, 0] != 0).all()
    fs.close()


def test_non_finite_inputs(ctx, tmp_path):
    """NaN and inf in the planes and in their gradient propagate to exactly the words and elements the reference names; non-finite
    positions blend nothing"""
    w, h = 64, 64
    t = ref.scene_tris(w, h, 60, False)
    frames = [frame(t, w, h), frame(t, w, h)]
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    T = len(t)
    c, g = planes(5, fs, 3)
    rng = np.random.default_rng(8)
    for j, val in enumerate((np.nan, np.inf, -np.inf)):
        ys, xs = rng.integers(0, h, 40), rng.integers(0, w, 40)
        c[1, j, ys, xs] = val
        ys, xs = rng.integers(0, h, 40), rng.integers(0, w, 40)
        g[1, (j + 1) % 3, ys, xs] = val
    want_out, want_gin, accs = expect(tmp_path, frames, v, c, g, T)
    same(forward(fs, vis, c), want_out, "non-finite out")
    gin, gp = backward(fs, vis, c, g, T)
    same(gin, want_gin, "non-finite gin")
    check_gpos(gp, accs, "non-finite gpos")
    assert np.isfinite(gp[0]).all() and np.isnan(gp[1]).any() and np.isfinite(gp[1]).any()
    assert np.isfinite(want_out[0]).all() and (~np.isfinite(want_out[1])).sum() > (~np.isfinite(c[1])).sum()
    fs.close()
    # positions that are not finite: ids written by hand over triangles whose every vertex holds a NaN or an infinity
    bad = t[:40].copy()
    bad["pos"][:, :, 0] = np.random.default_rng(9).choice(np.float32([np.nan, np.inf, -np.inf]), (40, 3))
    frames = [frame(bad, w, h)]
    fs = ctx.frameset(frames)
    hv = np.zeros((1, 4, h, w), np.float32)
    hv[0, 0] = np.random.default_rng(10).choice(np.float32([1, 2, 3]), (h, w))
    hv[0, 1] = run_ids(np.random.default_rng(11), 1, h, w, 40, 9)[0].view(np.float32)
    vis2 = torch.as_tensor(hv).cuda()
    c, g = planes(6, fs, 3)
    want_out, want_gin, accs = expect(tmp_path, frames, hv.view(np.uint32), c, g, 40)
    assert accs[0].counters["differ"] > 1000 and accs[0].counters["target_n"] + accs[0].counters["target_f"] == 0
    out = forward(fs, vis2, c)
    same(out, want_out, "non-finite positions out")
    same(out, c, "non-finite positions: out is in")
    gin, gp = backward(fs, vis2, c, g, 40)
    same(gin, g, "non-finite positions: gin is gout")
    assert (gp == 0).all()
    fs.close()


# ------------------------------------------------------------------------------------------------------ a mesh with shared edges
def test_mesh_with_shared_edges_frameset_and_sceneset(ctx, tmp_path):
    """spot and the bunny at 1080p: interior edges by the ten thousand (two triangles of a mesh share their vertices' bits, in the
    frame's stream and from the vertex stage alike) and a silhouette.  The counts are asserted here, on the GPU's buffer against the
    reference's counters: the CPU oracle's 1080p visibility buffer is too slow to make in the CPU suite."""
    from srz import scenes as pscenes
    wl = pscenes.spot_bunny_1080p()
    wl.upload_meshes(ctx)
    frames = [wl.frame(3), wl.frame(4)]
    fs, ss = ctx.frameset(frames), ctx.frameset([wl.scene_frame(3), wl.scene_frame(4)])
    vis_f, vis_s = visibility(fs), visibility(ss)
    assert torch.equal(vis_f.view(torch.int32), vis_s.view(torch.int32))
    v = words(vis_f)
    T = max(f.n_tris for f in frames)
    c, g = planes(8, fs, 3)
    want_out, want_gin, accs = expect(tmp_path, frames, v, c, g, T)
    for a in accs:
        print(a.counters)
        assert a.counters["target_n"] + a.counters["target_f"] > 1000 and a.counters["interior"] > 10000
    for name, s, vis in (("frameset", fs, vis_f), ("sceneset", ss, vis_s)):
        same(forward(s, vis, c), want_out, name + " out")
        gin, gp = backward(s, vis, c, g, T)
        same(gin, want_gin, name + " gin")
        check_gpos(gp, accs, name + " gpos")
        assert (gp != 0).sum() > 1000
    fs.close(), ss.close()


# ------------------------------------------------------------------------------------------------------ cross-checks
def test_cross_checks(ctx, tmp_path):
    w, h = 100, 70
    t = ref.scene_tris(w, h, 120, False)
    frames = [frame(t, w, h), frame(t, w, h)]
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    T = len(t)
    # ---- a constant image is a fixed point, and no position receives a gradient
    const = np.full(fs.interpolate_shape(3), 0.3, np.float32)
    _, g = planes(2, fs, 3)
    same(forward(fs, vis, const), const, "constant image")
    _, gp = backward(fs, vis, const, g, T, want_gin=False)
    assert (gp == 0).all()
    # ---- a render's own four planes as one n_ch = 4 call (z is blended too) equal four one-channel calls
    col = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render(col.data_ptr(), fs.out_bytes, F, stream())
    torch.cuda.synchronize()
    hc = col.cpu().numpy()
    four = forward(fs, vis, hc)
    for p in range(4):
        same(four[:, p:p + 1], forward(fs, vis, hc[:, p:p + 1]), f"plane {p} alone")
    assert (four != words(col)).sum() > 100
    # ---- two calls into one gpos: the bound of 2 n adds on twice the sums
    c, g = planes(3, fs, 3)
    _, _, accs = expect(tmp_path, frames, v, c, g, T)
    _, gp1 = backward(fs, vis, c, g, T, want_gin=False)
    _, gp2 = backward(fs, vis, c, g, T, want_gin=False, into=gp1)
    check_gpos(gp2, accs, "two calls", calls=2)
    assert (gp2 != gp1).any()
    fs.close()


# ------------------------------------------------------------------------------------------------------ autograd
def test_autograd(ctx, tmp_path, monkeypatch):
    """color = interpolate_geo(...), antialias(fs, vis, color, pos), a squared loss: pos.grad is the interior term (position_grad of
    the gbary planes of gin) plus the silhouette term (antialias_grad's gpos), each within its own bound — and one float32 add of the
    two, which autograd makes when it accumulates them: half an ulp of the sum more."""
    import srz
    from srz.visibility import antialias, antialias_grad, interpolate_bary_grad, interpolate_geo, position_grad
    w, h = 100, 70
    t = ref.scene_tris(w, h, 120, False)
    frames = [frame(t, w, h), frame(t, w, h)]
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    T = len(t)
    calls = []
    real = srz.FrameSet.antialias_grad
    monkeypatch.setattr(srz.FrameSet, "antialias_grad", lambda self, *a, **k: (calls.append("antialias_grad"), real(self, *a, **k))[1])
    pos = torch.as_tensor(padded_positions(frames, T).reshape(2, T, 3, 3)).cuda().requires_grad_(True)
    attr = torch.as_tensor(np.random.default_rng(9).normal(0, 1, (T, 3, 3)).astype(np.float32)).cuda().requires_grad_(True)
    color = interpolate_geo(fs, vis, attr, pos)
    out = antialias(fs, vis, color, pos)
    assert out.shape == color.shape and out.requires_grad
    out.square().sum().backward()
    torch.cuda.synchronize()
    assert calls == ["antialias_grad"]
    hc, hg = color.detach().cpu().numpy(), 2 * out.detach().cpu().numpy()
    want_out, want_gin, accs = expect(tmp_path, frames, v, hc, hg, T)
    same(out.detach().cpu().numpy(), want_out, "autograd forward")
    gin, gsil = antialias_grad(fs, vis, color.detach(), 2 * out.detach(), pos_tris=T)
    same(gin.cpu().numpy(), want_gin, "plain gin")
    check_gpos(gsil.cpu().numpy(), accs, "plain silhouette term")
    gbary = interpolate_bary_grad(fs, vis, attr.detach(), gin)
    gint = position_grad(fs, vis, gbary=gbary, pos_tris=T)
    iacc = [posgradref.Grad(T) for _ in frames]
    hb = gbary.cpu().numpy()
    for i, f in enumerate(frames):
        posgradref.grad(tmp_path, padded_positions(frames, T)[i], f.n_tris, v[i], hb[i], None, iacc[i], False)
    total = np.stack([a.gpos for a in accs]) + np.stack([a.gpos for a in iacc])
    bound = np.stack([a.bound() for a in accs]) + np.stack([a.bound() for a in iacc])
    assert (np.abs(gint.cpu().numpy().astype(np.float64) - np.stack([a.gpos for a in iacc])) <= np.stack([a.bound() for a in iacc])).all()
    err = np.abs(pos.grad.cpu().numpy().astype(np.float64) - total)
    assert (err <= bound + 2.0 ** -24 * (np.abs(total) + bound)).all(), float((err - bound).max())
    assert (pos.grad[..., 2] == 0).all() and (gsil != 0).sum() > 100 and (gint != 0).sum() > 100
    # ---- only the colour needs a gradient: one call; only pos: one call; neither: none
    n = len(calls)
    c2 = color.detach().clone().requires_grad_(True)
    antialias(fs, vis, c2).square().sum().backward()
    assert calls[n:] == ["antialias_grad"]
    same(c2.grad.cpu().numpy(), want_gin, "gin through autograd")
    n = len(calls)
    p2 = pos.detach().clone().requires_grad_(True)
    antialias(fs, vis, color.detach(), p2).square().sum().backward()
    assert calls[n:] == ["antialias_grad"]
    check_gpos(p2.grad.cpu().numpy(), accs, "silhouette term through autograd")
    n = len(calls)
    assert not antialias(fs, vis, color.detach(), pos.detach()).requires_grad and len(calls) == n
    fs.close()


# ------------------------------------------------------------------------------------------------------ misuse
def test_misuse(ctx):
    import srz
    L = srz.lib()
    t = ref.scene_tris(64, 64, 58, False)  # 60 triangles
    fs = ctx.frameset([frame(t, 64, 64), frame(t[:50], 64, 64)])
    vis = visibility(fs)
    T, C = 60, 3
    nb = fs.interpolate_bytes(C)
    assert nb == 2 * C * 64 * 64 * 4
    big = torch.full((nb // 4 + 2 * T * 9 + 64,), 5, dtype=torch.int32, device="cuda")  # the outputs are carved from this
    cin = torch.zeros(fs.interpolate_shape(C), dtype=torch.float32, device="cuda")
    gout = torch.zeros(fs.interpolate_shape(C), dtype=torch.float32, device="cuda")
    h, e = ctx.h, abi.SRZ_E_INVALID
    v, i, g, x = vis.data_ptr(), cin.data_ptr(), gout.data_ptr(), big.data_ptr()
    p = x + nb + 16  # gpos behind a gin-sized first output

    def fwd(vis=v, cin=i, n_ch=C, out=x, ob=nb, flags=F, ctxh=h, fsh=fs.h):
        return L.srz_frameset_antialias(ctxh, fsh, vis, cin, n_ch, out, ob, flags, None)

    def bwd(vis=v, cin=i, gout=g, n_ch=C, gin=x, pt=T, gpos=p, flags=F, ctxh=h, fsh=fs.h):
        return L.srz_frameset_antialias_grad(ctxh, fsh, vis, cin, gout, n_ch, gin, pt, gpos, flags, None)
    flags = [dict(flags=fl) for fl in (abi.UNIFIED, abi.ORDERED_RASTER, abi.NO_Z_READBACK, 16, F | abi.UNIFIED)]
    for kw in [dict(ctxh=None), dict(fsh=None), dict(vis=None), dict(cin=None), dict(out=None), dict(n_ch=0), dict(n_ch=65), dict(ob=nb - 1),
               dict(ob=0), dict(vis=v + 4), dict(cin=i + 8), dict(out=x + 4), dict(out=v), dict(out=v + 64), dict(out=i), dict(out=i + nb - 16),
               dict(cin=x + 16)] + flags:
        assert fwd(**kw) == e, kw
    for kw in [dict(ctxh=None), dict(fsh=None), dict(vis=None), dict(cin=None), dict(gout=None), dict(gin=None, gpos=None), dict(n_ch=0),
               dict(n_ch=65), dict(pt=59), dict(pt=0), dict(vis=v + 4), dict(cin=i + 4), dict(gout=g + 8), dict(gin=x + 4), dict(gpos=p + 2),
               dict(gin=v), dict(gpos=v + 32), dict(gin=i), dict(gpos=i + 32), dict(gin=g), dict(gpos=g + 32), dict(gpos=x + 32),
               dict(gpos=x + nb - 4), dict(gout=x + 16, gpos=None), dict(cin=p + 4 * 9 * T, gin=None)] + flags:
        assert bwd(**kw) == e, kw
    # a sharded context: a vertical pair across a band edge needs another rank's rows
    c2 = srz.Context(0, 0, 2)
    sfs = c2.frameset([frame(t, 64, 64)])
    svis = visibility(sfs)
    sb = sfs.interpolate_bytes(C)
    assert L.srz_frameset_antialias(c2.h, sfs.h, svis.data_ptr(), i, C, x, sb, F, None) == e
    assert L.srz_frameset_antialias_grad(c2.h, sfs.h, svis.data_ptr(), i, g, C, x, T, p, F, None) == e
    sfs.close(), c2.close()
    torch.cuda.synchronize()
    assert (big == 5).all() and (cin == 0).all() and (gout == 0).all()
    assert fwd() == 0 and fwd(flags=0) == 0 and fwd(n_ch=1) == 0 and fwd(ob=nb + 64) == 0
    assert bwd() == 0 and bwd(gin=None) == 0 and bwd(gpos=None) == 0 and bwd(pt=61) == 0 and bwd(flags=0) == 0 and bwd(gpos=None, pt=0) == 0
    torch.cuda.synchronize()
    fs.close()
