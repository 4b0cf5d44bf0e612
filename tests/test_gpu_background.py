"""-m gpu: the environment behind a visibility buffer, by view ray, and its gradients (srz_frameset_background / _background_grad,
k_background, k_background_grad<false / true>, k_light_fold).  The visibility buffer is the GPU's own render_visibility, except where a
test writes one by hand; the expected values are tests/backgroundref.py's on that very buffer (pinned on the CPU by
tests/test_background_ref.py).  Forward and gray: a NaN on one side must be a NaN on the other, every other word matches bit for bit.
gtex: exact where an element has one contributing add and in the dyadic case, else within Grad.bound — gamma_n * sum |w g|, gamma_n
= n u / (1 - n u), u = 2^-24, n the element's contributing adds: one rounding per add, the products being float32 products on both
sides: derived, not measured."""
import numpy as np
import pytest
import torch

import backgroundref as br
import cuberef
from srz import abi
from support import SENTINEL, ccw, ctx, filled, frame, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
SIZES = [(64, 64, 30), (100, 70, 40), (50, 37, 14), (33, 1, 3), (1, 1, 1)]
CUBE_N = (1, 2, 3, 8)
CHANNELS = (1, 3, 5, 17, 64)
TG_SLOTS = 2048  # the capacity of the table of distinct texels per tile


def n_tris(f):
    return sum(len(t) for t in f.tris)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def dims(cube, ray):
    return (cube.shape[0] if cube.ndim == 5 else 1), cube.shape[-2], cube.shape[-1], ray.reshape(-1, 9).shape[0]


def fwd(fs, vis, ray, cube, where=br.NOBODY, flags=F, fill=SENTINEL):
    """the forward pass into a buffer prefilled with the word `fill` → uint32 [n, C, rows, W]; vis None: a NULL d_vis"""
    tf, N, C, rf = dims(cube, ray)
    out, t, r = filled(fs.interpolate_shape(C), fill), dev(cube), dev(ray)
    fs.background(vis.data_ptr() if vis is not None else None, r.data_ptr(), rf, t.data_ptr(), N, C, tf, where, out.data_ptr(),
                  fs.interpolate_bytes(C), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def bwd(fs, vis, ray, gout, cube, where=br.NOBODY, want_tex=True, want_ray=True, flags=F, into=None):
    """the backward pass → (gtex float32 of the cube's shape, added into `into` or zeros; gray uint32 [ray frames, 9] from SENTINEL)"""
    tf, N, C, rf = dims(cube, ray)
    t, g, r = dev(cube), dev(gout), dev(ray)
    assert tuple(g.shape) == tuple(fs.interpolate_shape(C))
    gt = (torch.zeros_like(t) if into is None else dev(into)) if want_tex else None
    gr = filled((rf, 9)) if want_ray else None
    wb = fs.background_work_bytes() if want_ray else 0
    work = filled((wb // 4 + 1,)) if want_ray else None
    fs.background_grad(vis.data_ptr() if vis is not None else None, r.data_ptr(), rf, g.data_ptr(), t.data_ptr(), N, C, tf, where,
                       gt.data_ptr() if want_tex else None, gr.data_ptr() if want_ray else None, work.data_ptr() if want_ray else None, wb,
                       flags, stream())
    torch.cuda.synchronize()
    return (gt.cpu().numpy() if want_tex else None), (words(gr) if want_ray else None)


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def of(t, i, nd):
    return t[i] if t.ndim == nd + 1 else t


def expect_fwd(tmp_path, frames, v, ray, cube, where=br.NOBODY, fused=True, fill=SENTINEL):
    """v: the visibility buffer's words [n, 4, rows, W], or None (ALL)"""
    out = []
    for i, f in enumerate(frames):
        shape = (f.height, f.width)
        pre = np.full((cube.shape[-1],) + shape, fill, np.uint32)
        out.append(br.forward(tmp_path, of(cube, i, 4), n_tris(f), None if v is None else v[i, 1], of(ray.reshape(-1, 9), i, 1) if ray.size > 9
                              else ray.reshape(9), where, fused, pre, shape=shape))
    return np.stack(out)


def expect_bwd(tmp_path, frames, v, ray, gout, cube, where=br.NOBODY):
    """(Grad per cube frame — one for a shared cube; every Grad's .rows are in frame order —, gray [ray frames, 9] float32)"""
    shared = cube.ndim == 4
    accs = [br.Grad(cube.shape[-4:]) for _ in range(1 if shared else len(frames))]
    rows = []
    for i, f in enumerate(frames):
        r = ray.reshape(-1, 9)[i if ray.size > 9 else 0]
        rows.append(br.grad(tmp_path, of(cube, i, 4), n_tris(f), None if v is None else v[i, 1], r, gout[i], accs[0 if shared else i], where,
                            shape=(f.height, f.width))[0])
    rows = np.stack(rows)
    return accs, (rows if ray.size > 9 else br.fold(tmp_path, rows)[None])


def check_gtex(got, accs, what, exact=False):
    ref = np.stack([a.gtex for a in accs]).reshape(got.shape)
    bound = np.stack([a.bound() for a in accs]).reshape(got.shape)
    cnt = np.stack([np.broadcast_to(a.count[..., None], a.gtex.shape) for a in accs]).reshape(got.shape)
    if exact:
        assert (ref.astype(np.float32).astype(np.float64) == ref).all(), "the case is not dyadic"
        bound = np.zeros_like(bound)
    finite = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    err = np.abs(got.astype(np.float64)[finite] - ref[finite])
    b = bound[finite]
    print(f"{what}: max err {err.max() if err.size else 0:.3e}, max err / bound {np.max(err[b > 0] / b[b > 0]) if (b > 0).any() else 0:.3f}, "
          f"max n {int(cnt.max())}, elements with one add {int((cnt == 1).sum())}, untouched {int((cnt == 0).sum())}")
    assert (err <= b).all(), f"{what}: {int((err > b).sum())} elements beyond the bound"
    one = cnt == 1
    same((got + np.float32(0))[one], (ref.astype(np.float32) + np.float32(0))[one], what + " (n = 1)")
    assert (got[cnt == 0] == 0).all()


def pair(w, h, n, flags=F, k=2):
    """k frames of a soup that leaves holes (no backdrop): owned and nobody's pixels both"""
    return [frame(soup(1 + i, n, w, h, ZS, big=w < 40), w, h, flags=flags) for i in range(k)]


def rand_gout(seed, shape, mask=None):
    g = np.random.default_rng([seed, 8]).normal(0, 2, shape).astype(np.float32)
    if mask is not None:
        g[np.broadcast_to(~mask[:, None], g.shape)] = np.nan  # the words outside the pass may hold anything
    return g


def owners(v, frames):
    return np.stack([((v[i, 1] & 0x7fffffff) - np.uint32(1)) < n_tris(f) for i, f in enumerate(frames)])


def hand_vis(ids):
    v = np.zeros((ids.shape[0], 4) + ids.shape[1:], np.float32)
    v[:, 1] = ids.view(np.float32)
    return v


# ------------------------------------------------------------------------------------------------------ sizes, channels, sharing, where
@pytest.mark.parametrize("w,h,n", SIZES)
def test_sizes_channels_sharing_and_where(ctx, tmp_path, w, h, n):
    """every frame size with every cube size and channel count in turn, cubes and blocks shared and per frame, nobody's pixels and all
    of them (with the buffer and with a NULL d_vis), both backward builds"""
    frames = pair(w, h, n)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    own = owners(v, frames)
    assert w * h == 1 or (own.any() and (~own).any())
    rays = np.stack([br.camera_block(w, h, 1, 1.6), br.camera_block(w, h, 2, 1.2)])
    k = 0
    for N in CUBE_N:
        for C in CHANNELS:
            k += 1
            if (k + w) % 3 and (N, C) != (8, 64):  # a third of the grid per size, the widest always
                continue
            cube = cuberef.make_cube(k, N, C, frames=2)
            cube = cube if k % 2 else cube[0]
            ray = rays if (k // 2) % 2 else rays[0]
            for where, vv, mask in ((br.NOBODY, v, ~own), (br.ALL, v, None), (br.ALL, None, None)):
                what = f"{w}x{h} N {N} C {C} cube {cube.ndim} ray {ray.ndim} where {where} vis {vv is not None}"
                got = fwd(fs, vis if vv is not None else None, ray, cube, where)
                same(got, expect_fwd(tmp_path, frames, vv, ray, cube, where), what)
                if where == br.NOBODY:
                    assert (got[np.broadcast_to(own[:, None], got.shape)] == 0).all()
                gout = rand_gout(k, got.shape, mask)
                gt, gr = bwd(fs, vis if vv is not None else None, ray, gout, cube, where)
                accs, want = expect_bwd(tmp_path, frames, vv, ray, gout, cube, where)
                same(gr, want, what + " gray")
                check_gtex(gt, accs, what + " gtex")
                only_gt = bwd(fs, vis if vv is not None else None, ray, gout, cube, where, want_ray=False)[0]
                check_gtex(only_gt, accs, what + " gtex alone")
                only_gr = bwd(fs, vis if vv is not None else None, ray, gout, cube, where, want_tex=False)[1]
                assert np.array_equal(only_gr, gr), what  # the same words whatever else is asked for
    fs.close()


@pytest.mark.parametrize("fused_frame,fused_call", [(0, 0), (0, F), (F, 0)])
def test_owned_words_stay_or_are_zero(ctx, tmp_path, fused_frame, fused_call):
    """from the sentinel: without SRZ_FUSED_CLEAR (in the frame's flags or the call's) the owned words are untouched, with it they are
    0; the words at the pass's pixels are written either way; SRZ_BG_ALL writes every word"""
    w, h = 100, 70
    frames = pair(w, h, 40, flags=fused_frame)
    fs = ctx.frameset(frames)
    vis = visibility(fs, F)
    v = words(vis)
    own = owners(v, frames)
    cube, ray = cuberef.make_cube(3, 8, 5), br.camera_block(w, h, 5, 1.6)
    fused = bool(fused_frame | fused_call)
    got = fwd(fs, vis, ray, cube, br.NOBODY, fused_call)
    same(got, expect_fwd(tmp_path, frames, v, ray, cube, br.NOBODY, fused), "nobody")
    m = np.broadcast_to(own[:, None], got.shape)
    assert (got[m] == (0 if fused else SENTINEL)).all() and (got[~m] != SENTINEL).all()
    full = fwd(fs, None, ray, cube, br.ALL, fused_call)
    same(full, expect_fwd(tmp_path, frames, None, ray, cube, br.ALL, fused), "all")
    assert (full != SENTINEL).all() and np.array_equal(full[~m], got[~m])
    # a frame nobody owns a pixel of, and one that is owned everywhere (a tile with nothing to do)
    ids = np.zeros((2, h, w), np.uint32)
    ids[1] = 1
    hv = hand_vis(ids)
    got = fwd(fs, torch.as_tensor(hv).cuda(), ray, cube, br.NOBODY, fused_call)
    same(got, expect_fwd(tmp_path, frames, hv.view(np.uint32), ray, cube, br.NOBODY, fused), "empty and full frames")
    assert np.array_equal(got[0], full[0]) and (got[1] == (0 if fused else SENTINEL)).all()
    fs.close()


# ------------------------------------------------------------------------------------------------------ the table's capacity
def test_a_tile_over_more_texels_than_the_table_holds(ctx, tmp_path):
    """N = 256 and a block that steps 2.5 texels per pixel: every 32 x 32 tile touches 4096 distinct texels, twice TG_SLOTS, so corners
    without a slot add straight to memory; every element still has its adds"""
    w = h = 64
    N, C = 256, 5
    frames = [frame(soup(2, 3, w, h, ZS), w, h)]
    fs = ctx.frameset(frames)
    ray = br.sweep_block(2.5, N)
    cls, _, at = br.classify(tmp_path, N, 0, None, ray, br.ALL, shape=(h, w))
    for ty in (0, 32):
        for tx in (0, 32):
            assert ((cls[ty:ty + 32, tx:tx + 32] & br.SAMPLED) != 0).all() and len(np.unique(at[ty:ty + 32, tx:tx + 32])) > TG_SLOTS
    cube = cuberef.make_cube(7, N, C)
    same(fwd(fs, None, ray, cube, br.ALL), expect_fwd(tmp_path, frames, None, ray, cube, br.ALL), "sweep")
    gout = rand_gout(3, (1, C, h, w))
    gt, gr = bwd(fs, None, ray, gout, cube, br.ALL)
    accs, want = expect_bwd(tmp_path, frames, None, ray, gout, cube, br.ALL)
    same(gr, want, "sweep gray")
    check_gtex(gt, accs, "sweep gtex")
    check_gtex(bwd(fs, None, ray, gout, cube, br.ALL, want_ray=False)[0], accs, "sweep gtex alone")
    fs.close()


def test_rays_across_every_edge_and_the_vertices(ctx, tmp_path):
    """eight frames, each block looking at one cube vertex: the rays cross every edge from both of its faces and every vertex region"""
    w = h = 64
    N, C = 8, 3
    frames = pair(w, h, 30, k=8)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    rays = np.stack([br.vertex_block(w, h, c) for c in br.CORNERS])
    sides, vertex = set(), 0
    for i, f in enumerate(frames):
        cls, face, at = br.classify(tmp_path, N, n_tris(f), v[i, 1], rays[i])
        s = (cls & br.SAMPLED) != 0
        vertex += int(((cls & br.VERTEX) != 0).sum())
        sides |= {(int(a), int(b)) for a, four in zip(face[s], at[s] // (N * N)) for b in four if b != a}
    assert len(sides) == 24 and vertex >= 16
    for cube in (cuberef.make_cube(9, N, C), cuberef.make_cube(9, N, C, frames=8)):
        same(fwd(fs, vis, rays, cube), expect_fwd(tmp_path, frames, v, rays, cube), "edges")
        gout = rand_gout(4, (8, C, h, w), ~owners(v, frames))
        gt, gr = bwd(fs, vis, rays, gout, cube)
        accs, want = expect_bwd(tmp_path, frames, v, rays, gout, cube)
        same(gr, want, "edges gray")
        check_gtex(gt, accs, "edges gtex")
    fs.close()


# ------------------------------------------------------------------------------------------------------ values
def test_non_finite_and_zero_rays_are_unsampled(ctx, tmp_path):
    w, h, C = 50, 37, 3
    frames = pair(w, h, 14, k=6)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    good = br.camera_block(w, h, 1, 1.6)
    rays = np.stack([np.zeros(9, np.float32), np.float32([np.nan, 0, 1, 0, 0, 0, 0, 0, 0]), np.float32([1, 1, 1, np.inf, 0, 0, 0, 0, 0]),
                     np.float32([1, 1, 1, 0, 0, 0, 0, -np.inf, 0]), np.float32([-20, -10, 0, 1, 0, 0, 0, 1, 0]), good])
    cube = cuberef.make_cube(1, 5, C)
    got = fwd(fs, vis, rays, cube)
    same(got, expect_fwd(tmp_path, frames, v, rays, cube), "unsampled")
    assert (got[:4] == 0).all() and (got[4][:, 10, 20] == 0).all()  # d = (x - 20, y - 10, 0) is zero at (20, 10), whoever owns it
    gout = rand_gout(5, (6, C, h, w))
    gt, gr = bwd(fs, vis, rays, gout, cube)
    accs, want = expect_bwd(tmp_path, frames, v, rays, gout, cube)
    same(gr, want, "unsampled gray")
    assert (gr[:4] == 0).all() and (gr[5] != 0).any()
    check_gtex(gt, accs, "unsampled gtex")
    fs.close()


def test_nan_and_inf_texels_propagate(ctx, tmp_path):
    w, h, N, C = 64, 64, 8, 3
    frames = pair(w, h, 30)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    cube = cuberef.make_cube(2, N, C)
    rng = np.random.default_rng(6)
    hit = rng.random(cube.shape) < 0.02
    cube[hit] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), int(hit.sum()))
    ray = br.camera_block(w, h, 3, 1.6)
    got = fwd(fs, vis, ray, cube)
    same(got, expect_fwd(tmp_path, frames, v, ray, cube), "non-finite texels")
    assert np.isnan(got.view(np.float32)).any()
    gout = rand_gout(6, got.shape, ~owners(v, frames))
    gt, gr = bwd(fs, vis, ray, gout, cube)
    accs, want = expect_bwd(tmp_path, frames, v, ray, gout, cube)
    same(gr, want, "non-finite texels gray")
    check_gtex(gt, accs, "non-finite texels gtex")  # (the weights do not read the texels: gtex is finite)
    gnan = gout.copy()
    gnan[0, 1, 5:9, 7:30] = np.inf
    gt, gr = bwd(fs, vis, ray, gnan, cube)
    accs, want = expect_bwd(tmp_path, frames, v, ray, gnan, cube)
    same(gr, want, "non-finite gout gray")
    fs.close()


# ------------------------------------------------------------------------------------------------------ gray's tree, gtex exactly
def test_gray_is_reproducible_and_one_pixel_gives_its_term(ctx, tmp_path):
    w, h, N, C = 100, 70, 8, 5
    frames = pair(w, h, 40, k=3)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    cube = cuberef.make_cube(4, N, C)
    gout = rand_gout(7, (3, C, h, w))
    for ray in (br.camera_block(w, h, 4, 1.6), np.stack([br.camera_block(w, h, s, 1.6) for s in (5, 6, 7)])):
        a, b = bwd(fs, vis, ray, gout, cube, want_tex=False)[1], bwd(fs, vis, ray, gout, cube)[1]
        assert np.array_equal(a, b)
        same(a, expect_bwd(tmp_path, frames, v, ray, gout, cube)[1], "two launches")
    # one pixel of the pass in all: a hand-written buffer owned everywhere but at (41, 67) of frame 1
    ids = np.ones((3, h, w), np.uint32)
    ids[1, 41, 67] = 0
    hv = hand_vis(ids)
    ray = br.camera_block(w, h, 4, 1.6)
    gr = bwd(fs, torch.as_tensor(hv).cuda(), ray, gout, cube, want_tex=False)[1]
    acc = br.Grad(cube.shape)
    _, term, smp = br.grad(tmp_path, cube, n_tris(frames[1]), ids[1], ray, gout[1], acc)
    assert smp.sum() == 1 and smp[41, 67]
    same(gr, (term[:, 41, 67] + np.float32(0))[None], "one pixel")
    per = bwd(fs, torch.as_tensor(hv).cuda(), np.stack([ray] * 3), gout, cube, want_tex=False)[1].view(np.float32)
    assert (per[0] == 0).all() and (per[2] == 0).all() and np.array_equal(per[1], gr.view(np.float32)[0])
    fs.close()


def test_gtex_exact_on_dyadic_inputs(ctx, tmp_path):
    """N = 8, rays (x / 16 - 15 / 16, 15 / 16 - y / 16, 1) over 31 x 31 pixels: s, t, the fractions (multiples of 1 / 4) and the weights
    (of 1 / 16) are exact, gout small integers: every partial sum is representable, whatever the order of the adds"""
    w = h = 31
    N, C = 8, 4
    frames = [frame(soup(3, 4, w, h, ZS), w, h) for _ in range(9)]  # nine frames: the walk's other branch, a table handed on
    fs = ctx.frameset(frames)
    ray = np.float32([-15 / 16, 15 / 16, 1, 1 / 16, 0, 0, 0, -1 / 16, 0])
    gout = np.random.default_rng(8).integers(-8, 9, (9, C, h, w)).astype(np.float32)
    for cube in (cuberef.make_cube(5, N, C), cuberef.make_cube(5, N, C, frames=9)):
        for want_ray in (True, False):
            gt, _ = bwd(fs, None, ray, gout, cube, br.ALL, want_ray=want_ray)
            accs, _ = expect_bwd(tmp_path, frames, None, ray, gout, cube, br.ALL)
            assert max(int(a.count.max()) for a in accs) >= 16
            check_gtex(gt, accs, f"dyadic {cube.ndim} {want_ray}", exact=True)
    fs.close()


def test_gtex_adds_into_what_the_buffer_holds(ctx, tmp_path):
    w, h, N, C = 64, 64, 8, 3
    frames = pair(w, h, 30)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    cube, ray = cuberef.make_cube(6, N, C), br.camera_block(w, h, 8, 1.6)
    gout = rand_gout(9, (2, C, h, w), ~owners(v, frames))
    init = np.random.default_rng(10).integers(-4, 5, cube.shape).astype(np.float32)
    gt, _ = bwd(fs, vis, ray, gout, cube, into=init)
    accs, _ = expect_bwd(tmp_path, frames, v, ray, gout, cube)
    a = accs[0]
    err = np.abs(gt.astype(np.float64) - (a.gtex + init))
    n = (a.count.astype(np.float64)[..., None] + 1) * 2.0 ** -24
    assert (err <= n / (1 - n) * (a.gabs + np.abs(init))).all()  # Grad.bound with one more term: what the buffer held
    assert np.array_equal(gt[a.count == 0], init[a.count == 0])
    fs.close()
