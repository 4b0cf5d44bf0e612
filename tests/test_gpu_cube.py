"""-m gpu: a cube map looked up by direction over a visibility buffer and its gradients (srz_frameset_texture_cube /
_texture_cube_grad, k_cube, k_cube_grad).  The visibility buffer is the GPU's own render_visibility, except where a test writes one
by hand; the directions are the GPU's own interpolate of the frames' normals, except where a test writes the planes by hand; the
expected values are tests/cuberef.py's on those very buffers (pinned on the CPU by tests/test_cube_ref.py).  Forward and gdir: a NaN
on one side must be a NaN on the other, every other word matches bit for bit.  gtex: exact where every partial sum is representable
(the dyadic cases) and where an element has one contributing add, else within gamma_n * sum |w g|, gamma_n = n u / (1 - n u),
u = 2^-24, n the element's contributing adds (+ 1 when the buffer held a value) — one rounding per add, the products being float32
products on both sides: derived, not measured."""
import numpy as np
import pytest
import torch

import cuberef
import interpref
import vgkit
from srz import abi, parallel
from support import SENTINEL, ccw, ctx, filled, frame, scene_pair, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
BACKDROP = ccw((-8, -8), (400, -8), (-8, 400), z=80.0, uv=((0.1, 0.2), (0.9, 0.3), (0.4, 0.95)))
BACKDROP["nrm"] = np.float32([(0.9, -0.3, 0.2), (-0.4, 0.8, 0.5), (0.1, -0.2, -0.95)])  # a slow sweep across several faces
SIZES = [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6), (1, 1, 3)]
CHANNELS = (1, 3, 4, 5, 17, 64)
CUBE_SIZES = cuberef.CUBE_SIZES
TG_SLOTS = 2048  # the capacity of k_cube_grad's table of distinct texels per tile


def n_tris(f):
    return f if isinstance(f, int) else sum(len(t) for t in f.tris)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def interp_dirs(fs, vis, frames):
    """the GPU's interpolate of the frames' own normals → the planes on the device [n, 3, rows, W] (zeros where nobody owns the
    pixel) and the attributes [n, T, 3, 3] they came from"""
    T = max(n_tris(f) for f in frames)
    a = np.zeros((len(frames), T, 3, 3), np.float32)
    for i, f in enumerate(frames):
        a[i, :n_tris(f)] = np.concatenate([t["nrm"] for t in f.tris])
    out, a_dev = torch.zeros(fs.interpolate_shape(3), dtype=torch.float32, device="cuda"), dev(a)
    fs.interpolate(vis.data_ptr(), a_dev.data_ptr(), 3, len(frames), T, out.data_ptr(), fs.interpolate_bytes(3), F, stream())
    torch.cuda.synchronize()
    return out, a


def cube_dims(cube):
    return (cube.shape[0] if cube.ndim == 5 else 1), cube.shape[-2], cube.shape[-1]


def fwd(fs, vis, dirs, cube, flags=F, fill=0):
    """the forward pass into a buffer prefilled with the word `fill` → uint32 [n, C, rows, W]"""
    tf, N, C = cube_dims(cube)
    out, t = filled(fs.interpolate_shape(C), fill), dev(cube)
    fs.texture_cube(vis.data_ptr(), dirs.data_ptr(), t.data_ptr(), N, C, tf, out.data_ptr(), fs.interpolate_bytes(C), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def bwd(fs, vis, dirs, gout, cube, want_tex=True, want_dir=True, flags=F, fill=0, into=None):
    """the backward pass → (gtex float32 of the cube's shape, added into `into` or zeros; gdir uint32 [n, 3, rows, W] from `fill`)"""
    tf, N, C = cube_dims(cube)
    t, g = dev(cube), dev(gout)
    assert tuple(g.shape) == tuple(fs.interpolate_shape(C))
    gt = (torch.zeros_like(t) if into is None else dev(into)) if want_tex else None
    gd = filled(fs.interpolate_shape(3), fill) if want_dir else None
    fs.texture_cube_grad(vis.data_ptr(), dirs.data_ptr(), g.data_ptr(), t.data_ptr(), N, C, tf, gt.data_ptr() if want_tex else None,
                         gd.data_ptr() if want_dir else None, flags, stream())
    torch.cuda.synchronize()
    return (gt.cpu().numpy() if want_tex else None), (words(gd) if want_dir else None)


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def cube_of(t, i):
    return t[i] if t.ndim == 5 else t


def expect_fwd(tmp_path, frames, v, dw, cube, fused=True, fill=0):
    """v: the visibility buffer's words [n, 4, rows, W]; dw: the direction planes float32 [n, 3, rows, W]"""
    out = []
    for i, f in enumerate(frames):
        pre = np.full((cube.shape[-1],) + v.shape[2:], fill, np.uint32)
        out.append(cuberef.forward(tmp_path, cube_of(cube, i), n_tris(f), v[i, 1], dw[i], fused, pre))
    return np.stack(out)


def expect_bwd(tmp_path, frames, v, dw, gout, cube, fused=True, fill=0):
    """(Grad per cube frame — one for a shared cube —, gdir [n, 3, rows, W] float32)"""
    shared = cube.ndim == 4
    accs = [cuberef.Grad(cube.shape[-4:]) for _ in range(1 if shared else len(frames))]
    gd = []
    for i, f in enumerate(frames):
        pre = np.full((3,) + v.shape[2:], fill, np.uint32)
        gd.append(cuberef.grad(tmp_path, cube_of(cube, i), n_tris(f), v[i, 1], dw[i], gout[i], accs[0 if shared else i], True, fused, pre))
    return accs, np.stack(gd)


def check_gtex(got, accs, what, exact=False, init=None):
    """init: what the buffer held before the call (one more term of every element's sum)"""
    ref = np.stack([a.gtex for a in accs]).reshape(got.shape)
    mag = np.stack([a.gabs for a in accs]).reshape(got.shape)
    cnt = np.stack([np.broadcast_to(a.count[..., None], a.gtex.shape) for a in accs]).reshape(got.shape).astype(np.float64)
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


def hand_frames(w, h, n, tris):
    return [frame(soup(1, tris, w, h, ZS), w, h) for _ in range(n)]


def hand_vis(ids):
    """a visibility buffer [n, 4, h, w] float32 with these id words (z, alpha, beta: zeros — the cube passes read none of them)"""
    v = np.zeros((ids.shape[0], 4) + ids.shape[1:], np.float32)
    v[:, 1] = ids.view(np.float32)
    return v


def rand_ids(rng, n, h, w, tris, holes=True):
    ids = rng.integers(1, tris + 1, (n, h, w)).astype(np.uint32)
    ids |= (rng.random((n, h, w)) < 0.4).astype(np.uint32) << 31
    if holes:
        ids[rng.random((n, h, w)) < 0.1] = 0
    return ids


# ------------------------------------------------------------------------------------------------------ forward and gdir
@pytest.mark.parametrize("w,h,n", SIZES)
def test_forward_and_gdir_sizes_and_channels(ctx, tmp_path, w, h, n):
    """the directions are the GPU's interpolate of per-vertex normals; every channel count, shared and per frame, every cube size"""
    frames = pair(w, h, n)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    assert (v[:, 1] != 0).any(1).any(1).all()
    dirs, _ = interp_dirs(fs, vis, frames)
    dw = dirs.cpu().numpy()
    own = owners(v, frames)
    wide = cuberef.make_cube(1, 5, 64, frames=2)
    gwide = rand_gout(w, (2, 64, h, w), own)
    full = fwd(fs, vis, dirs, wide, F, SENTINEL)
    same(full, expect_fwd(tmp_path, frames, v, dw, wide, fill=SENTINEL), f"{w}x{h} C 64")
    for C in CHANNELS:
        for t in (wide[..., :C], wide[0][..., :C]):  # per frame, shared
            got = fwd(fs, vis, dirs, t, F, SENTINEL)
            same(got, expect_fwd(tmp_path, frames, v, dw, t, fill=SENTINEL), f"{w}x{h} C {C} {t.ndim}")
            if t.ndim == 5:
                assert np.array_equal(got, full[:, :C]), C  # every C is a slice of a wider call
            _, gd = bwd(fs, vis, dirs, gwide[:, :C], t, want_tex=False, fill=SENTINEL)
            same(gd, expect_bwd(tmp_path, frames, v, dw, gwide[:, :C], t, fill=SENTINEL)[1], f"gdir {w}x{h} C {C} {t.ndim}")
    for k, N in enumerate(CUBE_SIZES):
        C = CHANNELS[(k + w) % len(CHANNELS)]
        cube = cuberef.make_cube(k, N, C, frames=2)
        cube = cube if k % 2 else cube[0]
        what = f"{w}x{h} N {N} C {C} {cube.ndim}"
        got = fwd(fs, vis, dirs, cube, F, SENTINEL)
        same(got, expect_fwd(tmp_path, frames, v, dw, cube, fill=SENTINEL), what)
        assert (got[np.broadcast_to(~own[:, None], got.shape)] == 0).all()
        gout = rand_gout(k, got.shape, own)
        gt, gd = bwd(fs, vis, dirs, gout, cube, fill=SENTINEL)
        accs, want_gd = expect_bwd(tmp_path, frames, v, dw, gout, cube, fill=SENTINEL)
        same(gd, want_gd, what + " gdir")
        check_gtex(gt, accs, what + " gtex")
    fs.close()


@pytest.mark.parametrize("N", CUBE_SIZES)
def test_hand_written_directions_every_cube_size(ctx, tmp_path, N):
    """planes written by hand (cuberef.hostile_dirs) under a hand-written visibility buffer with holes: every face, every edge from
    both sides, the vertex regions, ties, +-0, NaN / inf / zero / subnormal / 3e38; forward and gdir bit for bit, gtex within its
    bound, each want flag alone"""
    w, h, n = 96, 64, 2
    rng = np.random.default_rng([N, 41])
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    ids = rand_ids(rng, n, h, w, 20)
    v = hand_vis(ids)
    vw = v.view(np.uint32)
    vis = torch.as_tensor(v).cuda()
    dw = np.stack([cuberef.hostile_dirs(rng, (h, w), N) for _ in range(n)])
    own = owners(vw, frames)
    cls, face = zip(*(cuberef.classify(tmp_path, N, 20, ids[i], dw[i]) for i in range(n)))
    cls, face = np.stack(cls), np.stack(face)
    sampled = (cls & cuberef.SAMPLED) != 0
    assert set(face[sampled]) == set(range(6)) and (own & ~sampled).sum() >= 100
    assert ((cls & cuberef.CROSSED) != 0).sum() >= 300 and ((cls & cuberef.VERTEX) != 0).sum() >= 50
    sub = own & (np.abs(dw) < 2.0 ** -126).all(1) & (dw != 0).any(1)
    assert sub.sum() >= 300 and sampled[sub].all()  # subnormal directions are sampled
    taps = cuberef.taps(tmp_path, N, dw.transpose(0, 2, 3, 1)[sampled])
    sides = {(int(f), int(g)) for f, at in zip(taps["face"], taps["at"] // (N * N)) for g in at if g != f}
    assert len(sides) == 24  # every edge, from both of its faces
    dw[np.broadcast_to(~own[:, None], dw.shape)] = np.nan  # never read
    dirs = dev(dw)
    C = CHANNELS[N % len(CHANNELS)]
    for cube in (cuberef.make_cube(N, N, C), cuberef.make_cube(N, N, C, frames=n)):
        what = f"hand-written N {N} C {C} {cube.ndim}"
        got = fwd(fs, vis, dirs, cube, F, SENTINEL)
        same(got, expect_fwd(tmp_path, frames, vw, dw, cube, fill=SENTINEL), what)
        assert (got[np.broadcast_to((own & ~sampled)[:, None], got.shape)] == 0).all()
        gout = rand_gout(N, got.shape, own)
        gt, gd = bwd(fs, vis, dirs, gout, cube, fill=SENTINEL)
        accs, want_gd = expect_bwd(tmp_path, frames, vw, dw, gout, cube, fill=SENTINEL)
        same(gd, want_gd, what + " gdir")
        assert (gd[np.broadcast_to(~sampled[:, None], gd.shape)] == 0).all()
        check_gtex(gt, accs, what + " gtex")
        only_gd = bwd(fs, vis, dirs, gout, cube, want_tex=False, fill=SENTINEL)[1]
        assert np.array_equal(only_gd, gd)
        only_gt = bwd(fs, vis, dirs, gout, cube, want_dir=False)[0]
        check_gtex(only_gt, accs, what + " gtex alone")
    fs.close()


def test_nine_frames_wrap_the_frame_deal(ctx, tmp_path):
    """eight frames and more take the walk's other branch (workgroup b serves the frames f = b mod 8): with nine frames of four tiles
    the 40 workgroups stride 5 tiles, so those of frame 0 go on to a tile of frame 8 — k_cube_grad's table is handed from one tile to
    the next, its keys released in between (test_gtex_exact_on_dyadic_inputs has the same set shape, exactly)"""
    t = np.concatenate([soup(11, 60, 64, 64, ZS), BACKDROP])
    frames = []
    for i in range(9):
        t2 = t.copy()
        t2["pos"][:-1, :, :2] += np.float32([1.5 * i, -1.0 * i])
        frames.append(frame(t2, 64, 64))
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    dirs, _ = interp_dirs(fs, vis, frames)
    dw = dirs.cpu().numpy()
    for cube in (cuberef.make_cube(4, 8, 5, frames=9), cuberef.make_cube(4, 8, 5)):
        got = fwd(fs, vis, dirs, cube, F, SENTINEL)
        same(got, expect_fwd(tmp_path, frames, v, dw, cube, fill=SENTINEL), "nine frames")
        gout = rand_gout(3, got.shape)
        gt, gd = bwd(fs, vis, dirs, gout, cube, fill=SENTINEL)
        accs, want_gd = expect_bwd(tmp_path, frames, v, dw, gout, cube, fill=SENTINEL)
        same(gd, want_gd, "nine frames gdir")
        check_gtex(gt, accs, f"nine frames gtex {cube.ndim}")
    assert len({got[i].tobytes() for i in range(9)}) == 9
    fs.close()


def test_not_fused_and_ids_out_of_range(ctx, tmp_path):
    """frames that do not clear; ids out of range and bare class bits written into the buffer; hand-written directions: with the fused
    clear nobody's words become 0, without it the prefilled sentinel survives on exactly nobody's pixels"""
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
    dw = np.stack([cuberef.hostile_dirs(rng, (80, 96), 5) for _ in range(2)])
    hit = rng.random(dw.shape) < 0.1
    dw[hit] = cuberef.SPECIALS[rng.integers(0, len(cuberef.SPECIALS), int(hit.sum()))]
    cls = np.stack([cuberef.classify(tmp_path, 5, len(t), vw[i, 1], dw[i])[0] for i in range(2)])
    unsampled = own & ((cls & cuberef.SAMPLED) == 0)
    assert unsampled.sum() >= 50
    dw[np.broadcast_to(~own[:, None], dw.shape)] = np.nan  # never read
    dirs = dev(dw)
    cube = cuberef.make_cube(6, 5, 6)
    fused, kept = fwd(fs, vis, dirs, cube, F, SENTINEL), fwd(fs, vis, dirs, cube, 0, SENTINEL)
    same(fused, expect_fwd(tmp_path, frames, vw, dw, cube, True, SENTINEL), "fused")
    same(kept, expect_fwd(tmp_path, frames, vw, dw, cube, False, SENTINEL), "not fused")
    assert (fused[0][:, nobody] == 0).all() and (kept[0][:, nobody] == SENTINEL).all()  # exactly the owned words change
    assert (kept[0][:, own[0]] != SENTINEL).all() and (kept[np.broadcast_to(unsampled[:, None], kept.shape)] == 0).all()
    gout = rand_gout(5, fused.shape, own)
    for fl, fused_ in ((F, True), (0, False)):
        gt, gd = bwd(fs, vis, dirs, gout, cube, flags=fl, fill=SENTINEL)
        accs, want_gd = expect_bwd(tmp_path, frames, vw, dw, gout, cube, fused_, SENTINEL)
        same(gd, want_gd, f"gdir fused {fused_}")
        assert (gd[0][:, nobody] == (0 if fused_ else SENTINEL)).all()
        check_gtex(gt, accs, f"gtex fused {fused_}")
    fs.close()


def test_non_finite_texels_and_gradients_propagate(ctx, tmp_path):
    frames = pair(64, 64, 90)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    dirs, _ = interp_dirs(fs, vis, frames)
    dw = dirs.cpu().numpy()
    cube = cuberef.make_cube(7, 5, 4)
    cube[0, 1, 2, 0], cube[3, 3, 3, 1], cube[5, 4, 0, 2] = np.nan, np.inf, -np.inf
    got = fwd(fs, vis, dirs, cube)
    same(got, expect_fwd(tmp_path, frames, v, dw, cube), "non-finite texels")
    assert np.isnan(got.view(np.float32)).any()
    gout = rand_gout(9, got.shape)
    _, gd = bwd(fs, vis, dirs, gout, cube, want_tex=False)
    same(gd, expect_bwd(tmp_path, frames, v, dw, gout, cube)[1], "non-finite texels gdir")
    fs.close()


# ------------------------------------------------------------------------------------------------------ gtex, by construction
def dyadic_dirs(rng, shape, lo=-64, hi=64):
    """directions whose major component is +-1, +-2 or +-0.5 and whose others are k / 64 of it, on a random face: s and t are k / 64,
    exactly, whichever face; at N = 8 the fractions are multiples of 1 / 16 and the weights of 1 / 256"""
    d = np.zeros(shape + (3,), np.float32)
    m = rng.integers(0, 3, shape)
    major = rng.choice(np.float32([1, -1, 2, -2, 0.5, -0.5]), shape)
    a, b = rng.integers(lo, hi + 1, shape), rng.integers(lo, hi + 1, shape)
    for ax in range(3):
        sel = m == ax
        d[sel, ax] = major[sel]
        d[sel, (ax + 1) % 3] = np.abs(major[sel]) * a[sel] / 64
        d[sel, (ax + 2) % 3] = np.abs(major[sel]) * b[sel] / 64
    return d


@pytest.mark.parametrize("C", [1, 5, 8])
@pytest.mark.parametrize("w,h,n", [(96, 96, 2), (50, 37, 2), (64, 64, 9)])
def test_gtex_exact_on_dyadic_inputs(ctx, tmp_path, C, w, h, n):
    """N = 8, s and t multiples of 1 / 64 up to and including +-1 (edges, ties and vertices among them), integer gout in [-16, 16],
    an integer buffer to add into: every product is a multiple of 1 / 256 and every partial sum is representable, so any order of
    adds gives the same bits — seam adds into the neighbouring faces included"""
    rng = np.random.default_rng([C, w, 3])
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    ids = rand_ids(rng, n, h, w, 20)
    v = hand_vis(ids)
    vis = torch.as_tensor(v).cuda()
    dw = np.ascontiguousarray(dyadic_dirs(rng, (n, h, w)).transpose(0, 3, 1, 2))
    dirs = dev(dw)
    shared = n != 2
    cube = rng.integers(-8, 9, ((6, 8, 8, C) if shared else (n, 6, 8, 8, C))).astype(np.float32)
    gout = rng.integers(-16, 17, (n, C, h, w)).astype(np.float32)
    init = rng.integers(-64, 65, cube.shape).astype(np.float32)
    gt, gd = bwd(fs, vis, dirs, gout, cube, fill=SENTINEL, into=init)
    accs, want_gd = expect_bwd(tmp_path, frames, v.view(np.uint32), dw, gout, cube, fill=SENTINEL)
    same(gd, want_gd, "dyadic gdir")
    check_gtex(gt, accs, f"dyadic {w}x{h} C {C}", exact=True, init=init)
    assert (gt != init).any()
    same(fwd(fs, vis, dirs, cube), expect_fwd(tmp_path, frames, v.view(np.uint32), dw, cube), "dyadic forward")
    fs.close()


def test_a_tile_straddling_a_cube_edge_adds_into_both_faces(ctx, tmp_path):
    """one 32 x 32 tile whose directions lie on both sides of the +X / +Z edge, and one around the vertex of +X, +Y and +Z: the adds of
    one tile's table land in two and in three faces; dyadic, so exact"""
    w = h = 32
    frames = hand_frames(w, h, 2, 20)
    fs = ctx.frameset(frames)
    ids = rand_ids(np.random.default_rng(5), 2, h, w, 20, holes=False)
    v = hand_vis(ids)
    vis = torch.as_tensor(v).cuda()
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    one = np.ones((h, w))
    # frame 0: the left half on +X running up to the edge (dz from 17/32 to 1), the right half on +Z running away from it; the major
    # component is 1 everywhere, so s and t stay multiples of 1 / 32 on both faces
    left = xs < 16
    d0 = np.stack([np.where(left, one, (48 - xs) / 32.0), (ys - 4) / 32.0, np.where(left, (17 + xs) / 32.0, one)])
    # frame 1: three column bands on +X, +Y and +Z, all within half a texel of the vertex they share
    a, b = 1 - (ys % 8) / 32.0, 1 - (xs % 8) / 32.0
    band = np.minimum(xs // 11, 2)
    d1 = np.stack([np.where(band == 0, one, a), np.where(band == 1, one, np.where(band == 0, a, b)), np.where(band == 2, one, b)])
    dw = np.stack([d0, d1]).astype(np.float32)
    dirs = dev(dw)
    cube = np.random.default_rng(6).integers(-8, 9, (6, 8, 8, 3)).astype(np.float32)
    gout = np.random.default_rng(7).integers(-16, 17, (2, 3, h, w)).astype(np.float32)
    cls0, face0 = cuberef.classify(tmp_path, 8, 20, ids[0], dw[0])
    cls1, face1 = cuberef.classify(tmp_path, 8, 20, ids[1], dw[1])
    assert set(face0.ravel()) == {0, 4} and ((cls0 & cuberef.CROSSED) != 0).sum() >= 64
    assert set(face1.ravel()) == {0, 2, 4} and ((cls1 & cuberef.VERTEX) != 0).sum() >= 4
    gt, gd = bwd(fs, vis, dirs, gout, cube, fill=SENTINEL)
    accs, want_gd = expect_bwd(tmp_path, frames, v.view(np.uint32), dw, gout, cube, fill=SENTINEL)
    same(gd, want_gd, "seam gdir")
    check_gtex(gt, accs, "seam adds", exact=True)
    per_face = (accs[0].count.reshape(6, -1) > 0).any(1)
    assert per_face[[0, 2, 4]].all() and (np.abs(gt).reshape(6, -1).sum(1)[[0, 2, 4]] > 0).all()
    same(fwd(fs, vis, dirs, cube), expect_fwd(tmp_path, frames, v.view(np.uint32), dw, cube), "seam forward")
    fs.close()


def test_table_overflow(ctx, tmp_path):
    """independent random directions per pixel on N = 64 over one 32 x 32 tile: up to 4 096 distinct texels against the table's 2 048
    slots — the corners without a slot add straight to memory, and the bound still holds"""
    w = h = 32
    n, C, N = 2, 5, 64
    frames = hand_frames(w, h, n, 20)
    fs = ctx.frameset(frames)
    rng = np.random.default_rng(31)
    ids = rand_ids(rng, n, h, w, 20, holes=False)
    v = hand_vis(ids)
    vis = torch.as_tensor(v).cuda()
    dw = rng.normal(0, 1, (n, 3, h, w)).astype(np.float32)
    dirs = dev(dw)
    for i in range(n):  # the tile really exceeds the table (counted from the reference's own taps: each add names its texel)
        probe = cuberef.Grad((6, N, N, 1))
        cuberef.grad(tmp_path, np.zeros((6, N, N, 1), np.float32), 20, ids[i], dw[i], np.ones((1, h, w), np.float32), probe, False)
        assert int((probe.count > 0).sum()) > TG_SLOTS and int(probe.count.sum()) == 4 * w * h
    for cube in (cuberef.make_cube(8, N, C), cuberef.make_cube(8, N, C, frames=n)):
        gout = rand_gout(11, (n, C, h, w))
        gt, gd = bwd(fs, vis, dirs, gout, cube, fill=SENTINEL)
        accs, want_gd = expect_bwd(tmp_path, frames, v.view(np.uint32), dw, gout, cube, fill=SENTINEL)
        same(gd, want_gd, "overflow gdir")
        check_gtex(gt, accs, f"overflow {cube.ndim}")
        assert (gt != 0).any()
    fs.close()


@pytest.mark.parametrize("w,h,n", SIZES[:3])
def test_gtex_on_rendered_buffers_and_accumulation(ctx, tmp_path, w, h, n):
    frames = pair(w, h, n)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    dirs, _ = interp_dirs(fs, vis, frames)
    dw = dirs.cpu().numpy()
    own = owners(v, frames)
    for C in (3, 17):
        for cube in (cuberef.make_cube(C, 64, C, frames=2), cuberef.make_cube(C, 2, C)):
            gout = rand_gout(C, (2, C, h, w), own)
            gt, gd = bwd(fs, vis, dirs, gout, cube)
            accs, want_gd = expect_bwd(tmp_path, frames, v, dw, gout, cube)
            same(gd, want_gd, f"gdir C {C}")
            check_gtex(gt, accs, f"{w}x{h} C {C} {cube.ndim}")
            only_gt = bwd(fs, vis, dirs, gout, cube, want_dir=False)[0]
            check_gtex(only_gt, accs, f"{w}x{h} C {C} {cube.ndim} gtex alone")
    # accumulation into a buffer that is not zero: one more term per element
    init = np.random.default_rng(4).normal(0, 5, cube.shape).astype(np.float32)
    gt2, _ = bwd(fs, vis, dirs, gout, cube, want_dir=False, into=init)
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
    dirs, _ = interp_dirs(fs, vis, frames)
    dw = dirs.cpu().numpy()
    cube = cuberef.make_cube(12, 5, 5)
    gout = rand_gout(13, (2, 5, h, w))
    full = fwd(fs, vis, dirs, cube)
    same(full, expect_fwd(tmp_path, frames, v, dw, cube), "whole frame")
    whole_gd = bwd(fs, vis, dirs, gout, cube, want_tex=False)[1]
    accs, _ = expect_bwd(tmp_path, frames, v, dw, gout, cube)
    fs.close()
    total = np.zeros(cube.shape, np.float64)
    for rank in (0, 1):
        c = srz.Context(0, rank, 2)
        sfs = c.frameset(frames)
        svis = visibility(sfs)
        sdirs, _ = interp_dirs(sfs, svis, frames)
        shard = fwd(sfs, svis, sdirs, cube)
        rows = parallel.band_rows(h, rank, 2)
        assert len(rows) == 2
        sg = np.zeros(sfs.interpolate_shape(5), np.float32)
        for (lb, _, r0, r1) in rows:
            same(shard[:, :, lb * 32: lb * 32 + r1 - r0], full[:, :, r0:r1], f"rank {rank} band {lb}")
            sg[:, :, lb * 32: lb * 32 + r1 - r0] = gout[:, :, r0:r1]
        part, part_gd = bwd(sfs, svis, sdirs, sg, cube)
        for (lb, _, r0, r1) in rows:
            same(part_gd[:, :, lb * 32: lb * 32 + r1 - r0], whole_gd[:, :, r0:r1], f"gdir rank {rank} band {lb}")
        assert (part != 0).any()
        total += part.astype(np.float64)
        sfs.close(), c.close()
    # each rank's sums lie within the bound of its own adds; the two bounds add up to at most the whole frame's
    err = np.abs(total - accs[0].gtex)
    assert (err <= accs[0].bound()).all(), float((err - accs[0].bound()).max())


# ------------------------------------------------------------------------------------------------------ the chain, autograd
def test_autograd(ctx, tmp_path, monkeypatch):
    import srz
    from srz.visibility import interpolate, texture_cube, texture_cube_grad
    frames = pair(100, 70, 120)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    dirs, attr = interp_dirs(fs, vis, frames)
    dw = dirs.cpu().numpy()
    calls = []
    real = srz.FrameSet.texture_cube_grad
    monkeypatch.setattr(srz.FrameSet, "texture_cube_grad", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    for shape in ((6, 5, 5, 6), (2, 6, 5, 5, 6)):
        cuben = np.random.default_rng(16).normal(0, 3, shape).astype(np.float32)
        cube = dev(cuben).requires_grad_(True)
        dt = dirs.clone().requires_grad_(True)
        out = texture_cube(fs, vis, cube, dt)
        assert out.shape == (2, 6, 70, 100) and out.requires_grad
        same(words(out.detach()), fwd(fs, vis, dirs, cuben), "forward")
        out.square().sum().backward()
        torch.cuda.synchronize()
        g = (2 * out.detach()).contiguous()  # float32: what the backward was handed
        gt, gd = texture_cube_grad(fs, vis, cube.detach(), dirs, g)
        same(words(dt.grad), words(gd), "dirs.grad")
        accs, want_gd = expect_bwd(tmp_path, frames, v, dw, g.cpu().numpy(), cuben)
        same(words(gd), want_gd, "plain gdir")
        check_gtex(cube.grad.cpu().numpy(), accs, "cube.grad")
        check_gtex(gt.cpu().numpy(), accs, "plain gtex")
        assert texture_cube_grad(fs, vis, cube.detach(), dirs, g, want_gdir=False)[1] is None
        assert texture_cube_grad(fs, vis, cube.detach(), dirs, g, want_gtex=False)[0] is None
    # through interpolate: the loss reaches the direction attributes
    a = dev(attr).requires_grad_(True)
    cube = dev(cuben).requires_grad_(True)
    n = len(calls)
    out = texture_cube(fs, vis, cube, interpolate(fs, vis, a))
    same(words(out.detach()), fwd(fs, vis, dirs, cuben), "composed forward")
    out.square().sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == n + 1  # one call for both gradients
    g = (2 * out.detach()).contiguous().cpu().numpy()
    accs, want_gd = expect_bwd(tmp_path, frames, v, dw, g, cuben)
    check_gtex(cube.grad.cpu().numpy(), accs, "composed cube.grad")
    got = a.grad.cpu().numpy()
    for i, f in enumerate(frames):
        acc = interpref.Grad(attr.shape[1:])
        interpref.grad(tmp_path, attr[i], n_tris(f), v[i], want_gd[i], into=acc, want_bary=False)
        assert (np.abs(got[i].astype(np.float64) - acc.gattr) <= acc.bound()).all() and (got[i] != 0).sum() > 100
    # nothing needs a gradient: no backward is there to launch; one input does: the call asks for that output alone
    n = len(calls)
    out = texture_cube(fs, vis, cube.detach(), dirs)
    assert not out.requires_grad and out.grad_fn is None and len(calls) == n
    dt = dirs.clone().requires_grad_(True)
    texture_cube(fs, vis, cube.detach(), dt).sum().backward()
    assert len(calls) == n + 1 and dt.grad is not None
    with pytest.raises(ValueError):
        texture_cube(fs, vis, dev(np.zeros((5, 4, 4, 3))), dirs)
    with pytest.raises(ValueError):
        texture_cube(fs, vis, cube.detach(), dirs[:, :2])
    fs.close()


def test_the_chain_from_the_vertices_on_a_sceneset(ctx, tmp_path):
    """texture_cube(fs, vis, cube, interpolate(fs, vis, corner_attr(fs, {slot: mesh_normals(ctx, slot, verts)}))): finite, non-zero
    gradients reach the cube and the vertices, and they are the chain composed from the plain gradient calls — gdir bit for bit
    (deterministic), cube.grad within gtex's bound, the direction attributes' gradient within interpolate_grad's own bound (its float
    atomics), and from there to the vertices bit for bit (corner_attr_grad and mesh_normals_grad are gathers)"""
    from srz import visibility as V
    W = H = 64
    SLOT = 3
    ident = np.eye(4, dtype=np.float32).reshape(16)
    pos, faces = vgkit.grid(16, 16, 3, extra=1)
    mvps = [vgkit.perspective(50.0, 46.0, 5.0, 6.0), vgkit.perspective(38.0, 52.0, 14.0, 3.0, w=1.5, wx=-0.2, wy=0.3, wz=0.25, sz=2.0, oz=4.0)]
    faces = vgkit.oriented(pos, faces, mvps[0])
    v8 = vgkit.verts8(pos)
    sframes, plain = [], []
    for i, m in enumerate(mvps):
        sf, f = scene_pair([(v8, faces, abi.SHADER_NORMAL, -1, m, ident)], W, H, (0.0, 0.0, 1.0), [], 1.75, 0.5, ctx=ctx if i == 0 else None,
                           slots=[SLOT])
        sframes.append(sf), plain.append(f)
    fs = ctx.frameset(sframes)
    T = max(f.n_tris for f in plain)
    vis = visibility(fs)
    v = words(vis)
    own = owners(v, [T, T])
    assert own.sum() > 500
    cuben = cuberef.make_cube(19, 8, 3)
    cube, verts = dev(cuben).requires_grad_(True), dev(pos).requires_grad_(True)
    normals = V.mesh_normals(ctx, SLOT, verts)
    attr = V.corner_attr(fs, {SLOT: normals}, pos_tris=T)
    dirs = V.interpolate(fs, vis, attr)
    attr.retain_grad(), dirs.retain_grad()
    out = V.texture_cube(fs, vis, cube, dirs)
    dw = dirs.detach().cpu().numpy()
    same(words(out.detach()), expect_fwd(tmp_path, [T, T], v, dw, cuben), "chain forward")
    weight = dev(np.random.default_rng(20).normal(0, 1, tuple(out.shape)))
    (out * weight).sum().backward()
    torch.cuda.synchronize()
    for g in (cube.grad, verts.grad):
        assert bool(torch.isfinite(g).all()) and int((g != 0).sum()) > g.numel() // 20
    # the same chain from the plain calls
    gout = weight.contiguous()
    gt, gd = V.texture_cube_grad(fs, vis, cube.detach(), dirs.detach(), gout)
    same(words(dirs.grad), words(gd), "dirs.grad against the plain call")
    accs, want_gd = expect_bwd(tmp_path, [T, T], v, dw, gout.cpu().numpy(), cuben)
    same(words(gd), want_gd, "plain gdir")
    check_gtex(cube.grad.cpu().numpy(), accs, "chain cube.grad")
    check_gtex(gt.cpu().numpy(), accs, "plain gtex")
    attrn, gattr = attr.detach().cpu().numpy(), attr.grad.cpu().numpy()
    for i in range(2):
        acc = interpref.Grad(attrn.shape[1:])
        interpref.grad(tmp_path, attrn[i], T, v[i], want_gd[i], into=acc, want_bary=False)
        assert (np.abs(gattr[i].astype(np.float64) - acc.gattr) <= acc.bound()).all() and (gattr[i] != 0).sum() > 100
    ga = attr.grad.contiguous()
    gn = torch.empty((2, len(pos), 3), dtype=torch.float32, device="cuda")
    fs.corner_attr_grad(SLOT, ga.data_ptr(), 3, gn.data_ptr(), T, stream())
    gnrm = gn.sum(0).contiguous()
    p = verts.detach().contiguous()
    work, gpos = torch.empty_like(p), torch.empty_like(p)
    ctx.mesh_normals_grad(SLOT, p.data_ptr(), 3, 1, gnrm.data_ptr(), 3, work.data_ptr(), gpos.data_ptr(), stream())
    torch.cuda.synchronize()
    same(words(verts.grad), words(gpos), "verts.grad against the plain calls")
    fs.close()
