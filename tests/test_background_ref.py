"""not-gpu: the background pass's CPU reference (tests/background_ref.c through tests/backgroundref.py) pinned against include/srz.h's
rule: the directions it computes, the forward against tests/cuberef.py's on those directions, seamlessness across all 12 edges, which
pixels are the pass's and what becomes of the others, the gradients against central differences of a binary64 restatement in numpy,
and the fixed tree against a tree written by hand."""
import numpy as np
import pytest

import backgroundref as br
import cuberef
from cuberef import AXES

B = np.array(AXES, np.float64)  # [face][n, su, sv][3]
U = 2.0 ** -24
NEAR = 1e-3  # pixels this close to a texel boundary (in texels) or to a face change (in s, t) stay out of the comparisons
CAP = 0.10   # and they may be at most this share of the sampled pixels


def hand_ids(rng, h, w, tris, holes=0.5):
    ids = rng.integers(1, tris + 1, (h, w)).astype(np.uint32)
    ids |= (rng.random((h, w)) < 0.4).astype(np.uint32) << 31
    k = rng.random((h, w))
    ids[k < holes] = 0
    ids[(k >= holes) & (k < holes + 0.05)] = 0x80000000       # the bare class bit
    ids[(k >= holes + 0.05) & (k < holes + 0.1)] = tris + 7   # an index outside the frame's triangles
    return ids


# ------------------------------------------------------------------------------------------------------ forward
def test_directions_are_the_rule(tmp_path):
    """dyadic blocks: every product and sum is exact, so the planes are r0 + x rx + y ry in any arithmetic; a general block: within
    the two roundings of the two fmafs"""
    ray = np.float32([1, -2, 0.5, 0.25, 0.5, -0.125, -0.5, 1, 2])
    d = br.dirs(tmp_path, ray, (37, 50))
    y, x = np.mgrid[0:37, 0:50]
    for c in range(3):
        assert np.array_equal(d[c], (ray[c] + x * ray[3 + c] + y * ray[6 + c]).astype(np.float32))
    ray = br.camera_block(50, 37, 3)
    d = br.dirs(tmp_path, ray, (37, 50)).astype(np.float64)
    r = ray.astype(np.float64)
    for c in range(3):
        inner = r[c] + x * r[3 + c]
        want = inner + y * r[6 + c]
        assert (np.abs(d[c] - want) <= U * (np.abs(inner) + np.abs(want)) * 1.0001).all()


@pytest.mark.parametrize("w,h,N,C", [(64, 64, 8, 3), (100, 70, 5, 1), (50, 37, 64, 5), (33, 1, 2, 17), (1, 1, 1, 64)])
def test_forward_is_cuberefs_on_the_computed_directions(tmp_path, w, h, N, C):
    """nobody's pixels, fused and not, and every pixel: the pass's pixels hold cuberef.forward's words for the directions the rule
    computes, the owned ones 0 or the words they held"""
    rng = np.random.default_rng([w, h, N])
    ids = hand_ids(rng, h, w, 20)
    ray = br.camera_block(w, h, N, spread=1.6)
    cube = cuberef.make_cube(N, N, C)
    d = br.dirs(tmp_path, ray, (h, w))
    everyone = cuberef.forward(tmp_path, cube, 1, np.ones((h, w), np.uint32), d)  # every pixel an owner there: every pixel sampled here
    owned = ((ids & 0x7fffffff) - np.uint32(1)) < 20
    assert owned.any() or w * h == 1
    pre = np.full((C, h, w), 0x7fc12345, np.uint32)
    full = br.forward(tmp_path, cube, 20, None, ray, br.ALL, True, pre, shape=(h, w))
    assert np.array_equal(full.view(np.uint32), everyone.view(np.uint32))
    assert np.array_equal(br.forward(tmp_path, cube, 20, ids, ray, br.ALL, False, pre).view(np.uint32), full.view(np.uint32))
    for fused in (True, False):
        got = br.forward(tmp_path, cube, 20, ids, ray, br.NOBODY, fused, pre).view(np.uint32)
        m = np.broadcast_to(owned, got.shape)
        assert np.array_equal(got[~m], everyone.view(np.uint32)[~m])
        assert (got[m] == (0 if fused else 0x7fc12345)).all()
    cls, face, _ = br.classify(tmp_path, N, 20, ids, ray)
    assert np.array_equal((cls & br.PASS) != 0, ~owned)
    assert np.array_equal((cls & br.SAMPLED) != 0, ~owned)  # a finite camera: every ray is sampled


def edge_blocks():
    """the 12 edges as ray blocks over a 29 x 1 frame: pixel x has the direction (+-1, +-1, (x - 14) / 16) in one of the three axis
    pairs, exactly (dyadic) → [(block, face A, face B)]"""
    out = []
    for m1, m2 in ((0, 1), (0, 2), (1, 2)):
        for s1 in (1, -1):
            for s2 in (1, -1):
                ray = np.zeros(9, np.float32)
                ray[m1], ray[m2], ray[3 - m1 - m2] = s1, s2, -14 / 16
                ray[3 + (3 - m1 - m2)] = 1 / 16
                out.append((ray, 2 * m1 + (s1 < 0), 2 * m2 + (s2 < 0)))
    return out


def test_a_ray_on_an_edge_gives_the_same_word_through_either_face(tmp_path):
    """tests/test_cube_ref.py's dyadic case — N = 8, integer texels, directions (+-1, +-1, k / 16): every product and sum of the
    lookup is exact —, the directions computed by the rule from twelve blocks"""
    N = 8
    cube = np.random.default_rng(1).integers(-8, 9, (6, N, N, 2)).astype(np.float32)
    want_d, fa, fb = cuberef.edge_dirs()
    got_d = []
    for i, (ray, a, b) in enumerate(edge_blocks()):
        d = br.dirs(tmp_path, ray, (1, 29))
        got_d.append(d[:, 0].T)
        out = br.forward(tmp_path, cube, 0, None, ray, br.ALL, shape=(1, 29))[:, 0].T
        for face in (a, b):
            assert np.array_equal(out.view(np.uint32), cuberef.sample(tmp_path, cube, d[:, 0].T, force=face).view(np.uint32)), (i, face)
    assert np.array_equal(np.concatenate(got_d), want_d) and len(set(zip(fa.tolist(), fb.tolist()))) == 12


def test_unsampled_rays_write_zeros_and_add_nothing(tmp_path):
    """non-finite and zero blocks: every pixel of the pass is written 0, contributes no add and no term; a block that is zero at one
    pixel only leaves that pixel out"""
    cube = cuberef.make_cube(2, 5, 3)
    pre = np.full((3, 4, 6), 0x7fc12345, np.uint32)
    g = np.ones((3, 4, 6), np.float32)
    for ray in (np.zeros(9), [np.nan, 0, 1, 0, 0, 0, 0, 0, 0], [1, 1, 1, np.inf, 0, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0, -np.inf, 0],
                [-0.0, 0.0, -0.0, 0, 0, 0, 0, 0, 0]):
        out = br.forward(tmp_path, cube, 1, None, ray, br.ALL, False, pre, shape=(4, 6)).view(np.uint32)
        if np.isinf(np.float32(ray)).any():  # x = 0 or y = 0 times inf is NaN, times a finite x it is inf: never finite
            assert (out == 0).all()
        acc = br.Grad(cube.shape)
        row, term, smp = br.grad(tmp_path, cube, 1, None, ray, g, acc, br.ALL, shape=(4, 6))
        assert (out == 0).all() and not smp.any() and acc.count.sum() == 0 and (row.view(np.uint32) == 0).all() and acc.n[0] == 0
    ray = np.float32([-2, -1, 0, 1, 0, 0, 0, 1, 0])  # d = (x - 2, y - 1, 0): zero at (2, 1) only
    cls, _, _ = br.classify(tmp_path, 5, 1, None, ray, br.ALL, shape=(4, 6))
    assert (cls[1, 2] & br.SAMPLED) == 0 and ((cls & br.SAMPLED) != 0).sum() == 23


# ------------------------------------------------------------------------------------------------------ gradients
def restate64(ray, cube, N, g, xs, ys, face, x0y0, at):
    """the loss sum_p sum_ch g * out in binary64 with the face and the texels of every pixel held: ray [9], cube [6, N, N, C] float64;
    g [P, C]; xs, ys, face [P]; x0y0 [P, 2]; at [P, 4].  Asserts that no pixel left its texel."""
    d = ray[0:3] + xs[:, None] * ray[3:6] + ys[:, None] * ray[6:9]
    n, su, sv = B[face, 0], B[face, 1], B[face, 2]
    ma = (d * n).sum(1)
    fx = ((d * su).sum(1) / ma * 0.5 + 0.5) * N - 0.5
    fy = ((d * sv).sum(1) / ma * 0.5 + 0.5) * N - 0.5
    a, b = fx - x0y0[:, 0], fy - x0y0[:, 1]
    assert (a > 0).all() and (a < 1).all() and (b > 0).all() and (b < 1).all() and (ma > 0).all()
    tex = cube.reshape(-1, cube.shape[-1])[at]  # [P, 4, C]
    top, bot = tex[:, 0] + a[:, None] * (tex[:, 1] - tex[:, 0]), tex[:, 2] + a[:, None] * (tex[:, 3] - tex[:, 2])
    return float(((top + b[:, None] * (bot - top)) * g).sum())


@pytest.mark.parametrize("w,h,N,C,spread", [(64, 64, 8, 3, 1.6), (100, 70, 5, 2, 1.0), (50, 37, 2, 4, 1.8), (33, 1, 8, 1, 1.2), (40, 40, 1, 3, 1.6)])
def test_gtex_and_gray_against_central_differences(tmp_path, w, h, N, C, spread):
    """L = sum over the pass's pixels and channels of g * out, restated in binary64 with each pixel's face and texels held.  Pixels within
    NEAR of a texel boundary or of a face change are left out on both sides (their g is 0), at most CAP of the sampled ones: asserted
    first, from the reference's own taps.
    gray: the exact (binary64) sum of the reference's float32 terms against the central difference of L in each of the nine entries,
    step h = NEAR / (8 N max(w, h)) — a ray moves by at most h max(x, y, 1), its texel coordinates by at most sqrt(3) N times that over
    |d| >= 1 / 2, so no pixel leaves its texel.  Tolerance per entry: sum over the pixels of m K ((C + 16 + 4 N) 2^-24 + 2^-22), m = 1,
    x, y — tests/test_cube_ref.py's gdir tolerance, with its derivation, K = N / ma * sum_ch |g| * (the largest difference of two of
    the four texels) — plus one rounding of the product by x or y, folded into the 16.  And the tree's float32 row against that exact
    sum: within Grad.ray_bound.
    gtex: L is linear in the texels, so the central difference in a texel element is its coefficient sum w64 g.  The reference's sum
    of the float32 products w32 * g differs by the rounding of the weights: tx, ty carry an absolute error below 4 N 2^-24 (s by one
    rounding, u by one, fx by two at magnitude <= N), a weight — a product of two such factors in [0, 1] — below (8 N + 3) 2^-24, and
    the product with g one more rounding: (8 N + 4) 2^-24 * sum |g| over the element's adds."""
    rng = np.random.default_rng([w, h, N, C])
    ids = hand_ids(rng, h, w, 20)
    ray = br.camera_block(w, h, N + C, spread)
    cube = cuberef.make_cube(N + 3, N, C)
    cls, _, _ = br.classify(tmp_path, N, 20, ids, ray)
    sampled = (cls & br.SAMPLED) != 0
    d = br.dirs(tmp_path, ray, (h, w))
    t = cuberef.taps(tmp_path, N, d.reshape(3, -1).T)
    frac, st = t["frac"].reshape(h, w, 2), t["st"].reshape(h, w, 2)
    near = (np.minimum(frac, 1 - frac).min(-1) < NEAR) | (1 - np.abs(st).max(-1) < NEAR)
    keep = sampled & ~near
    left_out = (sampled & near).sum() / sampled.sum()
    print(f"{w}x{h} N {N}: sampled {int(sampled.sum())}, left out {left_out:.3%}")
    assert left_out <= CAP and keep.sum() >= min(10, sampled.sum())
    g = rng.normal(0, 2, (C, h, w)).astype(np.float32)
    g[:, ~keep] = 0
    acc = br.Grad(cube.shape)
    row, term, smp = br.grad(tmp_path, cube, 20, ids, ray, g, acc)
    assert np.array_equal(smp, sampled)
    ys, xs = np.nonzero(keep)
    args = (g[:, keep].T.astype(np.float64), xs.astype(np.float64), ys.astype(np.float64), t["face"].reshape(h, w)[keep],
            t["x0y0"].reshape(h, w, 2)[keep].astype(np.float64), t["at"].reshape(h, w, 4)[keep].astype(np.int64))
    ray64, cube64 = ray.astype(np.float64), cube.astype(np.float64)
    # ---- gray
    step = NEAR / (8 * N * max(w, h))
    fd = np.zeros(9)
    for j in range(9):
        e = np.zeros(9)
        e[j] = step
        fd[j] = (restate64(ray64 + e, cube64, N, *args) - restate64(ray64 - e, cube64, N, *args)) / (2 * step)
    tex = cube64.reshape(-1, C)[args[5]]
    D = np.abs(tex[:, :, None] - tex[:, None]).max((1, 2))  # [P, C]
    ma = np.abs(d[:, keep].astype(np.float64)).max(0)
    K = N / ma * (np.abs(args[0]) * D).sum(1)
    per_px = K * ((C + 16 + 4 * N) * U + 2.0 ** -22)
    tol = np.concatenate([np.full(3, per_px.sum()), np.full(3, (per_px * args[1]).sum()), np.full(3, (per_px * args[2]).sum())])
    exact = term.astype(np.float64).sum((1, 2))
    assert np.array_equal(exact, acc.gsum) or np.allclose(exact, acc.gsum, rtol=1e-12, atol=0)
    print("gray: max |exact - fd| / tol", np.max(np.abs(acc.gsum - fd) / np.maximum(tol, 1e-300)))
    assert (np.abs(acc.gsum - fd) <= tol).all(), (acc.gsum, fd, tol)
    assert (np.abs(row.astype(np.float64) - acc.gsum) <= acc.ray_bound()).all() and acc.n[0] == sampled.sum()
    # ---- gtex: the coefficient of every element, and the central difference itself at some of the touched ones
    P = len(xs)
    a, b = np.zeros(P), np.zeros(P)
    dd = ray64[0:3] + args[1][:, None] * ray64[3:6] + args[2][:, None] * ray64[6:9]
    f = args[3]
    mm = (dd * B[f, 0]).sum(1)
    a = ((dd * B[f, 1]).sum(1) / mm * 0.5 + 0.5) * N - 0.5 - args[4][:, 0]
    b = ((dd * B[f, 2]).sum(1) / mm * 0.5 + 0.5) * N - 0.5 - args[4][:, 1]
    w64 = np.stack([(1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b], 1)  # [P, 4]
    coef, mag = np.zeros((6 * N * N, C)), np.zeros((6 * N * N, C))
    for k in range(4):
        np.add.at(coef, args[5][:, k], w64[:, k, None] * args[0])
        np.add.at(mag, args[5][:, k], np.abs(args[0]))
    got = acc.gtex.reshape(-1, C)
    assert (np.abs(got - coef) <= (8 * N + 4) * U * mag).all()
    touched = np.argwhere(mag > 0)
    for e_i in touched[rng.permutation(len(touched))[:24]]:
        e = np.zeros_like(cube64).reshape(-1, C)
        e[tuple(e_i)] = 0.5
        e = e.reshape(cube64.shape)
        fd_t = restate64(ray64, cube64 + e, N, *args) - restate64(ray64, cube64 - e, N, *args)  # (2 h = 1)
        assert abs(fd_t - coef[tuple(e_i)]) <= 1e-9 * (1 + mag[tuple(e_i)] * np.abs(cube64).max())
        assert abs(got[tuple(e_i)] - fd_t) <= (8 * N + 4) * U * mag[tuple(e_i)] + 1e-9 * (1 + mag[tuple(e_i)] * np.abs(cube64).max())
    # the adds of the pixels left out are there too, as products with g = 0: the counts are the sampled pixels' corners
    assert acc.count.sum() == 4 * sampled.sum()


# ------------------------------------------------------------------------------------------------------ the fixed tree
def hand_tree(term, smp):
    """one 32 x 32 tile by hand in numpy float32: a lane's four pixels left to right from +0, the xor butterfly, ((w0 + w1) + w2) + w3"""
    assert term.shape == (32, 32) and term.dtype == np.float32
    waves = []
    for w in range(4):
        v = np.zeros(64, np.float32)
        for lane in range(64):
            y, x4 = w * 8 + lane // 8, (lane % 8) * 4
            acc = np.float32(0)
            for k in range(4):
                if smp[y, x4 + k]:
                    acc = np.float32(acc + term[y, x4 + k])
            v[lane] = acc
        for o in (32, 16, 8, 4, 2, 1):
            v = (v + v[np.arange(64) ^ o]).astype(np.float32)
        assert (v.view(np.uint32) == v.view(np.uint32)[0]).all()  # float addition commutes: every lane ends with the same word
        waves.append(v[0])
    return np.float32(np.float32(np.float32(waves[0] + waves[1]) + waves[2]) + waves[3])


def test_gray_over_one_tile_is_the_hand_written_tree(tmp_path):
    rng = np.random.default_rng(9)
    N, C = 8, 3
    ids = hand_ids(rng, 32, 32, 20)
    ray = br.camera_block(32, 32, 1, 1.6)
    cube = cuberef.make_cube(4, N, C)
    g = rng.normal(0, 2, (C, 32, 32)).astype(np.float32)
    acc = br.Grad(cube.shape)
    row, term, smp = br.grad(tmp_path, cube, 20, ids, ray, g, acc)
    assert 300 < smp.sum() < 900
    want = np.float32([hand_tree(term[j], smp) for j in range(9)])
    assert np.array_equal(row.view(np.uint32), want.view(np.uint32))
    naive = term.sum((1, 2), dtype=np.float32)
    assert not np.array_equal(naive.view(np.uint32), want.view(np.uint32))  # (the order matters on these values)
    # the terms: gdir of cuberef on the computed directions, times 1, x, y
    d = br.dirs(tmp_path, ray, (32, 32))
    gd = cuberef.grad(tmp_path, cube, 1, np.ones((32, 32), np.uint32), d, g)
    y, x = np.mgrid[0:32, 0:32].astype(np.float32)
    for c in range(3):
        for r, m in enumerate((np.ones_like(x), x, y)):
            assert np.array_equal(term[3 * r + c][smp].view(np.uint32), (m * gd[c])[smp].view(np.uint32))
    assert (term[:, ~smp] == 0).all()
    # two tiles and two frames: tile order, then br_fold's frame order, each from +0
    ids2 = hand_ids(rng, 32, 64, 20)
    ray2 = br.camera_block(64, 32, 2, 1.6)
    g2 = rng.normal(0, 2, (C, 32, 64)).astype(np.float32)
    row2, term2, smp2 = br.grad(tmp_path, cube, 20, ids2, ray2, g2, br.Grad(cube.shape))
    for j in range(9):
        t0, t1 = hand_tree(np.ascontiguousarray(term2[j][:, :32]), smp2[:, :32]), hand_tree(np.ascontiguousarray(term2[j][:, 32:]), smp2[:, 32:])
        assert row2[j] == np.float32(np.float32(np.float32(0) + t0) + t1)
    both = br.fold(tmp_path, np.stack([row, row2]))
    assert np.array_equal(both, (np.float32(0) + row) + row2)
    # one sampled pixel in all: exactly its term (a term of -0 comes out +0)
    one = np.ones((32, 32), np.uint32)
    one[13, 21] = 0
    row1, term1, smp1 = br.grad(tmp_path, cube, 20, one, ray, g, br.Grad(cube.shape))
    assert smp1.sum() == 1 and np.array_equal(row1, term1[:, 13, 21] + np.float32(0))
