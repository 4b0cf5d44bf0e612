"""not-gpu: the silhouette antialiasing pass's test reference (tests/antialias_ref.c through tests/antialiasref.py) pinned to cases
worked out by hand, to central finite differences of its own double-precision restatement, and to the pair counts the GPU tests'
scenes must have."""
import numpy as np
import pytest

import antialiasref as ref
import visref
from support import frame, frame_positions, soup

TRI, BG = np.float32(8.0), np.float32(2.0)  # (dyadic: every blend below is exact)


def buffer_of(ids, z=None):
    v = np.zeros((4,) + ids.shape, np.uint32)
    v[0] = np.float32(np.where(ids != 0, 5.0, np.inf) if z is None else z).view(np.uint32)
    v[1] = ids
    return v


def edge_case(edge, tri_left, transposed, W=16, H=12):
    """one triangle whose straight side lies at coordinate `edge` across every row (column, when transposed) of the image and whose
    other two sides lie far outside it, on the left (top) or on the right (bottom) of that side → (pos [1, 9], vis words, planes)"""
    far = -200.0 if tri_left else 200.0
    p = np.float32([[edge, -16, 5], [edge, 48, 5], [far, 10, 5]])
    x = np.arange(W)[None, :].repeat(H, 0)
    own = (x <= 10) if tri_left else (x >= 11)
    if transposed:
        p = p[:, [1, 0, 2]]
        own = own[:W, :H].T if False else ((np.arange(H)[:, None].repeat(W, 1) <= 10) if tri_left else (np.arange(H)[:, None].repeat(W, 1) >= 11))
    ids = own.astype(np.uint32)
    return p.reshape(1, 9), buffer_of(ids), np.where(own, TRI, BG).astype(np.float32)[None]


@pytest.mark.parametrize("transposed", (False, True))
@pytest.mark.parametrize("tri_left", (True, False))
def test_quarter_pixel_edges(tmp_path, tri_left, transposed):
    """the side at 10.25: the triangle covers a quarter of pixel 10's footprint less than all of it (triangle on the left: t = 0.25,
    a = -0.25, target N = pixel 10) or a quarter of it (triangle on the right: N = pixel 11, s = -1, t = 0.75, a = 0.25, target
    F = pixel 10): either way pixel 10 moves 0.25 of the way to pixel 11's value and pixel 11 is unchanged.  The side at 10.75: pixel
    11 moves 0.25 of the way to pixel 10's value, pixel 10 is unchanged.  Every row, the border rows included."""
    W, H = (16, 12) if not transposed else (12, 16)
    for edge, moved in ((10.25, 10), (10.75, 11)):
        pos, v, c = edge_case(edge, tri_left, transposed, W, H)
        out = ref.forward(tmp_path, pos, 1, v, c)[0]
        want = c[0].copy()
        other = 21 - moved
        sl = (lambda i: (slice(None), i)) if not transposed else (lambda i: (i, slice(None)))
        want[sl(moved)] = c[0][sl(moved)] + np.float32(0.25) * (c[0][sl(other)] - c[0][sl(moved)])
        assert np.array_equal(out, want), (edge, out[:2] if transposed else out[:, 9:12])
        assert (out[sl(moved)] == (6.5 if (moved == 10) == tri_left else 3.5)).all()
        k = ref.counters(tmp_path, pos, 1, v)
        n = H if not transposed else W
        assert k["differ"] == n and k["target_n"] + k["target_f"] == n and k["f_nobody"] == n and k["interior"] == 0
        assert k["vertical" if transposed else "horizontal"] == n and k["target_n"] == (n if (moved == 10) == tri_left else 0)


def test_hand_gradient(tmp_path):
    """the triangle on the left, its side (corners 0 and 1, from y = -16 to y = 48) at x = 10.25: out[10] = tri + (0.5 - t)(bg - tri)
    with t = x_edge - 10 on row y, where the side's x is (1 - k) x0 + k x1, k = (16 + y) / 64.  So with gout = G at pixel 10 of every
    row: d L / d x0 = sum G (tri - bg)(1 - k), d L / d x1 = sum G (tri - bg) k; the side is vertical, so e = u1 - u0 = 0 and the y slots
    get exactly 0; corner 2 and the z slots get nothing.  gin: pixel 10 keeps 0.75 G, pixel 11 receives 0.25 G."""
    pos, v, c = edge_case(10.25, True, False)
    G = np.float32(4.0)
    gout = np.zeros_like(c)
    gout[0, :, 10] = G
    acc = ref.Grad(1)
    gin = ref.backward(tmp_path, pos, 1, v, c, gout, acc)
    k = (16 + np.arange(12)) / 64.0
    assert acc.gpos[0, 0, 0] == float(np.sum(4.0 * 6.0 * (1 - k))) and acc.gpos[0, 1, 0] == float(np.sum(4.0 * 6.0 * k))
    assert (acc.gpos[0, :, 1:] == 0).all() and (acc.gpos[0, 2] == 0).all()
    assert np.array_equal(acc.count[0], [[12, 12, 0], [12, 12, 0], [0, 0, 0]]) and np.array_equal(acc.gabs[0, :2, 0], acc.gpos[0, :2, 0])
    want = np.zeros_like(c)
    want[0, :, 10], want[0, :, 11] = 3.0, 1.0
    assert np.array_equal(gin, want)


def diagonal_pair(ulp=False):
    """T0 = (-.5,-.5) (15.5,-.5) (-.5,15.5) and T1 = (15.5,-.5) (15.5,15.5) (-.5,15.5) over a 16 x 16 image, one depth: pixels with
    x + y < 15 are T0's (no side lies on a sample row or column)"""
    pos = np.float32([[-.5, -.5, 5, 15.5, -.5, 5, -.5, 15.5, 5], [15.5, -.5, 5, 15.5, 15.5, 5, -.5, 15.5, 5]])
    if ulp:
        pos[1, 0] = np.nextafter(np.float32(15.5), np.float32(17))
    ys, xs = np.mgrid[0:16, 0:16]
    ids = np.where(xs + ys < 15, 1, 2).astype(np.uint32)
    return pos, buffer_of(ids), np.where(ids == 1, TRI, BG).astype(np.float32)[None], ids


def test_shared_diagonal_is_interior(tmp_path):
    """every differing pair straddles the diagonal; the depths tie, so N is the left / upper pixel, T0's; its edge (b, c) crosses the
    pair's line at t = 15 - x - y = 1, and both of its ends are corners of T1: interior, nothing blends.  With T1's copy of the
    vertex (15.5, -0.5) moved by one ulp the edge is shared no more: a = 0.5, the T1 pixel takes half of T0's colour."""
    pos, v, c, ids = diagonal_pair()
    assert np.array_equal(ref.forward(tmp_path, pos, 2, v, c), c)
    k = ref.counters(tmp_path, pos, 2, v)
    assert k["differ"] == 30 and k["interior"] == 30 and k["target_n"] + k["target_f"] == 0
    pos, v, c, ids = diagonal_pair(ulp=True)
    out = ref.forward(tmp_path, pos, 2, v, c)[0]
    ys, xs = np.mgrid[0:16, 0:16]
    on = xs + ys == 15
    assert (out[~on] == c[0][~on]).all() and (out[on] != c[0][on]).all()
    k = ref.counters(tmp_path, pos, 2, v)
    assert k["interior"] == 0 and k["target_f"] == 30


def test_nearer_pixel_ties_nan_and_nobody(tmp_path):
    """a 2 x 1 image; the active triangle has its side at x = 0.25 (pixel 0's if on the left, t = 0.25: pixel 0 moves) or, for the
    mirrored case, at x = 0.75 seen from pixel 1; the other triangle lies above the row and has no straddling edge: if it is taken
    for N nothing moves.  N is the right pixel only when its z is < the other's; ties and NaN give the left one; a nobody is always
    F whatever its z word says."""
    act_l = [0.25, -16, 5, 0.25, 48, 5, -200, 10, 5]   # covers pixel 0, side at 0.25
    act_r = [0.75, -16, 5, 0.75, 48, 5, 200, 10, 5]    # covers pixel 1, side at 0.75
    idle = [-5, -9, 5, 9, -9, 5, 0, -3, 5]
    c = np.float32([[[8, 2]]])
    nan, inf = np.nan, np.inf
    for tris, rows in (([act_l, idle], ((5, 5, True), (5, nan, True), (nan, 5, True), (5, 4, False), (4, 5, True), (-0.0, 0.0, True))),
                       ([idle, act_r], ((5, 5, False), (5, nan, False), (nan, 5, False), (5, 4, True), (inf, 5, True)))):
        pos = np.float32(tris)
        for za, zb, moves in rows:
            out = ref.forward(tmp_path, pos, 2, buffer_of(np.uint32([[1, 2]]), np.float32([[za, zb]])), c)
            assert (not np.array_equal(out, c)) == moves, (tris, za, zb, out)
    # upper / lower: the same, transposed
    posT = np.float32([act_l, idle]).reshape(2, 3, 3)[:, :, [1, 0, 2]].reshape(2, 9)
    cT = c.reshape(1, 2, 1)
    for za, zb, moves in ((5, 5, True), (5, nan, True), (5, 4, False)):
        out = ref.forward(tmp_path, posT, 2, buffer_of(np.uint32([[1], [2]]), np.float32([[za], [zb]])), cT)
        assert (not np.array_equal(out, cT)) == moves
    # nobody: F, even with a depth word in front of the owner's
    for ids, z, pos in (([[1, 0]], [[inf, -1.0]], [act_l]), ([[0, 1]], [[-inf, inf]], [act_r]), ([[1, 0x80000000]], [[5, 1]], [act_l]),
                        ([[1, 7]], [[5, 1]], [act_l])):
        out = ref.forward(tmp_path, np.float32(pos), 1, buffer_of(np.uint32(ids), np.float32(z)), c)
        want = [6.5, 2] if ids[0][0] == 1 else [8, 3.5]
        assert np.array_equal(out, np.float32([[want]])), (ids, out)
    # two nobodies, and two pixels of one triangle in either class: nothing
    for ids in ([[0, 9]], [[1, 1 | 0x80000000]]):
        assert np.array_equal(ref.forward(tmp_path, np.float32([act_l]), 1, buffer_of(np.uint32(ids), np.float32([[1, 2]])), c), c)


def test_borders_and_single_pixels(tmp_path):
    c = np.float32([[[3]]])
    assert np.array_equal(ref.forward(tmp_path, np.float32([[0.25, -16, 5, 0.25, 48, 5, -200, 10, 5]]), 1, buffer_of(np.uint32([[1]])), c), c)
    assert ref.counters(tmp_path, np.zeros((1, 9), np.float32), 1, buffer_of(np.uint32([[1]])))["differ"] == 0
    # the outline in the image's last column pair and last row pair
    pos = np.float32([[14.25, -16, 5, 14.25, 48, 5, -200, 10, 5]])
    ids = (np.arange(16)[None, :].repeat(3, 0) <= 14).astype(np.uint32)
    cc = np.where(ids == 1, TRI, BG).astype(np.float32)[None]
    out = ref.forward(tmp_path, pos, 1, buffer_of(ids), cc)[0]
    assert (out[:, 14] == 6.5).all() and (out[:, 15] == 2).all() and (out[:, :14] == 8).all()


def test_vertex_on_the_row_straddles_once(tmp_path):
    """a = (10.25, -16), b = (10.25, 4), c = (-200, 50): on row 4 vertex b has n = 0.  Edge (a, b) has n0 <= 0 but not n1 > 0, edge
    (b, c) has n0 <= 0 and n1 > 0: it alone straddles, k = 0, t = u_b = 0.25.  In the other winding (a, c, b) the edge (c, b) has
    n1 <= 0 and n0 > 0 and (b, a) neither.  One blended pair on the row either way, as on the rows above it."""
    ids = (np.arange(16)[None, :].repeat(5, 0) <= 10).astype(np.uint32)
    cc = np.where(ids == 1, TRI, BG).astype(np.float32)[None]
    for order in ((0, 1, 2), (0, 2, 1)):
        pos = np.float32([[10.25, -16, 5], [10.25, 4, 5], [-200, 50, 5]])[list(order)].reshape(1, 9)
        out = ref.forward(tmp_path, pos, 1, buffer_of(ids), cc)[0]
        assert (out[:, 10] == 6.5).all() and (out[:, 11] == 2).all()
        k = ref.counters(tmp_path, pos, 1, buffer_of(ids))
        assert k["target_n"] == 5 and k["no_edge"] == 0


# ------------------------------------------------------------------------------------------------------ finite differences
STEP = 2.0 ** -10  # pixels
FD_SEED = 4


def test_gradients_against_central_differences(tmp_path, orc):
    """L = sum gout * forward64(pos, in): gpos against central differences over every x and y of every triangle that receives a
    gradient, at a step of 2^-10 pixel, on the elements for which no pair's decision differs between the two ends of the step and
    the middle (at least 90 % of the non-zero elements); gin against central differences over every word of `in`.  Tolerance: 1e-4
    of the element's sum of |term| (the restatement is a rational function of the positions: the difference error is O(h^2))."""
    W, H, n = 48, 40, 30
    f = frame(soup(FD_SEED, n, W, H, ref.ZS), W, H)
    v = visref.Reference(tmp_path, f).expected(orc)[0]
    pos = frame_positions(f)
    rng = np.random.default_rng(5)
    c = rng.normal(0, 1, (3, H, W)).astype(np.float32)
    g = rng.normal(0, 1, (3, H, W)).astype(np.float32)
    acc = ref.Grad(n)
    gin, mag = ref.backward(tmp_path, pos, n, v, c, g, acc, want_abs=True)
    assert acc.counters["target_n"] > 50 and acc.counters["target_f"] > 50
    P, c64, g64 = pos.astype(np.float64), c.astype(np.float64), g.astype(np.float64)
    out0, dec0 = ref.forward64(tmp_path, P, n, v, c64)
    assert np.abs(out0 - ref.forward(tmp_path, pos, n, v, c)).max() < 1e-4

    def loss(p):
        out, dec = ref.forward64(tmp_path, p, n, v, c64)
        return float((out * g64).sum()), dec
    nz = acc.gabs > 0
    assert not nz[:, :, 2].any() and (acc.gpos[:, :, 2] == 0).all()
    kept = bad = 0
    worst = 0.0
    for t, k, x in np.argwhere(nz):
        hi, lo = P.copy(), P.copy()
        hi[t, 3 * k + x] += STEP
        lo[t, 3 * k + x] -= STEP
        (lh, dh), (ll, dl) = loss(hi), loss(lo)
        if not (np.array_equal(dh, dec0) and np.array_equal(dl, dec0)):
            continue
        kept += 1
        gap = abs((lh - ll) / (2 * STEP) - acc.gpos[t, k, x]) / acc.gabs[t, k, x]
        worst = max(worst, gap)
        bad += gap > 1e-4
    print(f"gpos: {kept} of {int(nz.sum())} non-zero elements kept, worst gap {worst:.3e} of sum |term|")
    assert kept >= 0.9 * nz.sum() and bad == 0
    # gin: the forward is linear in `in`, one channel at a time does
    worst = 0.0
    for ch in range(3):
        for y in range(H):
            for x in range(W):
                hi, lo = c64.copy(), c64.copy()
                hi[ch, y, x] += STEP
                lo[ch, y, x] -= STEP
                d = ((ref.forward64(tmp_path, P, n, v, hi[ch:ch + 1])[0] - ref.forward64(tmp_path, P, n, v, lo[ch:ch + 1])[0]) * g64[ch]).sum() / (2 * STEP)
                worst = max(worst, abs(d - gin[ch, y, x]) / mag[ch, y, x])
    print(f"gin: worst gap {worst:.3e} of sum |term|")
    assert worst <= 1e-4


# ------------------------------------------------------------------------------------------------------ the GPU tests' scenes
@pytest.mark.parametrize("backdrop", (True, False))
@pytest.mark.parametrize("w,h,n", ref.SIZES)
def test_counts_on_the_gpu_tests_scenes(tmp_path, orc, w, h, n, backdrop):
    """the oracle's visibility buffer of every scene tests/test_gpu_antialias.py runs has the pairs that test relies on (the GPU's
    own buffer is held to the oracle's by tests/test_gpu_visibility.py)"""
    t = ref.scene_tris(w, h, n, backdrop)
    f = frame(t, w, h)
    v = visref.Reference(tmp_path, f).expected(orc)[0]
    k = ref.counters(tmp_path, frame_positions(f), len(t), v)
    print(w, h, backdrop, k)
    for name in ref.relied_on(w, h, backdrop):
        assert k[name] > 0, (name, k)
    if w == 1 and h == 1:
        assert k["differ"] == 0
