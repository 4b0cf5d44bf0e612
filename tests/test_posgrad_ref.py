"""not-gpu: the position gradient's test reference (tests/posgrad_ref.c through tests/posgradref.py) pinned to a case worked out by
hand and to central finite differences in float64 numpy, ownership held fixed."""
import functools

import numpy as np

import posgradref
from support import bits

STEP = 2.0 ** -10  # pixels
# the worst gaps between the reference and the finite differences, measured on the CPU over measure()'s six scenes (relative to the
# scales the two tests name); the asserted tolerances are ten times these, and never looser than 1e-3
GAP_POS, GAP_PIX = 3.37e-6, 2.19e-7
TOL_POS, TOL_PIX = min(10 * GAP_POS, 1e-3), min(10 * GAP_PIX, 1e-3)


def buffer_of(ids, al, be):
    v = np.zeros((4,) + ids.shape, np.uint32)
    v[1], v[2], v[3] = ids, np.float32(al).view(np.uint32), np.float32(be).view(np.uint32)
    return v


def test_hand_case(tmp_path):
    """A = (0, 0), B = (16, 0), C = (0, 16): area = 16 * 16 - 0 * 0 = 256, r = 1 / 256,
    grad alpha = (by - cy, cx - bx) / area = (-16, -16) / 256, grad beta = (cy - ay, ax - cx) / area = (16, 0) / 256.
    The pixel at (8, 4): alpha = 1 - 8/16 - 4/16 = 1/4, beta = 8/16 = 1/2, gamma = 1/4.
    (a) dalpha = 32, dbeta = 16, no gz:
        gx = (32 * -16 + 16 * 16) / 256 = -1;  gy = (32 * -16 + 16 * 0) / 256 = -2
        corner k gets -w_k * (gx, gy): A (1/4, 1/2), B (1/2, 1), C (1/4, 1/2); the z slots get nothing.
    (b) the same with gz = 8 and z = (1, 3, 7): da = 32 + 8 * (1 - 7) = -16, db = 16 + 8 * (3 - 7) = -16
        gx = (-16 * -16 + -16 * 16) / 256 = 0;  gy = (-16 * -16 + -16 * 0) / 256 = 1
        A (-0, -1/4, 1/4 * 8 = 2), B (-0, -1/2, 4), C (-0, -1/4, 2).
    (c) gz = 8 alone: da = 8 * -6 = -48, db = 8 * -4 = -32: gx = (-48 * -16 + -32 * 16) / 256 = 1, gy = (-48 * -16) / 256 = 3
        A (-1/4, -3/4, 2), B (-1/2, -3/2, 4), C (-1/4, -3/4, 2).
    An S pixel has the same values here (gamma = 1 - 1/4 - 1/2 is exact either way)."""
    pos = np.float32([[0, 0, 1, 16, 0, 3, 0, 16, 7]])
    gb, gz = np.float32([32, 16]).reshape(2, 1, 1), np.float32([8]).reshape(1, 1, 1)
    for word in (1, 1 | 0x80000000):
        v = buffer_of(np.uint32([[word]]), [[0.25]], [[0.5]])
        for kw, gpix, gpos in ((dict(gbary=gb), (-1, -2), [[.25, .5, 0], [.5, 1, 0], [.25, .5, 0]]),
                               (dict(gbary=gb, gz=gz), (0, 1), [[0, -.25, 2], [0, -.5, 4], [0, -.25, 2]]),
                               (dict(gz=gz), (1, 3), [[-.25, -.75, 2], [-.5, -1.5, 4], [-.25, -.75, 2]])):
            acc = posgradref.Grad(1)
            px = posgradref.grad(tmp_path, pos, 1, v, into=acc, **kw)
            assert np.array_equal(px.reshape(2), np.float32(gpix)), (kw.keys(), px)
            assert np.array_equal(acc.gpos[0], np.float64(gpos)), (kw.keys(), acc.gpos)
            assert acc.count[0] == 1 and np.array_equal(acc.gabs[0], np.abs(np.float64(gpos)))
    # nobody: 0 when fused, the words stay when not; nothing is added
    for word in (0, 0x80000000, 2, 0xffffffff):
        v = buffer_of(np.uint32([[word]]), [[0.25]], [[0.5]])
        acc = posgradref.Grad(1)
        pre = np.full((2, 1, 1), 0xdeadbeef, np.uint32)
        assert (bits(posgradref.grad(tmp_path, pos, 1, v, gbary=gb, gz=gz, into=acc, prefill=pre)) == 0).all()
        assert (bits(posgradref.grad(tmp_path, pos, 1, v, gbary=gb, gz=gz, into=acc, fused=False, prefill=pre)) == 0xdeadbeef).all()
        assert (acc.gpos == 0).all() and acc.count[0] == 0


def scene(seed, T=40, H=48, W=64):
    """T triangles with coordinates within +-128 and |area| >= 8, either winding; every pixel of an H x W buffer owned by one of
    them (ownership is held fixed, so any assignment will do: a pixel need not lie inside its owner), either class; alpha and beta
    from the cross products in float64 at the pixel's integer corner, rounded to float32"""
    rng = np.random.default_rng([seed, 41])
    pos = np.zeros((T, 3, 3))
    for t in range(T):
        while True:
            xy = np.round(rng.uniform(-128, 128, (3, 2)) * 16) / 16
            area = (xy[1, 0] - xy[0, 0]) * (xy[2, 1] - xy[0, 1]) - (xy[1, 1] - xy[0, 1]) * (xy[2, 0] - xy[0, 0])
            if abs(area) >= 8:
                break
        pos[t, :, :2], pos[t, :, 2] = xy, rng.uniform(1, 50, 3)
    pos = pos.astype(np.float32)
    tri = rng.integers(0, T, (H, W))
    ids = (tri + 1).astype(np.uint32) | ((rng.random((H, W)) < 0.4).astype(np.uint32) << 31)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    al, be, _ = bary64(pos.astype(np.float64)[tri], xs, ys)
    return pos, tri, buffer_of(ids, al, be), xs, ys


def bary64(P, x, y):
    """alpha, beta and z at (x, y) of triangles P [..., 3, 3] in float64: the cross products over the area"""
    ax, ay, bx, by, cx, cy = P[..., 0, 0], P[..., 0, 1], P[..., 1, 0], P[..., 1, 1], P[..., 2, 0], P[..., 2, 1]
    area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    al = ((bx - x) * (cy - y) - (by - y) * (cx - x)) / area
    be = ((x - ax) * (cy - ay) - (y - ay) * (cx - ax)) / area
    return al, be, al * P[..., 0, 2] + be * P[..., 1, 2] + (1 - al - be) * P[..., 2, 2]


def loss64(P, tri, xs, ys, ga, gb, gz):
    """per pixel: ga alpha + gb beta + gz z, the positions P [T, 3, 3] float64"""
    al, be, z = bary64(P[tri], xs, ys)
    return ga * al + gb * be + gz * z


@functools.lru_cache(None)
def _measure(tmp_path, seeds):
    worst_pos = worst_pix = 0.0
    for seed in seeds:
        pos, tri, v, xs, ys = scene(seed)
        T = len(pos)
        rng = np.random.default_rng([seed, 43])
        for use_b, use_z in ((True, False), (False, True), (True, True)):
            gbary = rng.normal(0, 2, (2,) + tri.shape).astype(np.float32) if use_b else None
            gz = rng.normal(0, 2, (1,) + tri.shape).astype(np.float32) if use_z else None
            acc = posgradref.Grad(T)
            gpix = posgradref.grad(tmp_path, pos, T, v, gbary=gbary, gz=gz, into=acc)
            ga, gb = (gbary[0].astype(np.float64), gbary[1].astype(np.float64)) if use_b else (0.0, 0.0)
            g = gz[0].astype(np.float64) if use_z else 0.0
            P = pos.astype(np.float64)
            # ---- d L / d pos: one float at a time, every triangle at once (a triangle's pixels see only their own owner move)
            fd = np.zeros((T, 3, 3))
            for k in range(3):
                for c in range(3):
                    hi, lo = P.copy(), P.copy()
                    hi[:, k, c] += STEP
                    lo[:, k, c] -= STEP
                    d = (loss64(hi, tri, xs, ys, ga, gb, g) - loss64(lo, tri, xs, ys, ga, gb, g)) / (2 * STEP)
                    np.add.at(fd[:, k, c], tri.ravel(), d.ravel())
            scale = acc.gabs.reshape(T, 9).max(1)[:, None, None]
            assert (scale > 0).all()
            if not use_z:
                assert (acc.gpos[:, :, 2] == 0).all() and (acc.gabs[:, :, 2] == 0).all()
            worst_pos = max(worst_pos, float((np.abs(acc.gpos - fd) / scale).max()))
            # ---- d L / d (sample point)
            fx = (loss64(P, tri, xs + STEP, ys, ga, gb, g) - loss64(P, tri, xs - STEP, ys, ga, gb, g)) / (2 * STEP)
            fy = (loss64(P, tri, xs, ys + STEP, ga, gb, g) - loss64(P, tri, xs, ys - STEP, ga, gb, g)) / (2 * STEP)
            Pt = P[tri]
            area = (Pt[..., 1, 0] - Pt[..., 0, 0]) * (Pt[..., 2, 1] - Pt[..., 0, 1]) - (Pt[..., 1, 1] - Pt[..., 0, 1]) * (Pt[..., 2, 0] - Pt[..., 0, 0])
            da = np.abs(ga + g * (Pt[..., 0, 2] - Pt[..., 2, 2])) + np.abs(gb + g * (Pt[..., 1, 2] - Pt[..., 2, 2]))
            edge = np.abs(Pt[..., :, :2] - np.roll(Pt[..., :, :2], 1, -2)).max((-1, -2))
            pscale = da * edge / np.abs(area)
            worst_pix = max(worst_pix, float((np.abs(gpix[0] - fx) / pscale).max()), float((np.abs(gpix[1] - fy) / pscale).max()))
    return worst_pos, worst_pix


def measure(tmp_path):
    return _measure(str(tmp_path), tuple(range(6)))  # (computed once, shared by the two tests)


def test_gpos_against_central_differences(tmp_path):
    """L(pos) = sum over the owned pixels of ga alpha(pos) + gb beta(pos) + gz z(pos), alpha and beta recomputed in float64 from the
    perturbed positions by the cross products, ownership fixed; d L / d pos by central differences at a step of 2^-10 pixel against
    the reference's gpos, with gbary only, gz only and both.  The gap is taken relative to the triangle's largest sum of |term|.
    Measured worst gap: 3.37e-6 (the float32 rounding of alpha, beta and r: seed-dependent); asserted: ten times that.  A sign or an
    index error is a gap of order 1."""
    worst, _ = measure(tmp_path)
    print(f"worst gap of gpos {worst:.3e}, tolerance {TOL_POS:.3e}")
    assert worst <= TOL_POS


def test_gpix_against_central_differences(tmp_path):
    """the same loss per pixel as a function of the sample point; alpha, beta and z are affine in it, so the difference quotient is
    exact up to float64 rounding.  The gap is taken relative to (|da| + |db|) * the longest edge extent / |area|.  Measured worst
    gap: 2.19e-7; asserted: ten times that."""
    _, worst = measure(tmp_path)
    print(f"worst gap of gpix {worst:.3e}, tolerance {TOL_PIX:.3e}")
    assert worst <= TOL_PIX
