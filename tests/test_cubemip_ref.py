"""not-gpu: pins tests/cubemip_ref.c, the reference the GPU tests of the mipmapped cube lookup compare against: known answers worked
out by hand on a 2 x 2 cube with two levels (a face centre, an edge, a vertex; every clamp of the level), bit-equality with
tests/cuberef.py at one level, the binary64 build of the same text against float64 autograd of a plain-torch restatement and against
central differences, the constant-pyramid identity, and the footprint level at power-of-two footprints."""
import numpy as np
import pytest
import torch

import cubemipref
import cuberef

NAN, INF = np.float32(np.nan), np.float32(np.inf)
LAMS = np.float32([-1, 0, 0.5, 1, 2, NAN, INF])


def ones_ids(n):
    return np.ones((1, n), np.uint32)


def planes(d):
    """[n, 3] → [3, 1, n]"""
    return np.ascontiguousarray(np.asarray(d).T.reshape(3, 1, -1))


# ------------------------------------------------------------------------------------------------------ known answers
def kat_levels():
    """level 0: texel (face f, row y, column x) = 64 f + 16 (2 y + x) in channel 0 and its negative in channel 1; level 1: its own
    numbers 1000 + 8 f (NOT the box filter: the lookup takes whatever pyramid it is handed)"""
    l0 = np.zeros((6, 2, 2, 2), np.float32)
    for f in range(6):
        for y in range(2):
            for x in range(2):
                l0[f, y, x] = (64 * f + 16 * (2 * y + x), -(64 * f + 16 * (2 * y + x)))
    l1 = np.zeros((6, 1, 1, 2), np.float32)
    for f in range(6):
        l1[f, 0, 0] = (1000 + 8 * f, -(1000 + 8 * f))
    return [l0, l1]


def kat_expected():
    """(c_0, c_1) of channel 0 per direction, from include/srz.h's rule by hand.
    centre (1, 0, 0): +X, s = t = 0 -> level 0: fx = fy = 0.5, the four texels of +X at weight 1/4; level 1: fx = 0, tx = 0: its texel.
    edge (1, 1, 0): a tie, so +X; s = -0, t = -1 -> level 0: x0 = 0, tx = 1/2; fy = -1/2, y0 = -1, ty = 1/2: row -1 crosses to +Y at
      (column N - 1, row N - 1 - i): +Y[1][1] for x = 0 and +Y[0][1] for x = 1; row 0 is +X[0][0], +X[0][1].  level 1: tx = 0, x0 = 0;
      y0 = -1, ty = 1/2: +Y[0][0] and +X[0][0] at weight 1/2 (x1 = 1 has weight 0).
    vertex (1, 1, 1): +X; s = t = -1 -> x0 = y0 = -1, tx = ty = 1/2: (y -1, x -1) lies outside in both: row clamped to 0, then x = -1
      crosses to +Z at (N - 1, i = 0): +Z[0][1]; (y -1, x 0) -> +Y[1][1]; (y 0, x -1) -> +Z[0][1]; (y 0, x 0) -> +X[0][0].  level 1
      likewise with N = 1: +Z, +Y, +Z, +X."""
    t = lambda f, y, x: 64 * f + 16 * (2 * y + x)  # noqa: E731
    u = lambda f: 1000 + 8 * f  # noqa: E731
    return {(1, 0, 0): ((t(0, 0, 0) + t(0, 0, 1) + t(0, 1, 0) + t(0, 1, 1)) / 4, u(0)),
            (1, 1, 0): ((t(2, 1, 1) + t(2, 0, 1) + t(0, 0, 0) + t(0, 0, 1)) / 4, (u(2) + u(0)) / 2),
            (1, 1, 1): ((2 * t(4, 0, 1) + t(2, 1, 1) + t(0, 0, 0)) / 4, (2 * u(4) + u(2) + u(0)) / 4)}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_known_answers_by_hand(tmp_path, dtype):
    levels = kat_levels()
    for d, (c0, c1) in kat_expected().items():
        dirs = np.repeat(np.float32([d]), len(LAMS), 0)
        out = cubemipref.sample(tmp_path, levels, dirs, LAMS, dtype=dtype)
        want = [c0, c0, c0 + 0.5 * (c1 - c0), c1, c1, c0, c1]  # -1, 0, 0.5, 1, 2, NaN, +inf
        assert out[:, 0].tolist() == want and out[:, 1].tolist() == [-x for x in want], (d, out[:, 0])
        g = np.zeros((2, 1, len(LAMS)), dtype)
        g[0], g[1] = 3, 1  # glam = 3 (c1 - c0) + 1 (-(c1 - c0)) where 0 <= lam < 1
        acc = cubemipref.Grad(2, 2, 2)
        gdir, glam = cubemipref.grad(tmp_path, levels, 1, ones_ids(len(LAMS)), planes(dirs), LAMS.reshape(1, -1), g, acc, dtype=dtype)
        assert glam[0].tolist() == [0, 2 * (c1 - c0), 2 * (c1 - c0), 0, 0, 0, 0], (d, glam)
        # the level weights: level 0 gets 1 from lam -1, 0, NaN and 1/2 from 0.5; level 1 gets 1 from 1, 2, inf and 1/2 from 0.5;
        # gout's channel 0 is 3 everywhere and the four corner weights of a level sum to 1
        assert acc.level(acc.g, 0)[..., 0].sum() == 3 * 3.5 and acc.level(acc.g, 1)[..., 0].sum() == 3 * 3.5
        assert acc.level(acc.count, 0).sum() == 4 * 4 and acc.level(acc.count, 1).sum() == 4 * 4  # no add to level 1 at f == 0
    # the minus zero is a zero with a right-hand derivative; unsampled directions write zeros and add nothing
    dirs = np.float32([(1, 0, 0), (NAN, 0, 0), (0, 0, 0), (0, -0.0, INF)])
    lam = np.float32([-0.0, 0.5, 0.5, 0.5]).reshape(1, -1)
    acc = cubemipref.Grad(2, 2, 2)
    gdir, glam = cubemipref.grad(tmp_path, levels, 1, ones_ids(4), planes(dirs), lam, np.ones((2, 1, 4), dtype), acc, dtype=dtype)
    assert glam[0, 0] == 0 and (glam[0, 1:] == 0).all() and (gdir[:, 0, 1:] == 0).all()  # (1 - 1) (c1 - c0) = 0, but computed:
    gl = cubemipref.grad(tmp_path, levels, 1, ones_ids(1), planes(dirs[:1]), lam[:, :1], np.asarray([[[1]], [[0]]], dtype), dtype=dtype)[1]
    assert gl[0, 0] == 1000 - 24
    assert acc.count.sum() == 4 and (cubemipref.sample(tmp_path, levels, dirs, lam, dtype=dtype)[1:] == 0).all()


def test_nobody_and_the_fused_clear(tmp_path):
    levels = kat_levels()
    ids = np.uint32([[0, 1, 0x80000001, 2, 0x80000000, 0xffffffff]])
    d = planes(np.float32([(1, 0, 0)] * 6))
    lam = np.full((1, 6), 0.5, np.float32)
    pre = np.full((2, 1, 6), 0xdeadbeef, np.uint32)
    for fused in (True, False):
        out = cubemipref.forward(tmp_path, levels, 1, ids, d, lam, fused, pre).view(np.uint32)
        nobody = np.array([True, False, False, True, True, True])
        assert (out[:, 0, nobody] == (0 if fused else 0xdeadbeef)).all() and (out[:, 0, ~nobody] != 0xdeadbeef).all()
        gdir, glam = cubemipref.grad(tmp_path, levels, 1, ids, d, lam, np.ones((2, 1, 6), np.float32), fused=fused, prefill=0xdeadbeef)
        assert (glam.view(np.uint32)[0, nobody] == (0 if fused else 0xdeadbeef)).all()
        assert (gdir.view(np.uint32)[:, 0, nobody] == (0 if fused else 0xdeadbeef)).all()


# ------------------------------------------------------------------------------------------------------ one level: the flat lookup
@pytest.mark.parametrize("N", cuberef.CUBE_SIZES)
def test_one_level_is_the_flat_reference_bit_for_bit(tmp_path, N):
    rng = np.random.default_rng([N, 3])
    h, w, C, tris = 40, 48, 5, 9
    ids = rng.integers(0, tris + 2, (h, w)).astype(np.uint32)
    dirs = cuberef.hostile_dirs(rng, (h, w), N)
    cube = cuberef.make_cube(2, N, C)
    gout = rng.normal(0, 2, (C, h, w)).astype(np.float32)
    lam = cubemipref.hostile_lam(rng, (h, w), 1)  # ignored at one level, whatever it holds
    for lm in (None, lam):
        a = cubemipref.forward(tmp_path, [cube], tris, ids, dirs, lm)
        b = cuberef.forward(tmp_path, cube, tris, ids, dirs)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        acc, ref = cubemipref.Grad(N, C, 1), cuberef.Grad(cube.shape)
        gdir, glam = cubemipref.grad(tmp_path, [cube], tris, ids, dirs, lm, gout, acc)
        want = cuberef.grad(tmp_path, cube, tris, ids, dirs, gout, ref)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(gdir), nan) and np.array_equal(gdir.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
        assert (glam == 0).all()
        assert np.array_equal(acc.g, ref.gtex.ravel()) and np.array_equal(acc.gabs, ref.gabs.ravel()) and np.array_equal(acc.count, ref.count.ravel())


def test_pyramid_build_and_classification(tmp_path):
    assert [cubemipref.n_levels(n) for n in (1, 2, 5, 6, 8, 64, 96)] == [1, 2, 1, 2, 4, 7, 6]
    cube = cuberef.make_cube(1, 8, 3)
    lv = cubemipref.build(cube)
    assert [l.shape for l in lv] == [(6, 8, 8, 3), (6, 4, 4, 3), (6, 2, 2, 3), (6, 1, 1, 3)]
    assert lv[1][3, 1, 2, 0] == np.float32(np.float32(cube[3, 2, 4, 0] + cube[3, 2, 5, 0]) + np.float32(cube[3, 3, 4, 0] + cube[3, 3, 5, 0])) * np.float32(0.25)
    # the clamps and the fraction; an edge crossed at a level above 0
    d = planes(np.float32([(1, 0.99, 0)] * 6))
    lam = np.float32([[NAN, -2, 0.25, 2.5, 3, 7]])
    cls, face, l0, f = cubemipref.classify(tmp_path, 8, 4, 1, ones_ids(6), d, lam)
    C = cubemipref
    assert (cls[0] & C.CLAMP_LOW != 0).tolist() == [True, True, False, False, False, False]
    assert (cls[0] & C.CLAMP_HIGH != 0).tolist() == [False, False, False, False, True, True]
    assert (cls[0] & C.FRACTIONAL != 0).tolist() == [False, False, True, True, False, False]
    assert l0[0].tolist() == [0, 0, 0, 2, 3, 3] and f[0].tolist() == [0, 0, 0.25, 0.5, 0, 0] and (face == 0).all()
    assert (cls[0] & C.CROSSED_ABOVE0 != 0).tolist() == [False, False, True, True, True, True]  # (level 0 alone does not count)


def test_a_constant_pyramid_gives_the_constant_for_any_level(tmp_path):
    rng = np.random.default_rng(8)
    N, L, C = 8, 4, 3
    const = np.float32([1.7, -3e30, 2.0 ** -140])
    levels = [np.broadcast_to(const, (6, N >> l, N >> l, C)).copy() for l in range(L)]
    dirs = cuberef.hostile_dirs(rng, (60, 70), N)
    lam = cubemipref.hostile_lam(rng, (60, 70), L)
    ids = np.ones((60, 70), np.uint32)
    out = cubemipref.forward(tmp_path, levels, 1, ids, dirs, lam)
    cls = cubemipref.classify(tmp_path, N, L, 1, ids, dirs, lam)[0]
    smp = (cls & cubemipref.SAMPLED) != 0
    assert smp.sum() > 3000 and ((cls & cubemipref.FRACTIONAL) != 0).sum() > 500
    for ch in range(C):
        assert (out[ch][smp] == const[ch]).all() and (out[ch][~smp] == 0).all()
    gdir, glam = cubemipref.grad(tmp_path, levels, 1, ids, dirs, lam, np.ones((C, 60, 70), np.float32))
    assert (glam == 0).all()


# ------------------------------------------------------------------------------------------------------ float64: autograd, differences
def torch_lookup(tmp_path, levels, d, lam):
    """the rule restated in plain torch float64 — the face, the floors and the resolved texels held fixed (integers), everything
    else differentiable: d [n, 3], lam [n], levels: list of [6, N_l, N_l, C] tensors → [n, C]"""
    L, n = len(levels), d.shape[0]
    dn = d.detach().numpy()
    m = np.where((np.abs(dn[:, 0]) >= np.abs(dn[:, 1])) & (np.abs(dn[:, 0]) >= np.abs(dn[:, 2])), 0, np.where(np.abs(dn[:, 1]) >= np.abs(dn[:, 2]), 1, 2))
    face = 2 * m + (dn[np.arange(n), m] <= 0)
    ax = np.array(cuberef.AXES, np.float64)  # [face][n, su, sv][3]
    nrm, su, sv = (torch.as_tensor(ax[face, k]) for k in range(3))
    ma = (d * nrm).sum(1)
    s, t = (d * su).sum(1) / ma, (d * sv).sum(1) / ma

    def sample(l):
        N = levels[l].shape[1]
        fx, fy = (s * 0.5 + 0.5) * N - 0.5, (t * 0.5 + 0.5) * N - 0.5
        x0, y0 = torch.floor(fx).detach(), torch.floor(fy).detach()
        tx, ty = fx - x0, fy - y0
        flat = levels[l].reshape(-1, levels[l].shape[-1])
        tex = []
        for k in range(4):
            at = [cuberef.resolve(tmp_path, N, int(face[i]), int(x0[i]) + (k & 1), int(y0[i]) + (k >> 1))[0] for i in range(n)]
            tex.append(flat[torch.as_tensor([(g * N + y) * N + x for g, x, y in at])])
        top, bot = tex[0] + tx[:, None] * (tex[1] - tex[0]), tex[2] + tx[:, None] * (tex[3] - tex[2])
        return top + ty[:, None] * (bot - top)
    lc = lam.detach().numpy()
    l0 = np.where(lc > 0, np.minimum(np.floor(np.where(lc > 0, lc, 0)), L - 1), 0).astype(int)
    inside = (lc >= 0) & (lc < L - 1)
    f = torch.where(torch.as_tensor(inside), lam - torch.as_tensor(l0.astype(np.float64)), torch.zeros_like(lam))
    per = [sample(l) for l in range(L)]
    idx = torch.arange(n)
    c0 = torch.stack(per)[torch.as_tensor(l0), idx]
    c1 = torch.stack(per)[torch.as_tensor(np.minimum(l0 + 1, L - 1)), idx]
    return c0 + f[:, None] * (c1 - c0)


@pytest.mark.parametrize("N,L", [(8, 4), (6, 2), (64, 3)])
def test_binary64_build_against_float64_autograd(tmp_path, N, L):
    """the binary64 build of cubemip_ref.c against torch.autograd of the restatement above: out, gdir, glam and the pyramid's gradient.
    Both sides evaluate the same real function in binary64, in another order of operations and with or without fused multiply-adds;
    each has a few dozen roundings of 2^-53 relative to intermediates no larger than `scale` below, so 2^-40 scale leaves two orders
    of magnitude to spare and is eight orders below anything a wrong term would give."""
    rng = np.random.default_rng([N, L])
    n, C = 160, 3
    d = rng.normal(0, 1, (n, 3))
    d[:40] = cuberef.edge_dirs()[0][rng.integers(0, 348, 40)] * (1 + rng.uniform(-1e-3, 1e-3, (40, 3)))  # around the edges
    lam = rng.uniform(-0.5, L - 0.5, n)
    lam[:12] = np.repeat(np.arange(L), 12 // L + 1)[:12]  # integers: the right-hand derivative
    levels = [rng.normal(0, 3, (6, N >> l, N >> l, C)) for l in range(L)]
    g = rng.normal(0, 2, (n, C))
    td, tl = torch.tensor(d, requires_grad=True), torch.tensor(lam, requires_grad=True)
    tlev = [torch.tensor(l, requires_grad=True) for l in levels]
    out = torch_lookup(tmp_path, tlev, td, tl)
    (out * torch.as_tensor(g)).sum().backward()
    gout = np.ascontiguousarray(g.T.reshape(C, 1, n))
    got = cubemipref.sample(tmp_path, levels, d, lam, dtype=np.float64)
    acc = cubemipref.Grad(N, C, L)
    gdir, glam = cubemipref.grad(tmp_path, levels, 1, ones_ids(n), planes(d), lam.reshape(1, -1), gout, acc, dtype=np.float64)
    tmax = max(np.abs(l).max() for l in levels)
    eps = 2.0 ** -40
    assert np.abs(got - out.detach().numpy()).max() <= eps * tmax
    gsum, ma = np.abs(g).sum(1), np.abs(d).max(1)
    assert (np.abs(glam[0] - tl.grad.numpy()) <= eps * 2 * tmax * gsum).all() and (glam[0] != 0).sum() > n // 4
    assert (np.abs(gdir[:, 0].T - td.grad.numpy()) <= eps * (4 * N * tmax * gsum / ma)[:, None]).all() and (gdir != 0).sum() > n
    for l in range(L):
        assert np.abs(acc.level(acc.g, l) - tlev[l].grad.numpy()).max() <= eps * gsum.sum()


@pytest.mark.parametrize("N,L", [(8, 4), (64, 7)])
def test_gradients_against_central_differences(tmp_path, N, L):
    """glam and gdir of the binary64 build against central differences of its own forward, away from the kinks (integer levels, texel
    borders at either level read, face changes).  In lam the lookup is piecewise linear: the difference quotient is exact up to
    rounding.  In d it is smooth within a texel cell: with step h = 2^-20 ma the truncation error is below h^2 times a third
    derivative of order N^3 / ma^3 — relative 2^-40 N^2 — and the rounding error about 2^-53 / 2^-20; 2^-24 scale covers both."""
    rng = np.random.default_rng([N, L, 5])
    C = 2
    levels = [rng.normal(0, 3, (6, N >> l, N >> l, C)) for l in range(L)]
    d = rng.normal(0, 1, (4000, 3))
    lam = rng.uniform(0.05, L - 1.05, 4000)
    lam = np.floor(lam) + np.clip(lam - np.floor(lam), 0.05, 0.95)
    ma = np.abs(d).max(1)
    st = np.sort(np.abs(d), 1)[:, :2] / ma[:, None]
    keep = (st < 0.9).all(1)
    for l in range(L):  # away from every level's texel borders (a superset of the two levels read)
        fx = (np.concatenate([st, -st], 1) * 0.5 + 0.5) * (N >> l) - 0.5
        keep &= (np.abs(fx - np.round(fx)) > 0.02).all(1)
    d, lam, ma = d[keep][:200], lam[keep][:200], ma[keep][:200]
    n = len(d)
    assert n >= 100
    g = rng.normal(0, 2, (n, C))
    F = lambda dd, ll: (cubemipref.sample(tmp_path, levels, dd, ll, dtype=np.float64) * g).sum(1)  # noqa: E731
    gdir, glam = cubemipref.grad(tmp_path, levels, 1, ones_ids(n), planes(d), lam.reshape(1, -1), np.ascontiguousarray(g.T.reshape(C, 1, n)),
                                 dtype=np.float64)
    tmax, gsum = max(np.abs(l).max() for l in levels), np.abs(g).sum(1)
    h = 2.0 ** -10
    assert (np.abs((F(d, lam + h) - F(d, lam - h)) / (2 * h) - glam[0]) <= 2.0 ** -24 * tmax * gsum).all() and (glam != 0).all()
    for c in range(3):
        e = np.zeros((n, 3))
        e[:, c] = 2.0 ** -20 * ma
        fd = (F(d + e, lam) - F(d - e, lam)) / (2 * e[:, c])
        assert (np.abs(fd - gdir[c, 0]) <= 2.0 ** -24 * N ** 3 * tmax * gsum / ma).all(), c
    assert (np.abs((gdir[:, 0].T * d).sum(1)) <= 2.0 ** -40 * N * tmax * gsum).all()  # the lookup does not depend on the length


# ------------------------------------------------------------------------------------------------------ the footprint level
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cube_level_at_power_of_two_footprints(tmp_path, dtype):
    """a footprint of exactly 2^k texels of level 0 gives lam = k, clamped to L - 1; below one texel 0.  One texel of an N-texel face
    is 2 / N in s: on +X with ma = 1 and d/dx of z = -2^k 2 / N, sx = 2^k 2 / N and ax = 2^k exactly; likewise on -Y through t in y."""
    N, L = 64, 7
    ks = np.arange(-2, 10)
    n = len(ks)
    for d, comp, sign, step in (((1, 0, 0), 2, -1, 0), ((0, -4, 0), 2, -4, 1), ((0.5, 0.25, -2), 0, -2, 0)):
        dirs = planes(np.float32([d] * n))
        dd = np.zeros((6, 1, n), dtype)
        dd[2 * comp + step, 0] = sign * 2.0 ** ks * 2 / N
        lam, l0f = cubemipref.level(tmp_path, N, L, 1, ones_ids(n), dirs, dd, dtype=dtype, parts=True)
        assert lam[0].tolist() == np.clip(ks, 0, L - 1).tolist(), (d, lam)
        assert (l0f[0, :, 1] == 0).all()
    # between the powers of two the rule is linear in rho: rho = 3 * 2^(k-1) -> k + 1/2; the quotient rule's second term: moving
    # along the direction itself leaves no footprint
    dd = np.zeros((6, 1, 4), dtype)
    dd[4, 0] = -np.float32([3, 6, 12, 1.5]) * 2 / N
    lam = cubemipref.level(tmp_path, N, L, 1, ones_ids(4), planes(np.float32([(1, 0, 0)] * 4)), dd, dtype=dtype)
    assert lam[0].tolist() == [1.5, 2.5, 3.5, 0.5]
    d = np.float32([(3, -1.5, 0.75)] * 2)
    dd = np.zeros((6, 1, 2), dtype)
    dd[0::2, 0, 0], dd[1::2, 0, 1] = d[0] * 8, d[0] * -0.5  # the x step, the y step: both parallel to d
    assert (cubemipref.level(tmp_path, N, L, 1, ones_ids(2), planes(d), dd, dtype=dtype) == 0).all()
    # not finite -> the coarsest level; unsampled -> 0; nobody -> the fused-clear rule
    dd = np.zeros((6, 1, 3), dtype)
    dd[4, 0] = [np.nan, np.inf, 1e30]
    lam = cubemipref.level(tmp_path, N, L, 1, ones_ids(3), planes(np.float32([(1, 0, 0)] * 3)), dd, dtype=dtype)
    assert lam[0].tolist() == [L - 1] * 3
    lam = cubemipref.level(tmp_path, N, L, 1, ones_ids(2), planes(np.float32([(0, 0, 0), (np.nan, 1, 1)])), dd[:, :, :2], dtype=dtype)
    assert lam[0].tolist() == [0, 0]
    if dtype == np.float32:
        ids = np.uint32([[0, 1]])
        lam = cubemipref.level(tmp_path, N, L, 1, ids, planes(np.float32([(1, 0, 0)] * 2)), dd[:, :, :2], fused=False, prefill=0xdeadbeef)
        assert lam.view(np.uint32)[0, 0] == 0xdeadbeef and lam[0, 1] == L - 1
