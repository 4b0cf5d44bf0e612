"""not-gpu: the perspective-correct barycentrics' test reference (tests/persp_ref.c through tests/perspref.py) pinned: to the float64
closed form, to the geometry it exists for (the interpolated object-space point projects back onto the pixel's sample point, where the
screen-linear weights miss by pixels), to central differences of a float64 restatement for the backward and the derivatives, and to
the identity fallback for every q the rule does not accept."""
import numpy as np
import pytest

import mipref
import perspref
from support import bits, visibility_of

U = 2.0 ** -24
S_BIT = np.uint32(0x80000000)


# ------------------------------------------------------------------------------------------------ scenes under a real divide
SCENES = {"quad": perspref.quad_scene, "grid": perspref.grid_scene}
# the largest distance, in pixels, between a pixel's sample point and the float64 projection of the object-space point the C
# reference's alpha', beta' interpolate, over the two scenes above: MEASURED ONCE ON THE CPU with this file (test_geometry prints it);
# what is left is the float32 rounding of the screen positions the rasteriser's alpha, beta refer to and of the rule itself
GEOMETRY_WORST_PX = 1.04e-5  # (quad; the grid scene reaches 6.7e-6)
GEOMETRY_TOL_PX = 8 * GEOMETRY_WORST_PX


def _reproject(obj, rows, ap, bp):
    """object corners [n, 3, 3], weights [n] → the screen (x, y) of the interpolated point, float64"""
    p = ap[:, None] * obj[:, 0] + bp[:, None] * obj[:, 1] + (1.0 - ap - bp)[:, None] * obj[:, 2]
    r = p @ rows[:, :3].T + rows[:, 3]
    return r[:, 0] / r[:, 3], r[:, 1] / r[:, 3]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_geometry(tmp_path, orc, name):
    f, obj, q, rows, _ = SCENES[name]()
    v = visibility_of(tmp_path, orc, f)
    out = perspref.forward(tmp_path, q, v.n, v.words)
    assert np.array_equal(out[:2], v.words[:2]), "z and the ids are copied"
    assert np.array_equal(out[:, ~v.own], v.words[:, ~v.own]), "nobody's four words are copied"
    idx, _ = perspref.owners(v.words, v.n)
    ys, xs = np.nonzero(v.own)
    t = idx[ys, xs]
    ap, bp = out[2].view(np.float32)[ys, xs].astype(np.float64), out[3].view(np.float32)[ys, xs].astype(np.float64)
    px, py = _reproject(obj[t], rows, ap, bp)
    miss = np.hypot(px - xs, py - ys)
    al, be = v.words[2].view(np.float32)[ys, xs].astype(np.float64), v.words[3].view(np.float32)[ys, xs].astype(np.float64)
    lx, ly = _reproject(obj[t], rows, al, be)
    lin = np.hypot(lx - xs, ly - ys)
    print(f"[{name}] owned {len(t)}: perspective-correct miss max {miss.max():.3g} px; screen-linear miss median {np.median(lin):.3g} max {lin.max():.3g} px")
    assert miss.max() <= GEOMETRY_TOL_PX, miss.max()
    if name == "quad":
        assert (lin > 0.5).mean() >= 0.5, (lin > 0.5).mean()


# ------------------------------------------------------------------------------------------------ synthetic buffers: a triangle per pixel
def synthetic(seed, n, edge=False):
    """n pixels, pixel p owned by triangle p (odd p: S class), alpha, beta inside the triangle (edge: some weights slightly negative,
    as an edge pixel has them) → (words [4, 1, n], q [n, 3])"""
    rng = np.random.default_rng([seed, n])
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    if edge:
        w[::3, 0] -= 0.05
        w[::3, 1] += 0.05
    words = np.zeros((4, 1, n), np.uint32)
    words[0, 0] = bits(rng.uniform(1, 9, n).astype(np.float32))
    words[1, 0] = (np.arange(n, dtype=np.uint32) + 1) | np.where(np.arange(n) % 2 == 1, S_BIT, np.uint32(0))
    words[2, 0], words[3, 0] = bits(w[:, 0].astype(np.float32)), bits(w[:, 1].astype(np.float32))
    return words, perspref.make_q(seed, n)


def _f32_planes(words):
    al, be = words[2, 0].view(np.float32), words[3, 0].view(np.float32)
    isS = (words[1, 0] >> 31) != 0
    one = np.float32(1)
    ga = np.where(isS, (one - al) - be, one - (al + be))
    assert ga.dtype == np.float32
    return al, be, ga, isS


@pytest.mark.parametrize("edge", [False, True])
def test_closed_form(tmp_path, edge):
    """alpha', beta' against n0 / (n0 + n1 + n2) in float64 on the float32 inputs (gamma the float32 gamma of the class).  Each n_k
    rounds once (1 + d, |d| <= u); the two adds round once each, so s = sum n_k (1 + d_k)^(<=3): |s_f - s| <= 3u sum |n_k| (first
    order); the division rounds once.  alpha' = n0 (1 + d) / s_f (1 + d'): relative error <= u + 3u sum|n_k| / |s| + u <= 5u for
    weights >= 0 (sum |n_k| = s), and scaled by c = sum |n_k| / |s| >= 1 where an edge pixel has a negative weight.  The bound below
    carries the second-order terms in a factor 1.01.
    At equal q the closed form is alpha / (alpha + beta + gamma), within 5 c u of alpha' as above, and it is alpha itself only as
    far as the float32 gamma makes the three weights sum to 1: gamma = 1 - (alpha + beta) rounds twice (S: 1 - alpha, then - beta),
    each rounding at most u of a value below 2 in these inputs' range, so |alpha + beta + gamma - 1| <= 2u and the closed form lies
    within a relative 2u of alpha.  Hence the (5 c + 2) u of the second leg: the issue's bound plus that term, nothing measured."""
    words, q = synthetic(11, 4000, edge)
    out = perspref.forward(tmp_path, q, 4000, words)
    al, be, ga, _ = _f32_planes(words)
    n = np.stack([al.astype(np.float64) * q[:, 0], be.astype(np.float64) * q[:, 1], ga.astype(np.float64) * q[:, 2]])
    s = n.sum(0)
    assert (s > 0).all()
    cond = np.abs(n).sum(0) / np.abs(s)
    assert (cond > 1.0 + 1e-9).any() == edge
    for plane, k in ((2, 0), (3, 1)):
        got = out[plane, 0].view(np.float32).astype(np.float64)
        want = n[k] / s
        assert (np.abs(got - want) <= 1.01 * 5 * U * cond * np.abs(want) + 2.0 ** -149).all()
    # equal q: alpha' is alpha within the same bound
    qe = np.repeat(np.random.default_rng(5).uniform(0.25, 4, (4000, 1)).astype(np.float32), 3, 1)
    oute = perspref.forward(tmp_path, qe, 4000, words)
    c = (np.abs(al) + np.abs(be) + np.abs(ga)).astype(np.float64)  # (sum |n_k| / |s| at equal q; alpha + beta + gamma = 1 within 2u)
    for plane, wgt in ((2, al), (3, be)):
        got = oute[plane, 0].view(np.float32).astype(np.float64)
        assert (np.abs(got - wgt) <= 1.01 * (5 * c + 2) * U * np.abs(wgt.astype(np.float64)) + 2.0 ** -149).all()


def test_backward_against_central_differences(tmp_path):
    """galpha, gbeta and the three gq terms of every pixel against central differences of L = ga alpha' + gb beta' restated in
    float64.  Step h: the restatement is rational in (alpha, beta, q) with poles only at s = 0; its k-th derivatives are bounded by
    k! G (Q / s)^k ... with G = |ga| + |gb| and Q = max q, so the truncation term of a central difference is <= G (Q / s)^3 h^2 and
    its rounding term <= 4 * 2^-53 G / h.  At h = 1e-5 with Q / s <= 16 both are below 1e-6 G.  The float32 side: alpha', beta' carry
    5u each, t three more roundings, r one, g_k two, the outputs two: fewer than 16 roundings of quantities bounded by
    M = 2 G (q0 + q1 + q2) / s (galpha, gbeta) and 2 G / s (a gq term: |weight| <= 1), so 16 u M."""
    n, h = 3000, 1e-5
    words, q = synthetic(21, n)
    rng = np.random.default_rng(3)
    gbp = rng.normal(0, 2, (2, 1, n)).astype(np.float32)
    acc = perspref.Grad(q.shape)
    gb = perspref.grad(tmp_path, q, n, words, gbp, into=acc)
    assert (acc.count == 1).all()
    al, be, ga, _ = _f32_planes(words)
    al, be, ga = (x.astype(np.float64) for x in (al, be, ga))
    q64, gA, gB = q.astype(np.float64), gbp[0, 0].astype(np.float64), gbp[1, 0].astype(np.float64)

    def L(al_, be_, q_):
        # (gamma is the float32 gamma the pass multiplies by: the restatement differentiates through 1 - alpha - beta from there)
        n0, n1, n2 = al_ * q_[:, 0], be_ * q_[:, 1], (ga - (al_ - al) - (be_ - be)) * q_[:, 2]
        s = n0 + n1 + n2
        return gA * n0 / s + gB * n1 / s
    s = al * q64[:, 0] + be * q64[:, 1] + ga * q64[:, 2]
    G, Q = np.abs(gA) + np.abs(gB), q64.max(1)
    cd_err = G * (Q / s) ** 3 * h * h + 4 * 2.0 ** -53 * G / h
    M = 2 * G * q64.sum(1) / s
    for plane, d in ((0, (h, 0.0)), (1, (0.0, h))):
        want = (L(al + d[0], be + d[1], q64) - L(al - d[0], be - d[1], q64)) / (2 * h)
        err = np.abs(gb[plane, 0].astype(np.float64) - want)
        assert (err <= 16 * U * M + cd_err).all(), (plane, float((err / (16 * U * M + cd_err)).max()))
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        want = (L(al, be, q64 + e) - L(al, be, q64 - e)) / (2 * h)
        err = np.abs(acc.gq[:, k] - want)
        assert (err <= 16 * U * 2 * G / s + cd_err).all(), (k, float((err / (16 * U * 2 * G / s + cd_err)).max()))
    assert np.allclose(acc.gabs, np.abs(acc.gq), rtol=0, atol=0)


def test_derivatives_against_central_differences(tmp_path):
    """d/dx, d/dy of every channel against central differences of u(x, y) restated in float64, alpha and beta affine in the sample
    point with the triangle's own gradients.  Step and rounding as in the backward test with G replaced by A = max |corner value|
    and one more factor g = |grad alpha| + |grad beta| per derivative: truncation <= A (Q g / s)^3 h^2 ... rounding 4 * 2^-53 A /
    h.  The float32 side: u carries alpha', beta' (5u each) and three roundings, e_k two, the differences, the fma, the product and
    the division six, and gax .. gby (five roundings each from the positions); fewer than 32 roundings of quantities bounded by
    M = 4 A Q g / s."""
    n, C, h = 2000, 3, 1e-5
    words, q = synthetic(31, n)
    rng = np.random.default_rng(9)
    pos = np.zeros((n, 9), np.float32)
    tri = rng.uniform(0, 8, (n, 3, 2)) + np.float64([[0, 0], [30, 5], [8, 35]])  # areas well away from 0
    pos[:, [0, 1, 3, 4, 6, 7]] = tri.reshape(n, 6).astype(np.float32)
    attr = rng.normal(0, 2, (n, 3, C)).astype(np.float32)
    got = perspref.deriv(tmp_path, q, pos, attr, n, words)
    al, be, ga, _ = _f32_planes(words)
    al, be, ga = (x.astype(np.float64) for x in (al, be, ga))
    P, q64, a64 = pos.astype(np.float64), q.astype(np.float64), attr.astype(np.float64)
    area = (P[:, 3] - P[:, 0]) * (P[:, 7] - P[:, 1]) - (P[:, 4] - P[:, 1]) * (P[:, 6] - P[:, 0])
    assert (np.abs(area) > 100).all()
    grads = {"x": ((P[:, 4] - P[:, 7]) / area, (P[:, 7] - P[:, 1]) / area), "y": ((P[:, 6] - P[:, 3]) / area, (P[:, 0] - P[:, 6]) / area)}

    def u(da, db, ch):
        n0, n1, n2 = (al + da) * q64[:, 0], (be + db) * q64[:, 1], (ga - da - db) * q64[:, 2]
        s = n0 + n1 + n2
        return (n0 * a64[:, 0, ch] + n1 * a64[:, 1, ch] + n2 * a64[:, 2, ch]) / s
    s = al * q64[:, 0] + be * q64[:, 1] + ga * q64[:, 2]
    Q = q64.max(1)
    for ch in range(C):
        A = np.abs(a64[:, :, ch]).max(1)
        for axis, (gax, gbx) in enumerate((grads["x"], grads["y"])):
            g = np.abs(gax) + np.abs(gbx)
            want = (u(gax * h, gbx * h, ch) - u(-gax * h, -gbx * h, ch)) / (2 * h)
            tol = 32 * U * 4 * A * Q * g / s + A * (Q * g / s) ** 3 * h * h + 4 * 2.0 ** -53 * A / h
            err = np.abs(got[2 * ch + axis, 0].astype(np.float64) - want)
            assert (err <= tol).all(), (ch, axis, float((err / tol).max()))
    assert (got != 0).mean() > 0.99


# ------------------------------------------------------------------------------------------------ what the rule does not accept
def _identity_everywhere(tmp_path, words, q, n_tris, pos, attr):
    """forward: the four planes copied; backward: ga, gb passed through and nothing added; deriv: the screen-linear constants"""
    n = words.shape[2]
    out = perspref.forward(tmp_path, q, n_tris, words)
    assert np.array_equal(out, words)
    gbp = np.random.default_rng(1).normal(0, 2, (2, 1, n)).astype(np.float32)
    acc = perspref.Grad((len(q), 3))
    pre = np.full((2, 1, n), 0xdeadbeef, np.uint32)
    gb = perspref.grad(tmp_path, q, n_tris, words, gbp, into=acc, fused=False, prefill=pre)
    idx, _ = perspref.owners(words, n_tris)
    own = idx[0] >= 0
    assert np.array_equal(bits(gb)[:, 0, own], bits(gbp)[:, 0, own]) and (bits(gb)[:, 0, ~own] == 0xdeadbeef).all()
    assert not acc.gq.any() and not acc.gabs.any() and not acc.count.any()
    # every plane is interpolate_deriv's own word (tests/mip_ref.c, the reference of the screen-linear constants), nobody's 0
    got = perspref.deriv(tmp_path, q, pos, attr, n_tris, words)
    want = mipref.deriv(tmp_path, attr, pos, n_tris, words[1])
    assert got.shape == want.shape == (2 * attr.shape[2], 1, n) and np.array_equal(bits(got), bits(want))
    assert (not own.any() or (got[:, 0, own] != 0).any()) and (got[:, 0, ~own] == 0).all()


@pytest.mark.parametrize("bad", list(perspref.HOSTILE_Q), ids=lambda x: repr(float(x)))
@pytest.mark.parametrize("corner", [0, 1, 2])
def test_invalid_q_is_the_identity(tmp_path, bad, corner):
    n = 64
    words, q = synthetic(41, n)
    rng = np.random.default_rng(2)
    pos = np.zeros((n, 9), np.float32)
    pos[:, [0, 1, 3, 4, 6, 7]] = (rng.uniform(0, 10, (n, 6)) + [0, 0, 30, 5, 8, 35]).astype(np.float32)
    attr = rng.normal(0, 2, (n, 3, 2)).astype(np.float32)
    q = q.copy()
    q[:, corner] = bad
    if bad == np.float32(3e38):
        q[:] = bad  # (finite, positive and normal: only the sum overflows, at an edge pixel's weights 1.5, 0.5, -1)
        words[2, 0], words[3, 0] = bits(np.full(n, 1.5, np.float32)), bits(np.full(n, 0.5, np.float32))
        al, be, ga, _ = _f32_planes(words)
        with np.errstate(over="ignore"):
            s = (al * q[:, 0] + be * q[:, 1]) + ga * q[:, 2]
        assert np.isposinf(s).all() and perspref.valid32(q, np.float32(1)).all() and not perspref.valid32(q, s).any()
    _identity_everywhere(tmp_path, words, q, n, pos, attr)


def test_nonpositive_s_and_strangers(tmp_path):
    """s <= 0 from a negative edge weight against a large q; ids of nobody (0, the bare class bit) and of strangers (an index at or
    beyond the triangle count, either class): all four words copied, nothing else happens"""
    n = 64
    words, q = synthetic(43, n)
    rng = np.random.default_rng(4)
    pos = np.zeros((n, 9), np.float32)
    pos[:, [0, 1, 3, 4, 6, 7]] = (rng.uniform(0, 10, (n, 6)) + [0, 0, 30, 5, 8, 35]).astype(np.float32)
    attr = rng.normal(0, 2, (n, 3, 2)).astype(np.float32)
    words[2, 0] = bits(np.full(n, -0.25, np.float32))  # alpha < 0, beta + gamma = 1.25
    words[3, 0] = bits(np.full(n, 0.5, np.float32))
    q[:] = [4.0, 0.25, 0.25]
    q[::2] = [3.0, 1.0, 1.0]  # s = -0.75 + 0.5 + 0.75 = 0.5 > 0 would be valid: make it exactly 0 on these
    q[::2, 0] = 5.0           # s = -1.25 + 0.5 + 0.75 = 0
    al, be, ga, _ = _f32_planes(words)
    s = (al * q[:, 0] + be * q[:, 1]) + ga * q[:, 2]
    assert (s <= 0).all() and (s[::2] == 0).all() and (s[1::2] < 0).all()
    _identity_everywhere(tmp_path, words, q, n, pos, attr)
    words2, q2 = synthetic(44, n)
    words2[1, 0, 0::4] = 0
    words2[1, 0, 1::4] = S_BIT
    words2[1, 0, 2::4] = n + 1 + np.arange(n // 4, dtype=np.uint32)
    words2[1, 0, 3::4] = (n + 1) | S_BIT
    _identity_everywhere(tmp_path, words2, q2, n, pos, attr)
