"""not-gpu: the mip passes' test reference (tests/mip_ref.c through tests/mipref.py) pinned: hand-computed cases of the pyramid and of
the level rule, a float64 restatement in numpy with central differences (the level held fixed), the fold against an explicit
transpose of the build's linear map, the derivative planes against central differences of the interpolation's reference, and — on
the oracle's visibility buffer of the frames tests/test_gpu_texture_mip.py renders — the counts that keep those tests from passing
vacuously."""
import numpy as np
import pytest

import interpref
import mipref
import texref
from mipref import CLAMP, WRAP
from support import bits, frame_positions, visibility_of


def grid(n):
    """n owned pixels in a row, every one of triangle 0"""
    return np.ones((1, n), np.uint32)


def planes(*rows):
    return np.ascontiguousarray(np.float32(rows)[:, None, :])


# ------------------------------------------------------------------------------------------------------ the pyramid
def test_levels_and_the_32_by_8_chain(tmp_path):
    for (w, h), n in mipref.LEVELS.items():
        assert mipref.levels(tmp_path, w, h) == n, (w, h)
    assert mipref.sizes(tmp_path, 32, 8, 6) == [(32, 8), (16, 4), (8, 2), (4, 1), (2, 1), (1, 1)]
    assert [mipref.level(tmp_path, 32, 8, l)[2] for l in range(1, 6)] == [0.25, 0.25, 0.25, 0.5, 0.5]
    assert mipref.sizes(tmp_path, 96, 64, 6)[-1] == (3, 2) and mipref.sizes(tmp_path, 100, 70, 2) == [(100, 70), (50, 35)]
    assert [mipref.level(tmp_path, 8, 32, l)[2] for l in range(1, 6)] == [0.25, 0.25, 0.25, 0.5, 0.5]
    # a hand-built level: 4 x 2 -> 2 x 1 -> 1 x 1
    tex = np.float32([[[1], [2], [3], [4]], [[5], [6], [7], [9]]])
    lv = mipref.views(tmp_path, mipref.build(tmp_path, tex, 3), tex.shape, 3)
    assert lv[0].tolist() == [[[3.5], [5.75]]] and lv[1].tolist() == [[[4.625]]]
    col = np.float32([[[1.0]], [[2.0]], [[4.0]], [[9.0]]])  # 1 x 4: halves along y
    lv = mipref.views(tmp_path, mipref.build(tmp_path, col, 3), col.shape, 3)
    assert lv[0].tolist() == [[[1.5]], [[6.5]]] and lv[1].tolist() == [[[4.0]]]
    # frames are built apart
    two = mipref.make_tex(1, 32, 8, 3, frames=2)
    both = mipref.build(tmp_path, two, 6)
    for i in range(2):
        assert np.array_equal(mipref.frame_mip(tmp_path, both, two.shape, 6, i), mipref.build(tmp_path, two[i], 6))


def build_matrix(tmp_path, w, h, n_levels):
    """[texels of levels 1 .. , w * h] float64: the build as a matrix (one channel), from its own factors"""
    sz = mipref.sizes(tmp_path, w, h, n_levels)
    rows, prev = [], np.eye(w * h)
    for l in range(1, n_levels):
        (pw, ph), (lw, lh), k = sz[l - 1], sz[l], mipref.level(tmp_path, w, h, l)[2]
        m = np.zeros((lw * lh, pw * ph))
        for y in range(lh):
            for x in range(lw):
                for dy in range(2 if ph > 1 else 1):
                    for dx in range(2 if pw > 1 else 1):
                        m[y * lw + x, ((2 * y + dy) if ph > 1 else 0) * pw + ((2 * x + dx) if pw > 1 else 0)] = k
        prev = m @ prev
        rows.append(prev)
    return np.concatenate(rows)


@pytest.mark.parametrize("w,h", [(32, 8), (96, 64), (100, 70), (8, 32), (2, 1), (16, 16)])
def test_fold_is_the_transpose_of_the_build(tmp_path, w, h):
    L = mipref.levels(tmp_path, w, h)
    for n_levels in {2, L}:
        M = build_matrix(tmp_path, w, h, n_levels)
        rng = np.random.default_rng([w, h, n_levels])
        tex = rng.normal(0, 3, (h, w, 1)).astype(np.float32)
        mip = mipref.build(tmp_path, tex, n_levels)
        assert np.abs(mip - M @ tex.ravel().astype(np.float64)).max() <= 2.0 ** -20 * np.abs(tex).max()  # the matrix is the build
        gmip = rng.normal(0, 2, mip.size).astype(np.float32)
        g0 = rng.normal(0, 2, tex.shape).astype(np.float32)
        got = mipref.fold(tmp_path, gmip, tex.shape, n_levels, g0)
        want = g0.ravel().astype(np.float64) + M.T @ gmip.astype(np.float64)
        mag = np.abs(g0.ravel()) + np.abs(M.T) @ np.abs(gmip)
        assert (np.abs(got.ravel() - want) <= n_levels * 2.0 ** -23 * mag).all()  # one rounding per fma of the chain
        # exact on integers (factors are powers of two, sums of a few small integers are representable)
        gi, g0i = rng.integers(-8, 9, mip.size).astype(np.float32), rng.integers(-8, 9, tex.shape).astype(np.float32)
        assert np.array_equal(mipref.fold(tmp_path, gi, tex.shape, n_levels, g0i).ravel().astype(np.float64), g0i.ravel() + M.T @ gi.astype(np.float64))
    # several frames and channels: each (frame, channel) folds alone
    tex_shape = (2, h, w, 3)
    n = mipref.mip_floats(tmp_path, tex_shape, L)
    gm = np.random.default_rng(5).normal(0, 1, n).astype(np.float32)
    got = mipref.fold(tmp_path, gm, tex_shape, L, np.zeros(tex_shape, np.float32))
    lv = mipref.views(tmp_path, gm, tex_shape, L)
    for f in range(2):
        for c in range(3):
            one = np.concatenate([v[f, :, :, c].ravel() for v in lv])
            assert np.array_equal(got[f, :, :, c], mipref.fold(tmp_path, one, (h, w, 1), L, np.zeros((h, w, 1), np.float32))[:, :, 0])


# ------------------------------------------------------------------------------------------------------ the level rule
def test_the_level_rule_by_hand(tmp_path):
    W = H = 64
    L = 7
    for k in range(0, 9):
        for axis in range(4):  # rho from ux, uy, vx or vy alone
            for frac, f_want in ((1.0, 0.0), (1.5, 0.5), (1.25, 0.25), (1.75, 0.75)):
                d = np.zeros((4, 1), np.float32)
                d[axis, 0] = frac * 2.0 ** k / 64
                l0, f = mipref.lod(tmp_path, (H, W), L, d)
                if k >= L - 1:
                    assert (int(l0[0]), float(f[0])) == (L - 1, 0.0), (k, frac)  # at and beyond the coarsest level
                else:
                    assert (int(l0[0]), float(f[0])) == (k, f_want), (k, axis, frac)
    # the longer of the two footprint axes decides; a 3-4-5 footprint in x
    l0, f = mipref.lod(tmp_path, (H, W), L, np.float32([[3 * 2 / 64], [0.5 / 64], [4 * 2 / 64], [0]]))
    assert (int(l0[0]), float(f[0])) == (3, 0.25)  # rho = 10 = 1.25 * 2^3
    # magnified, no footprint, tiny
    for d in ([0, 0, 0, 0], [1 / 64, 0, 0, 0], [0.3 / 64, 0.2 / 64, -0.9 / 64, 0.1 / 64], [1e-30, 0, 0, 1e-38], [-0.0, 0, 0, 0]):
        l0, f = mipref.lod(tmp_path, (H, W), L, np.float32(d)[:, None])
        assert (int(l0[0]), float(f[0])) == (0, 0.0), d
    # not finite, and finite with an infinite footprint: the coarsest level
    for d in ([np.nan, 0, 0, 0], [0, np.inf, 0, 0], [0, 0, -np.inf, 0], [0, 0, 0, np.nan], [3e38, 0, 0, 0], [1e19, 0, 1e19, 0], [-3e38, 3e38, 3e38, -3e38]):
        l0, f = mipref.lod(tmp_path, (H, W), L, np.float32(d)[:, None])
        assert (int(l0[0]), float(f[0])) == (L - 1, 0.0), d
    # one level: always level 0
    l0, f = mipref.lod(tmp_path, (H, W), 1, np.float32([[5.0], [np.nan], [0], [0]]))
    assert (int(l0[0]), float(f[0])) == (0, 0.0)
    # lambda is continuous, monotone, log2 at the powers of two and within 0.0861 of it
    rho = np.exp2(np.linspace(0.001, 5.999, 4001)).astype(np.float32)
    d = np.zeros((4, rho.size), np.float32)
    d[2] = rho / 64
    l0, f = mipref.lod(tmp_path, (H, W), L, d)
    lam = l0 + f.astype(np.float64)
    true = np.log2((d[2].astype(np.float64) * 64))
    assert (np.diff(lam) >= 0).all() and np.abs(lam - true).max() <= 0.0861 and np.abs(lam - true).max() >= 0.085
    assert np.abs(np.diff(lam)).max() <= 0.01


@pytest.mark.parametrize("mode", [CLAMP, WRAP])
def test_constant_textures_magnified_pixels_and_the_coarsest_level(tmp_path, mode):
    rng = np.random.default_rng(mode)
    n = 300
    u, v = rng.uniform(-0.5, 1.5, n).astype(np.float32), rng.uniform(-0.5, 1.5, n).astype(np.float32)
    uv = planes(u, v)
    for (w, h) in ((64, 64), (96, 64), (32, 8)):
        L = mipref.levels(tmp_path, w, h)
        rho = np.exp2(rng.uniform(-2, L + 1, n))
        ang = rng.uniform(0, 2 * np.pi, n)
        uvd = planes(rho * np.cos(ang) / w, 0.3 * rho / w * np.sin(ang), rho * np.sin(ang) / h, -0.3 * rho / h * np.cos(ang))
        # a constant texture gives the constant exactly, at every level and every lambda
        const = np.full((h, w, 2), 2.7182817, np.float32)
        mip = mipref.build(tmp_path, const, L)
        assert (mip == np.float32(2.7182817)).all()
        out = mipref.forward(tmp_path, const, mip, mode, L, 1, grid(n), uv, uvd)
        assert (out == np.float32(2.7182817)).all()
        l0, f = mipref.lod(tmp_path, (h, w), L, uvd[:, 0])
        assert len(set(l0.tolist())) == L and ((f > 0) & (f < 1)).sum() > n // 2
        # rho <= 1: level 0, the bilinear pass's sample
        tex = mipref.make_tex(3, w, h, 3)
        mip = mipref.build(tmp_path, tex, L)
        small = uvd * np.float32(0.2 / np.abs(uvd * np.float32([w, w, h, h])[:, None, None]).max())
        out = mipref.forward(tmp_path, tex, mip, mode, L, 1, grid(n), uv, small)
        assert np.array_equal(bits(out), bits(texref.forward(tmp_path, tex, mode, 1, grid(n), uv)))
        # one level: the bilinear pass whatever the derivatives say
        assert np.array_equal(bits(mipref.forward(tmp_path, tex, None, mode, 1, 1, grid(n), uv, None)), bits(texref.forward(tmp_path, tex, mode, 1, grid(n), uv)))
        # non-finite derivatives: the coarsest level's bilinear sample
        bad = uvd.copy()
        bad[rng.integers(0, 4, n), 0, np.arange(n)] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), n)
        top = mipref.views(tmp_path, mip, tex.shape, L)[-1]
        out = mipref.forward(tmp_path, tex, mip, mode, L, 1, grid(n), uv, bad)
        assert np.array_equal(bits(out), bits(texref.forward(tmp_path, top, mode, 1, grid(n), uv)))
        # f == 0 at level k: exactly that level's bilinear sample; f == 0.5: the mean-ward blend of two levels
        for k in range(1, L - 1):
            d = np.zeros((4, 1, n), np.float32)
            d[0] = 2.0 ** k / w
            lv = [tex] + mipref.views(tmp_path, mip, tex.shape, L)
            out = mipref.forward(tmp_path, tex, mip, mode, L, 1, grid(n), uv, d)
            a = texref.forward(tmp_path, lv[k], mode, 1, grid(n), uv)
            assert np.array_equal(bits(out), bits(a))
            d[0] = 1.5 * 2.0 ** k / w
            out = mipref.forward(tmp_path, tex, mip, mode, L, 1, grid(n), uv, d)
            b = texref.forward(tmp_path, lv[k + 1], mode, 1, grid(n), uv)
            assert np.array_equal(bits(out), bits(a + np.float32(0.5) * (b - a)))  # fmaf(0.5, b - a, a): the product is exact


# ------------------------------------------------------------------------------------------------------ float64 restatement
def np_bilinear(tex, mode, u, v):
    """the bilinear rule in numpy float64, vectorised over u, v [n] → [n, C]"""
    H, W, _ = tex.shape

    def axis(c, n):
        if mode == WRAP:
            c = c - np.floor(c)
        f = c * n - 0.5
        if mode == CLAMP:
            f = np.clip(f, 0.0, n - 1.0)
        i0 = np.floor(f)
        t = f - i0
        i0 = i0.astype(np.int64)
        i1 = i0 + 1
        if mode == CLAMP:
            i1 = np.minimum(i1, n - 1)
        else:
            i0, i1 = i0 % n, i1 % n
        return i0, i1, t
    x0, x1, tx = axis(np.asarray(u, np.float64), W)
    y0, y1, ty = axis(np.asarray(v, np.float64), H)
    top = tex[y0, x0] + tx[:, None] * (tex[y0, x1] - tex[y0, x0])
    bot = tex[y1, x0] + tx[:, None] * (tex[y1, x1] - tex[y1, x0])
    return top + ty[:, None] * (bot - top)


def np_pyramid(tex64, n_levels):
    lv = [tex64]
    for _ in range(1, n_levels):
        t = lv[-1]
        h, w = t.shape[:2]
        if h > 1 and w > 1:
            t = (t[0::2, 0::2] + t[0::2, 1::2] + t[1::2, 0::2] + t[1::2, 1::2]) * 0.25
        elif w > 1:
            t = (t[:, 0::2] + t[:, 1::2]) * 0.5
        else:
            t = (t[0::2] + t[1::2]) * 0.5
        lv.append(t)
    return lv


def np_trilinear(tex64, n_levels, mode, u, v, l0, f):
    """the lookup in float64 with the level (l0, f) given: held fixed"""
    lv = np_pyramid(tex64, n_levels)
    out = np.zeros((len(u), tex64.shape[2]))
    for l in range(n_levels):
        here, above = l0 == l, (l0 + 1 == l) & (f != 0)
        if here.any():
            out[here] += (1 - f[here])[:, None] * np_bilinear(lv[l], mode, u[here], v[here])
        if above.any():
            out[above] += f[above][:, None] * np_bilinear(lv[l], mode, u[above], v[above])
    return out


@pytest.mark.parametrize("mode", [CLAMP, WRAP])
@pytest.mark.parametrize("w,h", [(64, 64), (96, 64), (32, 8), (100, 70)])
def test_gradients_against_central_differences_in_float64(tmp_path, mode, w, h):
    """guv and the folded gtex of the reference against central differences of np_trilinear with lambda held fixed, at points at
    least 0.05 texels away from a texel centre line of BOTH levels a pixel blends (the coarser level's grid contains none that the
    finer one's lacks — its centres lie on the finer level's texel borders — so both are checked) and inside the CLAMP borders"""
    rng = np.random.default_rng([w, h, mode, 7])
    C, n = 3, 400
    L = mipref.levels(tmp_path, w, h)
    tex = mipref.make_tex(2, w, h, C)
    mip = mipref.build(tmp_path, tex, L)
    lo, hi = (-0.2, 1.2) if mode == CLAMP else (-2.0, 3.0)
    m = 12 * n
    u, v = rng.uniform(lo, hi, m).astype(np.float32), rng.uniform(lo, hi, m).astype(np.float32)
    rho = np.exp2(rng.uniform(-2, L + 1, m))
    ang = rng.uniform(0, 2 * np.pi, m)
    uvd = np.float32([rho * np.cos(ang) / w, 0.5 * rho * np.sin(ang) / w, rho * np.sin(ang) / h, -0.5 * rho * np.cos(ang) / h])
    l0, f = mipref.lod(tmp_path, (h, w), L, uvd)
    sz = mipref.sizes(tmp_path, w, h, L)

    def away(c, size):
        x = c.astype(np.float64) * size - 0.5
        return np.abs(x - np.rint(x)) > 0.05
    keep = np.ones(m, bool)
    for l in range(L):
        at = (l0 == l) | ((l0 + 1 == l) & (f != 0))
        keep &= ~at | (away(u, sz[l][0]) & away(v, sz[l][1]))
    u, v, uvd, l0, f = u[keep][:n], v[keep][:n], uvd[:, keep][:, :n], l0[keep][:n], f[keep][:n]
    # (log2 rho is uniform over L + 3 octaves, L - 1 of which blend two levels: half that share at least)
    assert len(u) == n and len(set(l0.tolist())) == L and ((f > 0) & (f < 1)).sum() > n * (L - 1) // (2 * (L + 3))
    uv, uvdp = planes(u, v), np.ascontiguousarray(uvd[:, None, :])
    gout = rng.normal(0, 1, (C, 1, n)).astype(np.float32)
    tex64 = tex.astype(np.float64)
    fd = f.astype(np.float64)
    out = mipref.forward(tmp_path, tex, mip, mode, L, 1, grid(n), uv, uvdp)[:, 0].T
    want = np_trilinear(tex64, L, mode, u, v, l0, fd)
    scale = np.abs(tex).max()
    assert np.abs(out - want).max() <= 8 * 2.0 ** -22 * max(w, h) * scale
    acc = mipref.Grad(tmp_path, tex.shape, L)
    guv = mipref.grad(tmp_path, tex, mip, mode, L, 1, grid(n), uv, uvdp, gout, into=acc)[:, 0]
    g = gout[:, 0].T.astype(np.float64)
    eps = 1e-4 / max(w, h)
    u64, v64 = u.astype(np.float64), v.astype(np.float64)
    du = ((np_trilinear(tex64, L, mode, u64 + eps, v64, l0, fd) - np_trilinear(tex64, L, mode, u64 - eps, v64, l0, fd)) * g).sum(1) / (2 * eps)
    dv = ((np_trilinear(tex64, L, mode, u64, v64 + eps, l0, fd) - np_trilinear(tex64, L, mode, u64, v64 - eps, l0, fd)) * g).sum(1) / (2 * eps)
    tol = 1e-4 * scale * max(w, h) * C
    assert np.abs(guv[0] - du).max() <= tol and np.abs(guv[1] - dv).max() <= tol, (np.abs(guv[0] - du).max(), np.abs(guv[1] - dv).max(), tol)
    assert (guv != 0).any()
    # the texels: the loss sum(out * gout) is linear in level 0; per-level sums in double, folded
    assert acc.count.sum() == 4 * (n + int((f != 0).sum()))
    g0, a0, _ = acc.level(0)
    parts = [acc.level(l)[0].ravel() for l in range(1, L)]
    folded = mipref.fold(tmp_path, np.concatenate(parts).astype(np.float32), tex.shape, L, g0.astype(np.float32)).astype(np.float64)
    mags = mipref.fold(tmp_path, np.concatenate([acc.level(l)[1].ravel() for l in range(1, L)]).astype(np.float32), tex.shape, L, a0.astype(np.float32))
    loss = lambda t: (np_trilinear(t, L, mode, u, v, l0, fd) * g).sum()  # noqa: E731
    base = loss(tex64)
    picks = [(int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(0, C))) for _ in range(12)]
    for (y, x, c) in picks:
        bump = tex64.copy()
        bump[y, x, c] += 1.0
        assert abs((loss(bump) - base) - folded[y, x, c]) <= 1e-4 * max(1.0, mags[y, x, c]), (y, x, c)
    assert (folded != 0).sum() >= n  # (every sample reaches a texel or more of level 0, in every channel)


# ------------------------------------------------------------------------------------------------------ the derivatives
def test_deriv_against_central_differences_of_the_interpolation(tmp_path, orc):
    """interpolation is affine inside one owner, so (F(x + 1) - F(x - 1)) / 2 of the interpolation reference's planes is the
    derivative up to rounding.  The bound, per pixel: alpha and beta at a pixel are quotients of cross products of coordinates up to
    S (the owner's largest |coordinate|), each within a few 2^-24 S |edge| of exact before the division by the area, so an
    interpolated value is within K 2^-24 ((|da| + |db|) S G + |a| + |b| + |c|) of exact, G the largest of the four gradient
    components; the difference of two such values halves: the same bound, K = 16 for the handful of roundings on either side."""
    f = mipref.soup_frames()[0]
    vis = visibility_of(tmp_path, orc, f)
    rng = np.random.default_rng(3)
    attr = rng.normal(0, 1, (vis.n, 3, 5)).astype(np.float32)
    pos = frame_positions(f)
    F = interpref.forward(tmp_path, attr, vis.n, vis.words).astype(np.float64)  # [C, H, W]
    D = mipref.deriv(tmp_path, attr, pos, vis.n, vis.words[1]).astype(np.float64)  # [2 C, H, W]
    ids = vis.words[1] & 0x7fffffff
    assert (D[:, ~vis.own] == 0).all()
    t = np.maximum(ids.astype(np.int64) - 1, 0)
    S = np.abs(pos).max(1)[t]
    one = np.ones((1, 1), np.uint32)
    G = np.zeros(vis.n)
    for i in range(vis.n):  # the gradient components themselves, from a one-channel attribute (1, 0, 0) and (0, 1, 0)
        p = np.zeros((vis.n, 3, 2), np.float32)
        p[i, 0, 0] = p[i, 1, 1] = 1.0
        G[i] = np.abs(mipref.deriv(tmp_path, p, pos, vis.n, one * np.uint32(i + 1))).max()
    mag = (np.abs(attr[:, 0] - attr[:, 2]) + np.abs(attr[:, 1] - attr[:, 2]))[t] * (S * G[t])[..., None] + np.abs(attr).sum(1)[t]  # [H, W, C]
    tol = 16 * 2.0 ** -24 * np.moveaxis(mag, 2, 0)
    same_x = vis.own[:, 1:-1] & (ids[:, :-2] == ids[:, 1:-1]) & (ids[:, 2:] == ids[:, 1:-1])
    same_y = vis.own[1:-1] & (ids[:-2] == ids[1:-1]) & (ids[2:] == ids[1:-1])
    assert same_x.sum() > 1000 and same_y.sum() > 1000
    dx, dy = (F[:, :, 2:] - F[:, :, :-2]) / 2, (F[:, 2:] - F[:, :-2]) / 2
    ex, ey = np.abs(dx - D[0::2][:, :, 1:-1]), np.abs(dy - D[1::2][:, 1:-1])
    print(f"deriv: max err / tol x {np.max(ex[:, same_x] / tol[:, :, 1:-1][:, same_x]):.3f} y {np.max(ey[:, same_y] / tol[:, 1:-1][:, same_y]):.3f}")
    assert (ex[:, same_x] <= tol[:, :, 1:-1][:, same_x]).all() and (ey[:, same_y] <= tol[:, 1:-1][:, same_y]).all()
    assert (D[:, vis.own] != 0).mean() > 0.9
    # by hand: the right triangle (0,0) (4,0) (0,2): alpha = 1 - x/4 - y/2 ... a - c along x over 4 pixels, b - c ... along y over 2
    p1 = np.float32([[0, 0, 1, 4, 0, 1, 0, 2, 1]])
    a1 = np.float32([[[8.0], [12.0], [2.0]]])  # at (0,0), (4,0), (0,2)
    d1 = mipref.deriv(tmp_path, a1, p1, 1, one)
    assert d1[:, 0, 0].tolist() == [1.0, -3.0]
    # a zero area: inf / NaN as IEEE has them, nothing else
    d0 = mipref.deriv(tmp_path, a1, np.float32([[0, 0, 1, 1, 1, 1, 2, 2, 1]]), 1, one)
    assert not np.isfinite(d0).any()
    pre = np.full((2, 1, 1), 0xdeadbeef, np.uint32)
    assert (bits(mipref.deriv(tmp_path, a1, p1, 1, one * 2, fused=False, prefill=pre)) == 0xdeadbeef).all()
    assert (bits(mipref.deriv(tmp_path, a1, p1, 1, one * np.uint32(0x80000000), fused=True, prefill=pre)) == 0).all()
    assert np.array_equal(mipref.deriv(tmp_path, a1, p1, 1, one | np.uint32(0x80000000)), d1)  # the class bit plays no part


# ------------------------------------------------------------------------------------------------------ the GPU tests' frames
def test_the_gpu_tests_frames_are_not_vacuous(tmp_path, orc):
    """on the oracle's visibility buffer of the frame tests/test_gpu_texture_mip.py renders (soup(1, 90, 64, 64) in front of the
    backdrop), with uv the interpolation reference's planes of the frame's own uv and uvd this reference's derivative planes, under a
    64 x 64 texture: among the sampled pixels at least 100 at level 0 with f == 0, at least 100 with 0 < f < 1, and at least three
    distinct l0 >= 1 with at least 10 pixels each"""
    f = mipref.soup_frames()[0]
    vis = visibility_of(tmp_path, orc, f)
    uva = texref.frame_uv(f)
    uv = interpref.forward(tmp_path, uva, vis.n, vis.words)
    uvd = mipref.deriv(tmp_path, uva, frame_positions(f), vis.n, vis.words[1])
    smp = vis.own & np.isfinite(uv).all(0)
    l0, fr = mipref.lod(tmp_path, (64, 64), 7, uvd)
    magnified = int((smp & (l0 == 0) & (fr == 0)).sum())
    blended = int((smp & (fr > 0) & (fr < 1)).sum())
    per_level = {l: int((smp & (l0 == l)).sum()) for l in range(1, 7)}
    print(f"sampled {int(smp.sum())} magnified {magnified} blended {blended} per level {per_level}")
    assert magnified >= 100 and blended >= 100
    assert sum(1 for n in per_level.values() if n >= 10) >= 3


@pytest.mark.parametrize("mode", [CLAMP, WRAP])
def test_the_overflow_case_exceeds_the_table_in_every_tile(tmp_path, mode):
    """what tests/test_gpu_texture_mip.py's no-slot test rests on: each of the four tiles of both frames touches more than TG_SLOTS
    distinct texels of level 0 (every pixel's four corners its own: 4 * 32 * 32), frame 0 nothing else, frame 1 a level 1 that fits"""
    uv, uvd = mipref.overflow_planes()
    ids = np.ones((64, 64), np.uint32)
    for i in range(2):
        l0, f = mipref.lod(tmp_path, (256, 256), 9, uvd[i])
        assert (l0 == 0).all() and (f == (0.0, 0.5)[i]).all()
        per_tile = mipref.tile_texels(tmp_path, ids, uv[i], uvd[i], (256, 256), mode, 9, 1)
        assert per_tile.shape == (2, 2, 9) and (per_tile[..., 0] == 4096).all() and 4096 > mipref.TG_SLOTS
        level1 = per_tile[..., 1]
        assert (per_tile[..., 2:] == 0).all() and ((level1 == 0).all() if i == 0 else ((level1 > 0) & (level1 <= mipref.TG_SLOTS)).all())
