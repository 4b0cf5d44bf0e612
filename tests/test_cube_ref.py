"""not-gpu: the cube lookup's CPU reference (tests/cube_ref.c through tests/cuberef.py) pinned against include/srz.h's rule: the face
table by hand, the major-axis ties, the 24-row seam table against its geometric definition derived here in float64 from the faces'
(n, su, sv), seamlessness across all 12 edges on dyadic inputs, the gradients against central differences of a float64 restatement,
and what is and is not sampled."""
import numpy as np
import pytest

import cuberef
from cuberef import AXES

B = [tuple(np.array(v, np.float64) for v in f) for f in AXES]
U = 2.0 ** -24


def face_of(v):
    return next(i for i, b in enumerate(B) if (b[0] == v).all())


def geometric(f, x, y, N):
    """include/srz.h's definition in float64: texel (x, y) of face f, one of x, y in {-1, N} (both: the row clamped first) → the texel
    of the neighbour whose centre is n_g + (1 - 1 / N) n_f + (the corner's own coordinate) * (the other axis)"""
    n, su, sv = B[f]
    if not 0 <= x < N and not 0 <= y < N:
        y = min(max(y, 0), N - 1)
    s, t = (2 * x + 1) / N - 1, (2 * y + 1) / N - 1
    if not 0 <= x < N:
        g = face_of(np.sign(s) * su)
        p = B[g][0] + (1 - 1 / N) * n + t * sv
    else:
        g = face_of(np.sign(t) * sv)
        p = B[g][0] + (1 - 1 / N) * n + s * su
    x2, y2 = (p @ B[g][1] + 1) / 2 * N - 0.5, (p @ B[g][2] + 1) / 2 * N - 0.5
    assert abs(x2 - round(x2)) < 1e-9 and abs(y2 - round(y2)) < 1e-9
    return g, int(round(x2)), int(round(y2))


# ------------------------------------------------------------------------------------------------------ faces
KATS = [((1, 0, 0), 0, 0, 0), ((-3, 0, 0), 1, 0, 0), ((0, 2, 0), 2, 0, 0), ((0, -0.5, 0), 3, 0, 0), ((0, 0, 7), 4, 0, 0), ((0, 0, -1), 5, 0, 0),
        ((1, 0.5, 0.25), 0, -0.25, -0.5), ((-2, 1, 0.5), 1, 0.25, -0.5), ((0.5, 4, -1), 2, 0.125, -0.25), ((0.5, -4, -1), 3, 0.125, 0.25),
        ((1, 2, 4), 4, 0.25, -0.5), ((1, 2, -4), 5, -0.25, -0.5), ((3e38, 1.5e38, -3e38), 0, 1.0, -0.5)]


def test_face_table_by_hand(tmp_path):
    r = cuberef.taps(tmp_path, 8, np.float32([k[0] for k in KATS]))
    for i, (d, face, s, t) in enumerate(KATS):
        assert r["face"][i] == face and r["st"][i][0] == np.float32(s) and r["st"][i][1] == np.float32(t), (d, r["face"][i], r["st"][i])
    # and against the (n, su, sv) table: s = d . su / |d . n|
    rng = np.random.default_rng(1)
    d = rng.normal(0, 1, (500, 3)).astype(np.float32)
    r = cuberef.taps(tmp_path, 8, d)
    for i in range(len(d)):
        f = r["face"][i]
        n, su, sv = B[f]
        assert d[i] @ n == np.abs(d[i]).max() and d[i] @ n > 0
        ma = np.float32(d[i] @ n)
        assert r["st"][i][0] == np.float32(d[i] @ su) / ma and r["st"][i][1] == np.float32(d[i] @ sv) / ma
    assert set(r["face"]) == set(range(6))


def test_major_axis_ties_and_signed_zeros(tmp_path):
    cases = [((1, 1, 0), 0), ((1, -1, 0), 0), ((-1, 1, 1), 1), ((1, 1, 1), 0), ((-1, -1, -1), 1), ((0, 1, 1), 2), ((0, -1, 1), 3), ((0, 1, -1), 2),
             ((0.5, 1, 1), 2), ((0.5, 0.25, -0.5), 0), ((-0.0, 0.0, 2), 4), ((0.0, -0.0, -2), 5), ((-0.0, -3, 0.0), 3), ((1, -0.0, 0.0), 0)]
    r = cuberef.taps(tmp_path, 5, np.float32([c[0] for c in cases]))
    assert r["face"].tolist() == [c[1] for c in cases]
    # a zero of either sign in a minor component is the face's centre line: s or t is +-0, the texel indices those of 0
    z = cuberef.taps(tmp_path, 5, np.float32([(1, -0.0, 0.0), (1, 0.0, -0.0)]))
    assert (z["st"] == 0).all() and (z["at"][0] == z["at"][1]).all() and (z["frac"][0] == z["frac"][1]).all()


# ------------------------------------------------------------------------------------------------------ seams
@pytest.mark.parametrize("N", [1, 2, 5, 8])
def test_seam_table_equals_its_geometric_definition(tmp_path, N):
    for f in range(6):
        for i in range(N):
            for (x, y, xe, ye) in ((-1, i, 0, i), (N, i, N - 1, i), (i, -1, i, 0), (i, N, i, N - 1)):
                got, both = cuberef.resolve(tmp_path, N, f, x, y)
                g, x2, y2 = geometric(f, x, y, N)
                assert got == (g, x2, y2) and not both and g != f and g // 2 != f // 2, (f, x, y, got)
                assert 0 <= x2 < N and 0 <= y2 < N
                # crossing back: one step outward from the resolved texel lands on the edge texel it came from
                back = [cuberef.resolve(tmp_path, N, g, x2 + dx, y2 + dy)[0] for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1))
                        if not (0 <= x2 + dx < N and 0 <= y2 + dy < N)]
                assert (f, xe, ye) in back, (f, x, y, got, back)
        for x in range(N):
            for y in range(N):
                assert cuberef.resolve(tmp_path, N, f, x, y) == ((f, x, y), False)
        for (x, y) in ((-1, -1), (N, -1), (-1, N), (N, N)):  # the stated choice: the row clamped, then across in x
            got, both = cuberef.resolve(tmp_path, N, f, x, y)
            assert both and got == geometric(f, x, y, N) == cuberef.resolve(tmp_path, N, f, x, min(max(y, 0), N - 1))[0]


def test_seamless_across_all_twelve_edges(tmp_path):
    """dyadic inputs: N = 8, integer texels, directions (+-1, +-1, k / 16): every product and sum of the lookup is exact, so the word
    through the selected face, through face A and through face B must be identical"""
    N = 8
    cube = np.random.default_rng(1).integers(-8, 9, (6, N, N, 2)).astype(np.float32)
    d, fa, fb = cuberef.edge_dirs()
    assert len(d) == 12 * 29 and len({(a, b) for a, b in zip(fa, fb)}) == 12
    sel = cuberef.sample(tmp_path, cube, d)
    faces = cuberef.taps(tmp_path, N, d)["face"]
    assert (faces == fa).all()  # the tie goes to the first axis of the pair
    for i in range(len(d)):
        a = cuberef.sample(tmp_path, cube, d[i:i + 1], force=int(fa[i]))
        b = cuberef.sample(tmp_path, cube, d[i:i + 1], force=int(fb[i]))
        assert sel[i].tobytes() == a[0].tobytes() == b[0].tobytes(), (d[i], sel[i], a, b)
    assert len(np.unique(sel)) > 30
    # |k| = 15 lies in the vertex region: the lookup stays a convex combination of texels
    v = d.copy()
    v[v == np.float32(14 / 16)] = 15 / 16
    v[v == np.float32(-14 / 16)] = -15 / 16
    v = v[np.abs(v).min(1) == np.float32(15 / 16)]
    got = cuberef.sample(tmp_path, cube, v)
    cls, _ = cuberef.classify(tmp_path, N, 1, np.ones((1, len(v)), np.uint32), v.T.reshape(3, 1, -1))
    assert len(got) == 24 and (got >= cube.min()).all() and (got <= cube.max()).all() and ((cls & cuberef.VERTEX) != 0).all()


def test_smooth_cube_is_reproduced(tmp_path):
    """a cube filled with f = a . d / |d| at N = 8 comes back to bilinear accuracy, edges included: away from the vertex regions the
    error is at most h^2 / 8 (|f_ss| + |f_tt|) with h = 1 / 4 the texel spacing in s and t, and |f_ss|, |f_tt| <= 3 |a| (the second
    derivative of p / |p| along a unit axis is below 3 / |p|^2, |p| >= 1 on the cube); within half a texel of a vertex, where one
    corner is a substituted texel, the result stays inside the cube's range.  cube_dirs is the package's own torch helper"""
    import torch
    from srz.visibility import cube_dirs
    D = cube_dirs(8).numpy()
    assert D.shape == (6, 8, 8, 3) and D.dtype == np.float32 and np.allclose(np.linalg.norm(D, axis=-1), 1, atol=1e-6)
    for f, (n, su, sv) in enumerate(B):  # the centre of texel (x = 6, y = 1)
        p = n + ((2 * 6 + 1) / 8 - 1) * su + ((2 * 1 + 1) / 8 - 1) * sv
        assert np.allclose(D[f, 1, 6], p / np.linalg.norm(p), atol=1e-6)
    # every texel centre samples its own texel
    t = cuberef.taps(tmp_path, 8, D.reshape(-1, 3))
    assert (t["face"] == np.repeat(np.arange(6), 64)).all()
    a = np.float32([0.3, -0.5, 0.8])
    cube = (D @ a)[..., None].astype(np.float32)
    d = np.random.default_rng(2).normal(0, 1, (3000, 3)).astype(np.float32)
    got = cuberef.sample(tmp_path, cube, d)[:, 0]
    err = np.abs(got - (d / np.linalg.norm(d, axis=1, keepdims=True)) @ a)
    cls, _ = cuberef.classify(tmp_path, 8, 1, np.ones((1, len(d)), np.uint32), d.T.reshape(3, 1, -1))
    vertex = (cls[0] & cuberef.VERTEX) != 0
    bound = 0.25 ** 2 / 8 * 6 * float(np.linalg.norm(a))
    print("smooth cube N = 8: max err", err[~vertex].max(), "bound", bound, "vertex region", int(vertex.sum()), err[vertex].max())
    assert 10 <= vertex.sum() <= 1000 and err[~vertex].max() <= bound
    assert (got[vertex] >= cube.min()).all() and (got[vertex] <= cube.max()).all()
    assert isinstance(cube_dirs(1), torch.Tensor) and cube_dirs(1).shape == (6, 1, 1, 3)


# ------------------------------------------------------------------------------------------------------ gradients
def coords64(d, face, N):
    """the texel coordinates (fx, fy) of direction d on `face`, restated in float64"""
    n, su, sv = B[face]
    ma = d @ n
    return ((d @ su) / ma * 0.5 + 0.5) * N - 0.5, ((d @ sv) / ma * 0.5 + 0.5) * N - 0.5


def test_gdir_against_central_differences(tmp_path):
    """gdir against central differences, step h = ma 2^-12 per component, of the float64 restatement with the face and the texels held
    fixed.  With K = N / ma * sum_ch |g| * (the largest difference of two of the four texels) — |d out / d s| <= (N / 2) sum |g| D,
    |d s / d d_i| <= 1 / ma, two in-face axes — the tolerance is K * ((C + 16 + 4 N) 2^-24 + 2^-22): the float32 roundings of the C
    fma steps and of the handful of products and quotients behind them, the rounding of the fractions (fx carries an absolute error of
    about N 2^-24 texels, which moves the cross term of the other axis), and the truncation of the difference quotient, (h / ma)^2 =
    2^-24 times the third derivative of 1 / ma scaled by K, with a factor 4 to spare."""
    rng = np.random.default_rng(3)
    checked = 0
    for N, C in ((1, 3), (2, 1), (5, 4), (8, 7), (64, 3)):
        cube = cuberef.make_cube(5, N, C)
        flat = cube.reshape(-1, C).astype(np.float64)
        d = rng.normal(0, 1, (400, 3)).astype(np.float32)
        g = rng.normal(0, 2, (C, 1, len(d))).astype(np.float32)
        t = cuberef.taps(tmp_path, N, d)
        gdir = cuberef.grad(tmp_path, cube, 1, np.ones((1, len(d)), np.uint32), d.T.reshape(3, 1, -1), g)[:, 0].T
        for i in range(len(d)):
            tx, ty = t["frac"][i]
            if not (0.1 < tx < 0.9 and 0.1 < ty < 0.9):
                continue  # interior points that do not lie near a texel boundary: the step keeps the texels
            face, at = int(t["face"][i]), t["at"][i]
            x0, y0 = t["x0y0"][i]
            tex = flat[at]  # [4, C]

            def f64(dd):
                fx, fy = coords64(dd, face, N)
                a, b = fx - x0, fy - y0
                assert 0 < a < 1 and 0 < b < 1
                top, bot = tex[0] + a * (tex[1] - tex[0]), tex[2] + a * (tex[3] - tex[2])
                return float((top + b * (bot - top)) @ g[:, 0, i].astype(np.float64))

            d64 = d[i].astype(np.float64)
            ma = np.abs(d64).max()
            h = ma * 2.0 ** -12
            fd = np.array([(f64(d64 + h * e) - f64(d64 - h * e)) / (2 * h) for e in np.eye(3)])
            D = np.abs(tex[:, None] - tex[None]).max((0, 1))
            K = N / ma * float(np.abs(g[:, 0, i]).astype(np.float64) @ D)
            tol = K * ((C + 16 + 4 * N) * U + 2.0 ** -22)
            assert (np.abs(gdir[i] - fd) <= tol).all(), (N, C, d[i], gdir[i], fd, tol)
            checked += 1
    assert checked > 500


def test_gdir_is_orthogonal_to_the_direction(tmp_path):
    """the lookup does not depend on the direction's length: dot(gdir, d) = inv (gs sc + gt tc - (gs s + gt t) ma) is 0 in exact
    arithmetic.  In float32 the three products g_i d_i (exact in float64) carry the roundings of inv, of s and t, of gt * t, of the
    fmaf and of the three final products: at most 5 per term and 7 on any pair that must cancel, so |dot| <= 8 * 2^-24 * sum |g_i
    d_i|."""
    rng = np.random.default_rng(4)
    for N, C in ((1, 2), (5, 3), (64, 5)):
        cube = cuberef.make_cube(6, N, C)
        d = (rng.normal(0, 1, (2000, 3)) * 10.0 ** rng.uniform(-3, 3, (2000, 1))).astype(np.float32)
        g = rng.normal(0, 2, (C, 1, len(d))).astype(np.float32)
        gdir = cuberef.grad(tmp_path, cube, 1, np.ones((1, len(d)), np.uint32), d.T.reshape(3, 1, -1), g)[:, 0].T.astype(np.float64)
        prod = gdir * d.astype(np.float64)
        assert (np.abs(prod.sum(1)) <= 8 * U * np.abs(prod).sum(1)).all()
        assert (np.abs(prod).sum(1) > 0).mean() > (0.9 if N > 1 else -1)


def test_gtex_of_one_pixel_and_the_weights(tmp_path):
    rng = np.random.default_rng(5)
    for N in (1, 2, 5, 8):
        d = rng.normal(0, 1, (300, 3)).astype(np.float32)
        t = cuberef.taps(tmp_path, N, d)
        assert (np.abs(t["w"].astype(np.float64).sum(1) - 1.0) <= 2 * 2.0 ** -23).all()  # the four weights sum to 1 within 2 ulp
        assert (t["at"] < 6 * N * N).all()
        cube = cuberef.make_cube(7, N, 2)
        for i in range(0, 300, 7):
            g = rng.normal(0, 2, (2, 1, 1)).astype(np.float32)
            acc = cuberef.Grad(cube.shape)
            cuberef.grad(tmp_path, cube, 1, np.ones((1, 1), np.uint32), d[i].reshape(3, 1, 1), g, into=acc, want_dir=False)
            assert acc.count.sum() == 4
            flat, cnt = acc.gtex.reshape(-1, 2), acc.count.reshape(-1)
            for k in range(4):
                if cnt[t["at"][i][k]] == 1:  # n = 1: exactly the float32 product w_rc * g
                    assert (flat[t["at"][i][k]] == (t["w"][i][k] * g[:, 0, 0]).astype(np.float64)).all()
            assert set(np.flatnonzero(cnt)) == set(t["at"][i].tolist())


# ------------------------------------------------------------------------------------------------------ sampled or not
def test_unsampled_and_extreme_directions(tmp_path):
    N = 5
    cube = cuberef.make_cube(8, N, 3)
    bad = np.float32([(np.nan, 1, 1), (1, np.inf, 0), (0, 1, -np.inf), (0, 0, 0), (-0.0, 0.0, -0.0), (np.nan, np.nan, np.nan), (np.inf, np.inf, 1)])
    assert (cuberef.taps(tmp_path, N, bad)["face"] == -1).all()
    ids = np.ones((1, len(bad)), np.uint32)
    planes = bad.T.reshape(3, 1, -1)
    out = cuberef.forward(tmp_path, cube, 1, ids, planes, prefill=np.full((3, 1, len(bad)), 0x7fc12345, np.uint32))
    assert (out.view(np.uint32) == 0).all()  # written: the pixel has an owner
    acc = cuberef.Grad(cube.shape)
    gd = cuberef.grad(tmp_path, cube, 1, ids, planes, np.ones((3, 1, len(bad)), np.float32), into=acc,
                      prefill=np.full((3, 1, len(bad)), 0x7fc12345, np.uint32))
    assert (gd.view(np.uint32) == 0).all() and acc.count.sum() == 0
    cls, face = cuberef.classify(tmp_path, N, 1, ids, planes)
    assert (cls == cuberef.OWNED).all() and (face == 255).all()
    # nobody: zeros when fused, the words stay when not
    nobody = np.zeros((1, len(bad)), np.uint32)
    pre = np.full((3, 1, len(bad)), 0x7fc12345, np.uint32)
    assert (cuberef.forward(tmp_path, cube, 1, nobody, planes, True, pre).view(np.uint32) == 0).all()
    assert (cuberef.forward(tmp_path, cube, 1, nobody, planes, False, pre).view(np.uint32) == 0x7fc12345).all()
    # 3e38 components sample; subnormal components sample, s and t by the IEEE division (no flush to zero)
    big = np.float32([(3e38, -3e38, 1e38), (-3e38, 3e38, 3e38), (1e30, 3e38, -2e38)])
    r = cuberef.taps(tmp_path, N, big)
    assert r["face"].tolist() == [0, 1, 2] and np.isfinite(cuberef.sample(tmp_path, cube, big)).all()
    tiny = np.array([(1e-40, 2e-41, -3e-42), (-7e-45, 1.4e-45, 4e-45), (3e-39, -6e-39, 6e-39)], np.float32)
    assert (np.abs(tiny) < 2.0 ** -126).all() and (tiny != 0).all()
    r = cuberef.taps(tmp_path, N, tiny)
    assert r["face"].tolist() == [0, 1, 3]
    t64 = tiny.astype(np.float64)
    for i, f in enumerate(r["face"]):
        n, su, sv = B[f]
        assert r["st"][i][0] == np.float32((t64[i] @ su) / (t64[i] @ n)) and r["st"][i][1] == np.float32((t64[i] @ sv) / (t64[i] @ n))
    same_dir = cuberef.sample(tmp_path, cube, tiny[:1] * np.float32(2.0 ** 20))
    assert np.array_equal(cuberef.sample(tmp_path, cube, tiny[:1]), same_dir)  # a power of two: the same s and t
