"""not-gpu: pins tests/prefilter_ref.c, the reference the GPU tests of the cube prefilter compare against: the identities of the rule
(a constant cube, GGX at roughness 1 = COSINE, the roughness clamp), adjointness of the backward in binary64, the cosine lobe of a
linear environment against its closed form, the texels' solid angles against 4 pi, the measured distance of the binary32 build from
the binary64 one, and the outputs that no pair reaches."""
import numpy as np
import pytest

import prefilterref as P
from support import bits

KINDS = [P.COSINE, P.GGX]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [1.0, 2.0 ** -3])
def test_a_constant_cube_stays_that_constant(tmp_path, kind, k):
    """fmaf(w, k, num) and den + w round alike for a power of two k, so num == k * den exactly and the quotient is k, wherever some
    pair was taken; with a cutoff that leaves outputs empty, those are 0"""
    for n_src, n_dst, r, cmin in [(8, 8, 0.3, 0.0), (5, 2, 0.0625, 0.5), (3, 8, 0.5, 0.97)]:
        cube = np.full((6, n_src, n_src, 2), k, np.float32)
        out, den, count = P.forward(tmp_path, cube, n_dst, kind, r, cmin)
        assert ((den > 0) == (count > 0)).all()
        assert (out[den > 0] == np.float32(k)).all() and not bits(out[den == 0]).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ggx_at_roughness_one_is_the_cosine_lobe_and_the_roughness_clamps(tmp_path, dtype):
    rng = np.random.default_rng(1)
    cube = rng.uniform(0, 1, (2, 6, 5, 5, 3))
    g = rng.uniform(-1, 1, (2, 6, 4, 4, 3))
    word = np.uint32 if dtype == np.float32 else np.uint64
    for cmin in (0.0, 0.5):
        cos = P.forward(tmp_path, cube, 4, P.COSINE, 0.3, cmin, dtype)  # (the cosine lobe ignores the roughness)
        one = P.forward(tmp_path, cube, 4, P.GGX, 1.0, cmin, dtype)
        zero = P.forward(tmp_path, cube, 4, P.GGX, 0.0, cmin, dtype)
        low = P.forward(tmp_path, cube, 4, P.GGX, 0.0625, cmin, dtype)
        for a, b in zip(cos + zero, one + low):
            assert np.array_equal(a.view(word) if a.dtype == dtype else a, b.view(word) if b.dtype == dtype else b)
        assert not np.array_equal(one[0], low[0])
        grads = [P.grad(tmp_path, g, den, 5, kind, r, cmin, dtype) for kind, r, den in
                 [(P.COSINE, 0.3, cos[1]), (P.GGX, 1.0, one[1]), (P.GGX, 0.0, zero[1]), (P.GGX, 0.0625, low[1])]]
        assert np.array_equal(grads[0].view(word), grads[1].view(word)) and np.array_equal(grads[2].view(word), grads[3].view(word))


@pytest.mark.parametrize("kind,r,cmin", [(P.COSINE, 1.0, 0.0), (P.GGX, 0.25, 0.0), (P.GGX, 0.5, 0.5), (P.GGX, 0.5, 0.97)])
def test_the_backward_is_the_transpose_in_binary64(tmp_path, kind, r, cmin):
    """<gdst, P src> = <P^T gdst, src> to 1e-12 relative"""
    rng = np.random.default_rng(2)
    for n_src, n_dst in [(7, 4), (3, 8)]:
        src = rng.uniform(-1, 1, (2, 6, n_src, n_src, 3))
        gdst = rng.uniform(-1, 1, (2, 6, n_dst, n_dst, 3))
        out, den, _ = P.forward(tmp_path, src, n_dst, kind, r, cmin, np.float64)
        gsrc = P.grad(tmp_path, gdst, den, n_src, kind, r, cmin, np.float64)
        lhs, rhs = float((gdst * out).sum()), float((gsrc * src).sum())
        scale = float(np.abs(gdst * out).sum())
        assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)


# the cosine lobe of the linear environment a + b.d is a + (2 / 3) b.n; the distance is discretisation only.  Measured with this
# reference in binary64, n_dst 8, a = 0.7, b = (0.3, -0.4, 0.33), |b| = 0.599: the values below; asserted at twice that, and falling
LINEAR_MEASURED = {8: 3.02e-4, 16: 3.18e-5, 32: 7.48e-6}


def test_the_cosine_lobe_of_a_linear_environment(tmp_path):
    a, b = 0.7, np.array([0.3, -0.4, 0.33])
    do, _ = P.geometry(tmp_path, 8, np.float64)
    exact = a + (2.0 / 3.0) * (do @ b)
    errs = []
    for n_src, measured in LINEAR_MEASURED.items():
        d, _ = P.geometry(tmp_path, n_src, np.float64)
        out, _, _ = P.forward(tmp_path, (a + d @ b)[..., None], 8, P.COSINE, dtype=np.float64)
        errs.append(float(np.abs(out[..., 0] - exact).max()))
        print(f"n_src {n_src}: max |out - closed form| {errs[-1]:.3e}")
        assert errs[-1] <= 2 * measured
    assert errs[0] > errs[1] > errs[2]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_texels_solid_angles_sum_to_the_sphere(tmp_path, dtype):
    """sum jac * 4 / N^2 against 4 pi: the midpoint rule's ratios (numpy: 1.0153, 1.0038, 1.00096, 1.00024), and unit directions"""
    for n, ratio in [(4, 1.0153), (8, 1.0038), (16, 1.00096), (32, 1.00024)]:
        d, jac = P.geometry(tmp_path, n, dtype)
        got = float(jac.astype(np.float64).sum()) * 4 / n ** 2 / (4 * np.pi)
        assert abs(got - ratio) <= 1e-3, (n, got)
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1).max() <= (2e-7 if dtype == np.float32 else 1e-15)
    d, _ = P.geometry(tmp_path, 2, np.float32)  # the faces' axes: texel (0, 0) of +X lies towards +y, +z, of -Z towards +x, +y
    assert (d[0, 0, 0] > 0).all() and (d[5, 0, 0] * [1, 1, -1] > 0).all()


# binary32 against binary64, random texels in [0, 1], random gradients in [-1, 1], n_src 32 -> n_dst 8, relative to the plane's
# largest magnitude: no bound is derived, these are the maxima MEASURED with this reference (dst, den, gsrc); asserted at 8 x.  The
# narrow lobe is the worst: t = fma(nh2, a2 - 1, 1) cancels to about a2 = 1.5e-5 at c near 1.
F32_MEASURED = {(P.COSINE, 0.0625): (3.6e-7, 3.0e-7, 5.3e-7), (P.COSINE, 0.25): (3.6e-7, 3.0e-7, 5.3e-7), (P.COSINE, 0.5): (3.6e-7, 3.0e-7, 5.3e-7),
                (P.COSINE, 1.0): (3.6e-7, 3.0e-7, 5.3e-7), (P.GGX, 0.0625): (1.9e-4, 5.5e-4, 5.7e-4), (P.GGX, 0.25): (2.3e-6, 7.9e-6, 2.1e-5),
                (P.GGX, 0.5): (4.0e-7, 7.0e-7, 1.5e-6), (P.GGX, 1.0): (3.6e-7, 3.0e-7, 5.3e-7)}


@pytest.fixture(scope="module")
def f32_inputs():
    rng = np.random.default_rng(5)
    return rng.uniform(0, 1, (6, 32, 32, 3)).astype(np.float32), rng.uniform(-1, 1, (6, 8, 8, 3)).astype(np.float32)


@pytest.mark.parametrize("kind,r", sorted(F32_MEASURED))
def test_binary32_against_binary64(tmp_path, f32_inputs, kind, r):
    cube, g = f32_inputs
    o32, d32, _ = P.forward(tmp_path, cube, 8, kind, r)
    o64, d64, _ = P.forward(tmp_path, cube, 8, kind, r, dtype=np.float64)
    g32 = P.grad(tmp_path, g, d32, 32, kind, r)
    g64 = P.grad(tmp_path, g, d64, 32, kind, r, dtype=np.float64)
    rel = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in ((o32, o64), (d32, d64), (g32, g64))]
    print(f"kind {kind} roughness {r}: relative dst {rel[0]:.3e} den {rel[1]:.3e} gsrc {rel[2]:.3e}")
    assert all(x <= 8 * m for x, m in zip(rel, F32_MEASURED[kind, r])), rel


def test_outputs_that_no_pair_reaches(tmp_path):
    """a narrow cutoff over a coarse source: the share of output texels without a single pair is 31 %, 20 % and 100 % (numpy
    restatement); those outputs are exactly 0 and so is their share of the backward"""
    rng = np.random.default_rng(3)
    shares = []
    for n_src, n_dst, kind, r, cmin in P.EMPTY_CASES:
        cube = rng.uniform(0.5, 1, (6, n_src, n_src, 2)).astype(np.float32)
        out, den, count = P.forward(tmp_path, cube, n_dst, kind, r, cmin)
        empty = count == 0
        shares.append(float(empty.mean()))
        assert ((den == 0) == empty).all() and not bits(out[empty]).any() and (out[~empty] > 0).all()
        # a gradient on the empty outputs alone reaches nothing; on all of them it is what the others alone give
        g = rng.uniform(0.5, 1, out.shape).astype(np.float32)
        assert not bits(P.grad(tmp_path, np.where(empty[..., None], g, 0), den, n_src, kind, r, cmin)).any()
        assert np.array_equal(bits(P.grad(tmp_path, g, den, n_src, kind, r, cmin)),
                              bits(P.grad(tmp_path, np.where(empty[..., None], 0, g), den, n_src, kind, r, cmin)))
    assert 0.1 < shares[0] < 0.6 and 0.1 < shares[1] < 0.6 and shares[2] == 1.0, shares
