"""not-gpu: the SH9 passes' reference (tests/sh_ref.c through tests/shref.py) against mathematics, against the cosine prefilter's
reference, against torch autograd, and its binary32 build against its binary64 build.  Nothing of the product runs here."""
import numpy as np
import pytest
import torch

import prefilterref
import shref

U = 2.0 ** -24
N_TRIS = 5
KMAX = float(shref.YC.max())


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("shref")


def order2_cube(n, coef):
    """the cube [1, 6, n, n, C] of the order-2 function with the coefficients coef [9, C], sampled at the texel centres in float64"""
    d, _ = shref.cube_geometry(n)
    return np.einsum("kfyx,kc->fyxc", shref.basis(d), coef)[None]


def smooth_env(n):
    """a smooth environment that is NOT band-limited: an exponential lobe, a product of sines, a narrow lobe about +y"""
    (x, y, z), _ = shref.cube_geometry(n)
    return np.stack([np.exp(1.5 * (0.6 * x + 0.3 * y + 0.74 * z)), 1.0 + 0.5 * np.sin(3 * x) * np.cos(2 * y) + 0.3 * z ** 3,
                     np.exp(-2 * (1 - y))], -1)[None]


def test_the_numpy_geometry_is_the_c_text(tmp):
    """cube_geometry (numpy, for the tests' own environments) against prefilter_ref.c's geometry in binary64"""
    for n in (1, 3, 8):
        d, jac = shref.cube_geometry(n)
        dr, jr = prefilterref.geometry(tmp, n, np.float64)
        assert np.allclose(d.transpose(1, 2, 3, 0), dr, rtol=0, atol=4e-16) and np.allclose(jac, jr, rtol=2e-15, atol=0)


@pytest.mark.parametrize("n", [1, 8, 33])
def test_a_constant_environment(tmp, n):
    """L everywhere: sh[0] = FOURPI Yc0 L up to rounding, and the other eight vanish — every one of their polynomials is odd in some
    axis or sums to zero over the cube's symmetric texel set, so only rounding is left: 6 n^2 terms of size <= 1.1 L jac, bounded
    here by 6 n^2 eps L.  The irradiance is then L at every normal."""
    L = np.array([1.75, 0.3])
    cube = np.broadcast_to(L, (1, 6, n, n, 2))
    sh, den = shref.cube_sh(tmp, cube, np.float64)
    eps = np.finfo(np.float64).eps
    assert np.allclose(sh[0, 0], shref.FOURPI * shref.YC[0] * L, rtol=(6 * n * n + 8) * eps, atol=0)
    assert np.abs(sh[0, 1:]).max() <= 6 * n * n * eps * shref.FOURPI * L.max()
    _, jac = shref.cube_geometry(n)
    assert np.isclose(den[0], jac.sum(), rtol=(6 * n * n) * eps)
    nrm = np.random.default_rng(1).normal(0, 1, (3, 4, 5))
    ids = np.ones((4, 5), np.uint32)
    irr = shref.forward(tmp, N_TRIS, ids, nrm, sh[0], shref.IRRADIANCE, dtype=np.float64)
    # H0 Yc0 FOURPI = 1 up to the constants' binary32 rounding, three of them
    assert np.allclose(irr, L.reshape(2, 1, 1) * np.ones((2, 4, 5)), rtol=4 * U, atol=6 * 33 * 33 * eps * 4 * L.max())


def test_an_order_2_function_comes_back_as_its_coefficients(tmp):
    """the midpoint rule over the texels is second order in 1 / n: the binary64 reference's largest coefficient error at n = 8 was
    4.87e-3, at n = 32 2.95e-4, at n = 64 7.35e-5 — a ratio of 16.5 between 8 and 32 (16 is the second-order figure).  Asserted with
    margin 2: the error at 32 is at most the error at 8 over 8.25."""
    coef = np.random.default_rng(5).normal(0, 1, (9, 3))
    err = {}
    for n in (8, 32):
        sh, _ = shref.cube_sh(tmp, order2_cube(n, coef), np.float64)
        err[n] = np.abs(sh[0] - coef).max()
    print("order-2 projection errors", err, "ratio", err[8] / err[32])
    assert 0 < err[32] <= err[8] / 8.25


def test_radiance_reproduces_the_function(tmp):
    """RADIANCE evaluation of coefficients IS the function sum coef_k Yc_k p_k: against numpy in binary64, to rounding"""
    rng = np.random.default_rng(6)
    coef = rng.normal(0, 1, (9, 3))
    nrm = rng.normal(0, 1, (3, 6, 7)) * rng.uniform(0.3, 4, (1, 6, 7))
    N = nrm / np.sqrt((nrm * nrm).sum(0))
    want = np.einsum("kyx,kc->cyx", shref.basis(N), coef)
    got = shref.forward(tmp, N_TRIS, np.ones((6, 7), np.uint32), nrm, coef, shref.RADIANCE, dtype=np.float64)
    assert np.allclose(got, want, rtol=0, atol=64 * np.finfo(np.float64).eps * np.abs(coef).sum(0).max() * 2 * KMAX)
    # and the round trip: project the function at n = 64, evaluate — the quadrature error of the projection, 7.35e-5 per
    # coefficient with margin 2, times the basis' size
    sh, _ = shref.cube_sh(tmp, order2_cube(64, coef), np.float64)
    back = shref.forward(tmp, N_TRIS, np.ones((6, 7), np.uint32), nrm, sh[0], shref.RADIANCE, dtype=np.float64)
    assert np.abs(back - want).max() <= 9 * 2 * KMAX * 2 * 7.36e-5


def test_irradiance_against_the_cosine_prefilter(tmp):
    """SH9 irradiance against prefilterref's COSINE prefilter (the brute cosine-normalised sum), both binary64, on a smooth
    environment that is not band-limited, N = 32 looked up on an 8 x 8 cube: the two differed by 7.6e-4 of the largest value
    (channel by channel 7.6e-4, 3.8e-6, 1.56e-3 of the channel's own largest).  Asserted with margin 2: 1.52e-3 of the largest
    value.  The order-2 truncation is the difference; Ramamoorthi and Hanrahan's 1 % is its expected order."""
    env = smooth_env(32)
    sh, _ = shref.cube_sh(tmp, env, np.float64)
    dst, _, _ = prefilterref.forward(tmp, env, 8, prefilterref.COSINE, dtype=np.float64)
    d8, _ = shref.cube_geometry(8)
    ids = np.ones((6 * 8, 8), np.uint32)
    irr = shref.forward(tmp, N_TRIS, ids, d8.reshape(3, 48, 8), sh[0], shref.IRRADIANCE, dtype=np.float64)
    irr = irr.reshape(3, 6, 8, 8).transpose(1, 2, 3, 0)
    diff = np.abs(irr - dst[0]).max() / np.abs(dst[0]).max()
    print("irradiance against the cosine prefilter: of the largest value", diff)
    assert diff <= 1.52e-3


@pytest.mark.parametrize("kind", [shref.IRRADIANCE, shref.RADIANCE])
@pytest.mark.parametrize("n_ch", [1, 3, 7])
def test_binary64_build_against_torch_autograd(tmp, kind, n_ch):
    """the float64 torch_rule's forward and autograd against the reference's forward, gnrm and gsh"""
    shape = (9, 11)
    nrm, gout = shref.make_planes(3, shape, n_ch)
    nrm[:, 0, 0] = 0  # not lit
    sh = shref.make_sh(4, n_ch)
    ids = np.ones(shape, np.uint32)
    ids[2, 3] = 0  # nobody
    fwd = shref.forward(tmp, N_TRIS, ids, nrm, sh, kind, dtype=np.float64)
    acc = shref.Grad(n_ch)
    gn = shref.grad(tmp, N_TRIS, ids, nrm, sh, kind, gout, into=acc, dtype=np.float64)
    t_sh = torch.tensor(sh, dtype=torch.float64, requires_grad=True)
    t_n = torch.tensor(nrm, dtype=torch.float64, requires_grad=True)
    owned = torch.tensor(ids != 0)
    out = shref.torch_rule(t_sh, t_n, kind) * owned
    out.backward(torch.tensor(gout, dtype=torch.float64))
    assert np.allclose(out.detach().numpy(), fwd, rtol=1e-12, atol=1e-12)
    assert np.allclose(t_n.grad.numpy(), gn, rtol=1e-10, atol=1e-11)
    assert np.allclose(t_sh.grad.numpy(), acc.gsum, rtol=1e-10, atol=1e-11)
    assert (acc.count == ids.size - 2).all() and (fwd[:, 0, 0] == 0).all() and (gn[:, 2, 3] == 0).all()


@pytest.mark.parametrize("n,n_ch,frames", [(1, 1, 1), (3, 3, 2), (8, 7, 1), (65, 2, 1)])
def test_cube_backward_against_torch_autograd(tmp, n, n_ch, frames):
    """cube_sh's backward is the derivative of its forward: the float64 torch_cube_rule's autograd against cube_sh_grad; and the
    rule's forward against the fixed tree's"""
    cube = shref.make_cube(7, n, n_ch, frames)
    sh, den = shref.cube_sh(tmp, cube, np.float64)
    gsh = np.random.default_rng(8).normal(0, 1, sh.shape)
    gsrc = shref.cube_sh_grad(tmp, gsh, den, n, np.float64)
    t = torch.tensor(cube, dtype=torch.float64, requires_grad=True)
    out = shref.torch_cube_rule(t)
    out.backward(torch.tensor(gsh))
    assert np.allclose(out.detach().numpy(), sh, rtol=1e-12, atol=1e-12)
    assert np.allclose(t.grad.numpy(), gsrc, rtol=1e-12, atol=1e-13)


def cube_bound(cube, n):
    """the rounding bound of binary32 cube_sh against binary64, per channel [C]: a weight w_k = jac Yc p_k carries at most 16
    roundings of size u relative to 1.1 jac (s, t: 2 each; r2: 2; the root and the division; d: 1; jac: 2; the polynomial: 3, on
    values up to 2; Yc and jac products: 2); the tree adds at most ceil(n / 64) + 6 + n + 6 roundings per term, twice (num and den);
    FOURPI *, / : 2 more.  All relative to FOURPI sum(1.1 jac |src|) / den."""
    _, jac = shref.cube_geometry(n)
    depth = -(-n // 64) + n + 12
    return (16 + 2 * depth + 4) * U * shref.FOURPI * 1.1 * 2 * np.einsum("fyx,bfyxc->bc", jac, np.abs(np.float64(cube))) / jac.sum()


@pytest.mark.parametrize("n,n_ch,frames", [(1, 1, 1), (3, 3, 2), (8, 7, 1), (65, 2, 1), (130, 1, 1)])
def test_cube_binary32_build_against_binary64(tmp, n, n_ch, frames):
    cube = shref.make_cube(9, n, n_ch, frames)
    sh32, den32 = shref.cube_sh(tmp, cube, np.float32)
    sh64, den64 = shref.cube_sh(tmp, cube, np.float64)
    bound = cube_bound(cube, n)
    ratio = (np.abs(sh32 - sh64) / bound[:, None, :]).max()
    print("cube_sh binary32 against binary64: error over bound", ratio)
    assert ratio <= 1
    assert abs(float(den32[0]) - den64[0]) <= (n + 16) * U * den64[0]
    gsh = np.random.default_rng(10).normal(0, 1, sh32.shape).astype(np.float32)
    g32 = shref.cube_sh_grad(tmp, gsh, den32, n, np.float32)
    g64 = shref.cube_sh_grad(tmp, gsh, den64, n, np.float64)
    # a texel's gradient: nine terms w_k q_k, each with the weight's 16 roundings, q's 2 + den's, the chain's 9
    gb = (16 + n + 16 + 3 + 9) * U * 1.1 * 2 * shref.FOURPI * np.abs(np.float64(gsh)).sum(1) / den64[0]  # [frames, C], times jac <= 1
    assert (np.abs(g32 - g64) <= gb[:, None, None, None, :]).all()


@pytest.mark.parametrize("kind", [shref.IRRADIANCE, shref.RADIANCE])
def test_pixel_binary32_build_against_binary64(tmp, kind):
    """binary32 against binary64 on normals of ordinary length.  N carries 6 roundings (the dot: 3, the root, the division, the
    product), a polynomial of values up to 2 at most 3 more on top of its arguments' (2 x 6), the constant 1: delta e_k <= 24 u 2
    Kmax; the chain of nine fmafs adds 9 u of sum |sh_k e_k|.  So |out32 - out64| <= 33 u 2 Kmax sum_k |sh_k|.  The terms g e_k: 25 u
    |g| 2 Kmax.  gnrm: gN is four products of gp = ge K with ge = sum_c g_c sh_kc and factors up to 6, so |gN_i| <= 24 G with G =
    Kmax sum |g_c| |sh_kc|; the projection and the scale by inl keep that size times inl (times 4: the dot's three terms and gN itself);
    every operand carries the roundings above plus C for the channel sum: (C + 64) u in all."""
    n_ch, shape = 3, (16, 24)
    nrm, gout = shref.make_planes(11, shape, n_ch)
    sh = shref.make_sh(12, n_ch)
    ids = np.ones(shape, np.uint32)
    f32 = shref.forward(tmp, N_TRIS, ids, nrm, sh, kind)
    f64 = shref.forward(tmp, N_TRIS, ids, nrm, sh, kind, dtype=np.float64)
    S = np.abs(np.float64(sh)).sum(0).reshape(n_ch, 1, 1)
    assert (np.abs(f32 - f64) <= 33 * U * 2 * KMAX * S).all()
    a32, a64 = shref.Grad(n_ch), shref.Grad(n_ch)
    gn32, t32 = shref.grad(tmp, N_TRIS, ids, nrm, sh, kind, gout, into=a32, want_terms=True)
    gn64, t64 = shref.grad(tmp, N_TRIS, ids, nrm, sh, kind, gout, into=a64, want_terms=True, dtype=np.float64)
    assert (np.abs(t32 - t64) <= 25 * U * 2 * KMAX * np.abs(np.float64(gout))[None]).all()
    G = KMAX * np.einsum("cyx,kc->yx", np.abs(np.float64(gout)), np.abs(np.float64(sh)))
    inl = 1.0 / np.sqrt((np.float64(nrm) ** 2).sum(0))
    assert (np.abs(gn32 - gn64) <= (n_ch + 64) * U * 4 * 24 * G * inl).all()
    # the double accumulations of the two builds' terms differ by the terms' differences
    assert (np.abs(a32.gsum - a64.gsum) <= 25 * U * 2 * KMAX * np.abs(np.float64(gout)).sum((1, 2))[None]).all()


def test_unlit_and_nobody_give_zeros_and_no_term(tmp):
    """every SPECIAL_NORMALS row by the binary32 rule: lit or not as the header says; a pixel that is not lit, and nobody's, gives
    zeros, a zero gradient and no term"""
    sp = shref.SPECIAL_NORMALS
    lit_want = np.array([0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1], bool)
    nrm = np.ascontiguousarray(sp.T.reshape(3, 1, len(sp)))
    ids = np.ones((1, len(sp)), np.uint32)
    cls = shref.classify(tmp, N_TRIS, ids, nrm)
    assert ((cls & shref.LIT) != 0).reshape(-1).tolist() == lit_want.tolist()
    sh = shref.make_sh(13, 2)
    gout = np.ones((2, 1, len(sp)), np.float32)
    out = shref.forward(tmp, N_TRIS, ids, nrm, sh, shref.IRRADIANCE)
    acc = shref.Grad(2)
    gn, terms = shref.grad(tmp, N_TRIS, ids, nrm, sh, shref.IRRADIANCE, gout, into=acc, want_terms=True)
    dark = ~lit_want
    assert (out[:, 0, dark].view(np.uint32) == 0).all() and (gn[:, 0, dark].view(np.uint32) == 0).all() and (terms[:, :, 0, dark] == 0).all()
    assert (acc.count == lit_want.sum()).all() and np.isfinite(out).all() and np.isfinite(gn).all()
    # nobody: untouched without the fused clear, zeros with it
    pre = np.full((2, 1, len(sp)), 0x7fc0dead, np.uint32)
    none = np.zeros_like(ids)
    kept = shref.forward(tmp, N_TRIS, none, nrm, sh, shref.IRRADIANCE, fused=False, prefill=pre)
    assert (kept.view(np.uint32) == pre).all()
    assert (shref.forward(tmp, N_TRIS, none, nrm, sh, shref.IRRADIANCE, fused=True, prefill=pre).view(np.uint32) == 0).all()


def test_a_nan_texel_reaches_its_own_channel_and_frame_only(tmp):
    cube = shref.make_cube(14, 5, 3, 2)
    cube[1, 2, 3, 4, 1] = np.nan
    sh, den = shref.cube_sh(tmp, cube)
    nan = np.isnan(sh)
    want = np.zeros_like(nan)
    want[1, :, 1] = True
    assert np.array_equal(nan, want) and np.isfinite(den).all()
