"""not-gpu: the lighting pass's CPU reference (tests/light_ref.c through lightref.py) is pinned before the GPU is held to it.  Its
binary64 build against the same rule written in torch float64 ops with autograd (both binary64: they differ in the order of
operations only); its binary32 build — the rule itself — against the binary64 build, at 8 x the error measured here; hand KATs."""
import numpy as np
import pytest
import torch

import lightref

SHAPE = (48, 64)
N_TRIS = 7
CASES = ((1, 1), (3, 5), (3, 150), (8, 2))  # (lights, p)
# binary32 against binary64 on well-conditioned pixels, MEASURED on the CPU with the seeds below (the worst of CASES; printed by
# test_binary32_build_against_binary64): the parameter entries relative to sum |term|, the planes relative to the plane's largest
# magnitude.  The tests assert 8 x these, because seeds differ.
MEASURED_PAR, MEASURED_PLANE = 1.41e-6, 1.71e-5  # (both at 3 lights, p = 150: the power's derivative amplifies cs's rounding p-fold)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """per (lights, p): the planes, the parameters, the ids (well-conditioned pixels owned, the others nobody's) and both builds'
    results, computed once"""
    tmp = tmp_path_factory.mktemp("lightref")
    out = {}
    for L, p in CASES:
        nrm, pos, kd, gout = lightref.make_planes(11 + L, SHAPE)
        par = lightref.make_params(5 + L, L)
        good = lightref.well_conditioned(nrm, pos, par)
        ids = np.where(good, np.uint32(3), np.uint32(0))
        r = dict(nrm=nrm, pos=pos, kd=kd, gout=gout, par=par, good=good, ids=ids)
        for name, dt in (("f32", np.float32), ("f64", np.float64)):
            g = lightref.Grad(L)
            fwd = lightref.forward(tmp, N_TRIS, ids, nrm, pos, kd, par, p, dtype=dt)
            planes = lightref.grad(tmp, N_TRIS, ids, nrm, pos, kd, par, p, gout, into=g, dtype=dt)
            r[name] = dict(fwd=fwd, planes=planes, g=g)
        out[(L, p)] = r
    return tmp, out


@pytest.mark.parametrize("case", CASES)
def test_generator_keeps_nine_pixels_in_ten(cases, case):
    """the cap is a condition of the comparison below: a generator that excluded more would test the easy pixels only"""
    good = cases[1][case]["good"]
    assert good.mean() >= 0.9, good.mean()


@pytest.mark.parametrize("case", CASES)
def test_binary64_build_against_torch_autograd(cases, case):
    L, p = case
    r = cases[1][case]
    t = lambda a: torch.tensor(np.float64(a), dtype=torch.float64)  # noqa: E731
    nrm, pos, kd = (t(r[k]).requires_grad_() for k in ("nrm", "pos", "kd"))
    par = t(r["par"])
    eye, ka, ks = (par[i:i + 3].clone().requires_grad_() for i in (0, 3, 6))
    lights = par[9:].reshape(L, 6).clone().requires_grad_()
    mask = t(r["good"])
    out = lightref.torch_rule(nrm, pos, kd, lights, eye, ka, ks, p) * mask
    (out * t(r["gout"])).sum().backward()
    ref = r["f64"]
    scale = lambda a: np.abs(a).max()  # noqa: E731
    o = out.detach().numpy()
    assert np.abs(ref["fwd"] - o).max() <= 1e-9 * scale(o)
    for got, want in zip(ref["planes"], (nrm.grad, pos.grad, kd.grad)):
        want = want.numpy()
        assert np.abs(got - want).max() <= 1e-9 * scale(want)
    g = ref["g"]
    want = np.concatenate([eye.grad.numpy(), ka.grad.numpy(), ks.grad.numpy(), lights.grad.numpy().reshape(-1)])
    assert (g.count[:9] == int(r["good"].sum())).all() and (g.gabs > 0).all()
    assert (np.abs(g.gsum - want) <= 1e-9 * g.gabs).all(), np.abs(g.gsum - want) / g.gabs


def _errors(r):
    a, b = r["f32"], r["f64"]
    par = float((np.abs(a["g"].gsum - b["g"].gsum) / b["g"].gabs).max())
    planes = [(a["fwd"], b["fwd"])] + list(zip(a["planes"], b["planes"]))
    plane = max(float(np.abs(np.float64(x) - y).max() / np.abs(y).max()) for x, y in planes)
    return par, plane


def test_binary32_build_against_binary64(cases):
    """the rule in binary32 against the same operations in binary64 on the same well-conditioned pixels.  No cheap derivation of this
    tolerance exists (about 60 operations, a p-th power, three normalisations): it is measured here and asserted at 8 x"""
    worst_par = worst_plane = 0.0
    for case in CASES:
        par, plane = _errors(cases[1][case])
        print(f"lights {case[0]} p {case[1]}: parameter entries {par:.3g} of sum |term|, planes {plane:.3g} of the plane's max")
        worst_par, worst_plane = max(worst_par, par), max(worst_plane, plane)
    print(f"worst: {worst_par:.3g} {worst_plane:.3g}; recorded {MEASURED_PAR:.3g} {MEASURED_PLANE:.3g}")
    assert worst_par <= 8 * MEASURED_PAR and worst_plane <= 8 * MEASURED_PLANE


def _one(tmp, n, P, kd, par, p, g=(1.0, 1.0, 1.0), dtype=np.float32):
    col = lambda v: None if v is None else np.float32(v).reshape(3, 1, 1)  # noqa: E731
    ids = np.ones((1, 1), np.uint32)
    out = lightref.forward(tmp, 1, ids, col(n), col(P), col(kd), par, p, dtype=dtype)
    acc = lightref.Grad((len(par) - 9) // 6)
    planes = lightref.grad(tmp, 1, ids, col(n), col(P), col(kd), par, p, col(g), into=acc, dtype=dtype)
    return out.reshape(3), planes, acc


@pytest.mark.parametrize("p", (1, 2))
def test_one_light_straight_above_a_flat_normal(cases, p):
    """n = (0, 0, 2), P = 0, the light at (0, 0, 2): Ld = N, cd = 1, att = 1 / 4; the eye at (3, 0, 4): Vd = (0.6, 0, 0.8), Hs = (0.6,
    0, 1.8), cs = 1.8 / sqrt(3.6) = sqrt(0.9), so p = 1 and p = 2 differ: sp = sqrt(0.9) and 0.9"""
    tmp = cases[0]
    I, ka, ks, kd = np.float64([8, 4, 2]), np.float64([0.1, 0.2, 0.3]), np.float64([0.5, 0.25, 1.0]), np.float64([1.0, 0.5, 0.25])
    par = np.float32(np.concatenate([[3, 0, 4], ka, ks, [0, 0, 2], I]))
    out, (gn, gP, gkd), acc = _one(tmp, (0, 0, 2), (0, 0, 0), kd, par, p)
    sp = np.sqrt(0.9) ** p
    E = I / 4
    np.testing.assert_allclose(out, kd * (E + ka * I) + ks * E * sp, rtol=2e-6)
    np.testing.assert_allclose(gkd.reshape(3), E + ka * I, rtol=2e-6)          # d out_c / d kd_c, gout = 1
    np.testing.assert_allclose(acc.gsum[3:6], kd * I, rtol=2e-6)               # ka
    np.testing.assert_allclose(acc.gsum[6:9], E * sp, rtol=2e-6)               # ks
    np.testing.assert_allclose(acc.gsum[12:15], kd * (0.25 + ka) + ks * 0.25 * sp, rtol=2e-6)  # the intensity
    # the normal's gradient is perpendicular to the normal (the rule does not depend on its length); the diffuse cosine is at its
    # maximum, so only the specular term pulls: towards H, that is +x
    assert abs(float(gn.reshape(3)[2])) <= 1e-6 * abs(float(gn.reshape(3)[0])) and gn.reshape(3)[0] > 0 and gn.reshape(3)[1] == 0
    # moving the eye along its own ray changes nothing
    assert abs(float(np.dot(acc.gsum[0:3], [0.6, 0, 0.8]))) <= 1e-6 * np.abs(acc.gsum[0:3]).max()
    # a translation of everything changes nothing: gP + d eye + d light = 0
    np.testing.assert_allclose(np.float64(gP.reshape(3)) + acc.gsum[0:3] + acc.gsum[9:12], 0, atol=1e-6 * np.abs(gP).max())


def test_kd_null_equals_kd_ones_bit_for_bit(cases):
    tmp, c = cases
    r = c[(3, 5)]
    ones = np.ones_like(r["kd"])
    a = lightref.forward(tmp, N_TRIS, r["ids"], r["nrm"], r["pos"], None, r["par"], 5)
    b = lightref.forward(tmp, N_TRIS, r["ids"], r["nrm"], r["pos"], ones, r["par"], 5)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.abs(a).max() > 0
    ga, gb = lightref.Grad(3), lightref.Grad(3)
    pa = lightref.grad(tmp, N_TRIS, r["ids"], r["nrm"], r["pos"], None, r["par"], 5, r["gout"], into=ga)
    pb = lightref.grad(tmp, N_TRIS, r["ids"], r["nrm"], r["pos"], ones, r["par"], 5, r["gout"], into=gb)
    assert pa[2] is None
    for x, y in zip(pa[:2], pb[:2]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(ga.gsum, gb.gsum) and np.array_equal(ga.count, gb.count)


def test_a_skipped_light_equals_the_call_without_it(cases):
    """the middle light so far away that r2 overflows to inf: skipped at every pixel, no term, no gradient"""
    tmp, c = cases
    r = c[(3, 5)]
    far = r["par"].copy()
    far[15:18] = 3e30
    two = np.concatenate([r["par"][:15], r["par"][21:]])
    args = (tmp, N_TRIS, r["ids"], r["nrm"], r["pos"], r["kd"])
    a, b = lightref.forward(*args, far, 5), lightref.forward(*args, two, 5)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    ga, gb = lightref.Grad(3), lightref.Grad(2)
    pa, pb = lightref.grad(*args, far, 5, r["gout"], into=ga), lightref.grad(*args, two, 5, r["gout"], into=gb)
    for x, y in zip(pa, pb):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    keep = np.r_[0:15, 21:27]
    assert np.array_equal(ga.gsum[keep], gb.gsum) and not ga.gsum[15:21].any() and not ga.count[15:21].any()
    cls, lcls = lightref.classify(tmp, N_TRIS, r["ids"], r["nrm"], r["pos"], far, 5)
    own = (cls & lightref.LIT) != 0
    assert own.sum() == r["good"].sum() and ((lcls[1][own] & lightref.SKIPPED) != 0).all() and not (lcls[0][own] & lightref.SKIPPED).any()


def test_unlit_and_nobody_give_zeros_and_no_term(cases):
    tmp = cases[0]
    par = lightref.make_params(1, 1)
    for n in ((0, 0, 0), (np.nan, 0, 1), (np.inf, 0, 1), (1e-30, 0, 0)):  # (1e-30: nn underflows to 0)
        out, planes, acc = _one(tmp, n, (0.1, 0.2, 0), (1, 1, 1), par, 3)
        assert not out.view(np.uint32).any() and not acc.count.any()
        assert all(not q.view(np.uint32).any() for q in planes)
