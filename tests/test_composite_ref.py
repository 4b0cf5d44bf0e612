"""not-gpu: the depth-layer composite's CPU reference (tests/composite_ref.c through tests/compositeref.py) pinned without the
library: against an op-by-op numpy restatement, a hand case, central differences and torch's float64 autograd through the existing
srz.visibility.composite; and the measured binary32-against-binary64 error of the gradients that the device's autograd test uses."""
import numpy as np
import pytest
import torch

import compositeref as cr


def val(a):
    """the one element of a one-element array"""
    return np.asarray(a).reshape(-1)[0].item()


def case(seed, n_layers, n_ch, shape=(2, 5, 7), scalar=(), dtype=np.float32, cover=0.6, lo=0.0, hi=1.0):
    """random layers: coverage with probability `cover`, colours and alphas in [lo, hi], the layers in `scalar` with a scalar opacity"""
    rng = np.random.default_rng(seed)
    n, rows, W = shape
    covs = [rng.random((n, rows, W)) < cover for _ in range(n_layers)]
    colors = [rng.uniform(lo, hi, (n, n_ch, rows, W)).astype(dtype) for _ in range(n_layers)]
    alphas = [float(np.float32(rng.uniform(lo, hi))) if k in scalar else rng.uniform(lo, hi, (n, 1, rows, W)).astype(dtype)
              for k in range(n_layers)]
    bg = rng.uniform(lo, hi, (n, n_ch, rows, W)).astype(dtype)
    return covs, colors, alphas, bg, rng


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n_layers, n_ch, with_bg, through", [(1, 1, False, False), (2, 3, True, False), (3, 5, True, True), (8, 3, False, True),
                                                              (8, 64, True, True)])
def test_binary32_is_the_numpy_restatement(tmp_path_factory, n_layers, n_ch, with_bg, through):
    tmp = tmp_path_factory.getbasetemp()
    covs, colors, alphas, bg, rng = case(11 + n_layers, n_layers, n_ch, shape=(2, 3, 5), scalar=(1, 4), lo=-1.0, hi=2.0)
    bg = bg if with_bg else None
    out = cr.forward(tmp, covs, colors, alphas, bg, through)
    assert np.array_equal(bits(out), bits(cr.numpy_forward(covs, colors, alphas, bg, through)))
    gout = rng.uniform(-1, 1, out.shape).astype(np.float32)
    got, want = cr.grad(tmp, covs, colors, alphas, gout, bg, through), cr.numpy_grad(covs, colors, alphas, gout, bg, through)
    for k in range(n_layers):
        assert np.array_equal(bits(got[0][k]), bits(want[0][k])), ("gcolor", k)
        assert np.array_equal(bits(got[1][k]), bits(want[1][k])), ("galpha", k)
    if with_bg:
        assert np.array_equal(bits(got[2]), bits(want[2]))
    else:
        assert got[2] is None


def test_cover_is_the_passes_owner_test(tmp_path_factory):
    ids = np.uint32([[[0, 1, 5, 6, 0x80000000, 0x80000001, 0x80000005, 0x80000006, 0xffffffff, 0x7fffffff]]])
    cov = cr.cover(tmp_path_factory.getbasetemp(), ids, [5])
    assert cov.tolist() == [[[False, True, True, False, False, True, True, False, False, False]]]


def test_hand_case_two_layers_one_pixel(tmp_path_factory):
    """a0 = 0.5, a1 = 0.25, colours 2 and 4, bg 8: w0 = 0.5, T = 0.5, w1 = 0.125, T = 0.375; out = 1 + 0.5 + 3 = 4.5"""
    tmp = tmp_path_factory.getbasetemp()
    one = lambda v: np.full((1, 1, 1, 1), v, np.float32)  # noqa: E731
    covs = [np.ones((1, 1, 1), bool)] * 2
    colors, alphas, bg = [one(2), one(4)], [one(0.5), 0.25], one(8)
    out = cr.forward(tmp, covs, colors, alphas, bg, True)
    assert out.reshape(-1).tolist() == [4.5, 0.375]
    # g = 1, gT = 2: gbg = T_n = 0.375; S = 2 + 8 = 10; layer 1: d = 4, gcol = w1 = 0.125, galpha = T_1 (4 - 10) = -3,
    # S = 0.25 * 4 + 0.75 * 10 = 8.5; layer 0: d = 2, gcol = 0.5, galpha = 1 * (2 - 8.5) = -6.5
    gcol, galpha, gbg = cr.grad(tmp, covs, colors, alphas, np.float32([1, 2]).reshape(1, 2, 1, 1), bg, True)
    assert [val(gcol[0]), val(gcol[1]), val(galpha[0]), val(galpha[1]), val(gbg)] == [0.5, 0.125, -6.5, -3.0, 0.375]
    # the second layer not covering: skipped, the pixel is layer 0 over bg, and its gradients are +0
    covs = [covs[0], np.zeros((1, 1, 1), bool)]
    assert cr.forward(tmp, covs, colors, alphas, bg, True).reshape(-1).tolist() == [5.0, 0.5]
    gcol, galpha, gbg = cr.grad(tmp, covs, colors, alphas, np.float32([1, 2]).reshape(1, 2, 1, 1), bg, True)
    assert bits(gcol[1]).item() == 0 and bits(galpha[1]).item() == 0 and val(galpha[0]) == 2.0 - 10.0 and val(gbg) == 0.5


def loss64(tmp, covs, colors, alphas, bg, through, gout):
    return float((cr.forward(tmp, covs, colors, alphas, bg, through, np.float64) * gout).sum())


@pytest.mark.parametrize("through", [False, True])
@pytest.mark.parametrize("with_bg", [False, True])
def test_binary64_gradients_are_central_differences_and_torch_autograd(tmp_path_factory, with_bg, through):
    tmp = tmp_path_factory.getbasetemp()
    covs, colors, alphas, bg, rng = case(5, 3, 3, shape=(1, 2, 3), scalar=(1,), dtype=np.float64, cover=0.7)
    bg = bg if with_bg else None
    gout = rng.uniform(-1, 1, (1, 3 + through, 2, 3))
    gcol, galpha, gbg = cr.grad(tmp, covs, colors, alphas, gout, bg, through, np.float64)

    def rel(got, want):
        return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
    # central differences: the loss is linear in every single input word, so any step is exact up to rounding
    h = 0.25

    def diff(arr, setter=None):
        d = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            keep = arr[i]
            arr[i] = keep + h
            up = loss64(tmp, covs, colors, alphas, bg, through, gout)
            arr[i] = keep - h
            dn = loss64(tmp, covs, colors, alphas, bg, through, gout)
            arr[i] = keep
            d[i] = (up - dn) / (2 * h)
        return d
    for k in range(3):
        assert rel(gcol[k], diff(colors[k])) <= 1e-9, ("gcolor", k)
        if k != 1:
            assert rel(galpha[k], diff(alphas[k])) <= 1e-9, ("galpha", k)
    keep = alphas[1]
    alphas[1] = keep + h
    up = loss64(tmp, covs, colors, alphas, bg, through, gout)
    alphas[1] = keep - h
    dn = loss64(tmp, covs, colors, alphas, bg, through, gout)
    alphas[1] = keep
    assert abs(galpha[1].sum() - (up - dn) / (2 * h)) <= 1e-9 * abs(galpha[1].sum()), "the scalar's gradient is its plane's sum"
    if with_bg:
        assert rel(gbg, diff(bg)) <= 1e-9
    # torch float64 autograd through the existing composite, coverage folded into the alphas
    from srz.visibility import composite
    tc = [torch.tensor(c, requires_grad=True) for c in colors]
    ta = [torch.tensor(np.full((1, 1, 2, 3), a) if np.isscalar(a) else a, requires_grad=True) for a in alphas]
    tb = None if bg is None else torch.tensor(bg, requires_grad=True)
    eff = [a * torch.tensor(c[:, None].astype(np.float64)) for a, c in zip(ta, covs)]
    out = composite(tc, eff)
    T = torch.ones_like(eff[0])
    for e in eff:
        T = T * (1 - e)
    if tb is not None:
        out = out + T * tb
    tg = torch.tensor(gout)
    loss = (out * tg[:, :3]).sum() + ((T * tg[:, 3:]).sum() if through else 0.0)
    loss.backward()
    for k in range(3):
        assert rel(gcol[k], tc[k].grad.numpy()) <= 1e-9 and rel(galpha[k], ta[k].grad.numpy()) <= 1e-9, k
    if with_bg:
        assert rel(gbg, tb.grad.numpy()) <= 1e-9


def test_an_opaque_front_layer_still_gets_its_alpha_gradient(tmp_path_factory):
    """a = 1 in layer 0: T_1 = 0, nothing behind shows, and still galpha_0 = T_0 (d_0 - S) with the layers behind it in S"""
    tmp = tmp_path_factory.getbasetemp()
    one = lambda v: np.full((1, 1, 1, 1), v, np.float32)  # noqa: E731
    covs = [np.ones((1, 1, 1), bool)] * 3
    colors, alphas, bg = [one(3), one(5), one(7)], [one(1.0), one(0.5), one(0.25)], one(2)
    out = cr.forward(tmp, covs, colors, alphas, bg, True)
    assert out.reshape(-1).tolist() == [3.0, 0.0]
    gcol, galpha, gbg = cr.grad(tmp, covs, colors, alphas, one(1), bg, False)
    # S = 2; layer 2: d = 7, S = 0.25 * 7 + 0.75 * 2 = 3.25; layer 1: d = 5, S = 0.5 * 5 + 0.5 * 3.25 = 4.125; layer 0: 1 * (3 - 4.125)
    assert val(galpha[0]) == 3.0 - 4.125 and val(galpha[1]) == 0.0 and val(galpha[2]) == 0.0
    assert [val(g) for g in gcol] == [1.0, 0.0, 0.0] and val(gbg) == 0.0
    # and it is the derivative: at a_0 = 1 - h the pixel is (1 - h) 3 + h 4.125
    lo = cr.forward(tmp, covs, colors, [one(0.5), alphas[1], alphas[2]], bg, False, np.float64)
    assert val(lo) == 0.5 * 3 + 0.5 * 4.125


def test_a_non_covering_layer_full_of_nan_changes_nothing(tmp_path_factory):
    tmp = tmp_path_factory.getbasetemp()
    covs, colors, alphas, bg, rng = case(7, 3, 3, scalar=(2,))
    gout = rng.uniform(-1, 1, (2, 4, 5, 7)).astype(np.float32)
    want_out = cr.forward(tmp, covs, colors, alphas, bg, True)
    want = cr.grad(tmp, covs, colors, alphas, gout, bg, True)
    nan = np.float32(np.nan)
    covs2 = [covs[0], np.zeros_like(covs[0]), covs[1], covs[2]]
    colors2 = [colors[0], np.full_like(colors[0], nan), colors[1], colors[2]]
    alphas2 = [alphas[0], np.full_like(alphas[0], nan), alphas[1], alphas[2]]
    assert np.array_equal(bits(cr.forward(tmp, covs2, colors2, alphas2, bg, True)), bits(want_out))
    got = cr.grad(tmp, covs2, colors2, alphas2, gout, bg, True)
    for k2, k in ((0, 0), (2, 1), (3, 2)):
        assert np.array_equal(bits(got[0][k2]), bits(want[0][k])) and np.array_equal(bits(got[1][k2]), bits(want[1][k]))
    assert not bits(got[0][1]).any() and not bits(got[1][1]).any() and np.array_equal(bits(got[2]), bits(want[2]))
    # NaN in the words a covering layer does not cover: the same
    colors3 = [np.where(c[:, None], col, nan).astype(np.float32) for c, col in zip(covs, colors)]
    alphas3 = [a if np.isscalar(a) else np.where(c[:, None], a, nan).astype(np.float32) for c, a in zip(covs, alphas)]
    assert np.array_equal(bits(cr.forward(tmp, covs, colors3, alphas3, bg, True)), bits(want_out))
    got = cr.grad(tmp, covs, colors3, alphas3, gout, bg, True)
    for k in range(3):
        assert np.array_equal(bits(got[0][k]), bits(want[0][k])) and np.array_equal(bits(got[1][k]), bits(want[1][k]))


def measured_errors(tmp, n_layers):
    """the binary32 gradients against the binary64 ones on random inputs in [0, 1], every layer covering: the largest error of each
    kind of plane, relative to that plane's largest magnitude"""
    worst = {"gcolor": 0.0, "galpha": 0.0, "gbg": 0.0}
    for seed in range(4):
        covs, colors, alphas, bg, rng = case(100 + seed, n_layers, 3, shape=(1, 32, 32), cover=1.1)
        gout = rng.uniform(0, 1, (1, 4, 32, 32)).astype(np.float32)
        g32 = cr.grad(tmp, covs, colors, alphas, gout, bg, True)
        g64 = cr.grad(tmp, covs, [c.astype(np.float64) for c in colors], [a.astype(np.float64) for a in alphas], gout.astype(np.float64),
                      bg.astype(np.float64), True, np.float64)
        for k in range(n_layers):
            for name, i in (("gcolor", 0), ("galpha", 1)):
                worst[name] = max(worst[name], float(np.abs(g32[i][k] - g64[i][k]).max() / np.abs(g64[i][k]).max()))
        worst["gbg"] = max(worst["gbg"], float(np.abs(g32[2] - g64[2]).max() / np.abs(g64[2]).max()))
    return worst


@pytest.mark.parametrize("n_layers", [3, 8])
def test_measured_binary32_error_of_the_gradients(tmp_path_factory, n_layers):
    """no bound is derived: the error is measured here, and held to 8 x the values measured when this was written (compositeref.GRAD_ERR,
    DESIGN.md has the table)"""
    worst = measured_errors(tmp_path_factory.getbasetemp(), n_layers)
    print(n_layers, worst)
    for name, e in worst.items():
        assert 0.0 < e <= 8.0 * cr.GRAD_ERR[n_layers][name], (name, e)
