"""-m gpu: k_composite and k_composite_grad beyond tile_grid's cap, on tests/walkkit.py's `many` (6,144 frames of four tiles) and
`large` (seven frames of 2,401) sets: a workgroup's second trip round the walk.  Three layers made with peel on those sets, an alpha
plane, a scalar and a plane again, the background and the transmittance plane; forward and every gradient plane against
tests/compositeref.py on every frame (walkkit.same), no sentinel left, and a second launch gives the same words."""
import numpy as np
import pytest
import torch

import compositeref as cr
import walkkit
from srz import visibility as V
from support import SENTINEL, ctx, filled, stream, words  # noqa: F401
from walkkit import F, SHAPES, dev, same

pytestmark = pytest.mark.gpu

N_LAYERS = 3
OPACITY = 0.375  # layer 1's scalar alpha


@pytest.fixture(scope="module")
def worlds(ctx):
    yield from walkkit.make_worlds(ctx)


def make_inputs(w):
    """the three layers (layer 1 is the world's own visibility buffer), their coverage, colours and alphas with NaN where the layer
    does not cover, bg and gout — host arrays and their copies on the device"""
    lay = [w.vis]
    while len(lay) < N_LAYERS:
        lay.append(V.peel(w.fs, lay[-1], stream=stream()))
    torch.cuda.synchronize()
    n_tris = np.uint32(w.n_tris)[:, None, None]
    cov = [((words(t)[:, 1] & np.uint32(0x7fffffff)) - np.uint32(1)) < n_tris for t in lay]
    assert np.array_equal(cov[0], w.own) and cov[1].any() and not (cov[1] & ~cov[0]).any()
    assert cov[1][:w.n // 2].any() and cov[1][w.n // 2:].any(), w.name  # the second layer owns pixels on both trips of the walk
    C, shape = w.C, w.shape(w.C)
    rng = w.rng(90)
    nan = np.float32(np.nan)
    cols = [np.where(cv[:, None], rng.uniform(0, 1, shape).astype(np.float32), nan) for cv in cov]
    alphas = [np.where(cov[0][:, None], rng.uniform(0, 1, w.shape(1)).astype(np.float32), nan), OPACITY,
              np.where(cov[2][:, None], rng.uniform(0, 1, w.shape(1)).astype(np.float32), nan)]
    bg = rng.uniform(0, 1, shape).astype(np.float32)
    gout = rng.normal(0, 1, w.shape(C + 1)).astype(np.float32)
    on = dict(cols=[dev(c) for c in cols], alphas=[a if np.isscalar(a) else dev(a) for a in alphas], bg=dev(bg), gout=dev(gout))
    tup = [(lay[k].data_ptr(), on["cols"][k].data_ptr(), None if np.isscalar(alphas[k]) else on["alphas"][k].data_ptr(),
            alphas[k] if np.isscalar(alphas[k]) else 0.0) for k in range(N_LAYERS)]
    return lay, cov, cols, alphas, bg, gout, on, tup


def inputs_of(w):
    return w.memo("composite", make_inputs)


def forward(w):
    *_, on, tup = inputs_of(w)
    out = filled(w.shape(w.C + 1))
    w.fs.composite(tup, w.C, on["bg"].data_ptr(), True, out.data_ptr(), out.numel() * 4, F, stream())
    torch.cuda.synchronize()
    return words(out)


def backward(w):
    *_, on, tup = inputs_of(w)
    gc, ga, gb = [filled(w.shape(w.C)) for _ in tup], [filled(w.shape(1)) for _ in tup], filled(w.shape(w.C))
    w.fs.composite_grad(tup, w.C, on["bg"].data_ptr(), True, on["gout"].data_ptr(), [t.data_ptr() for t in gc], [t.data_ptr() for t in ga],
                        gb.data_ptr(), F, stream())
    torch.cuda.synchronize()
    return [words(t) for t in gc], [words(t) for t in ga], words(gb)


@pytest.mark.parametrize("shape", SHAPES)
def test_composite_forward_beyond_the_cap(worlds, tmp_path, shape):
    w = worlds(shape)
    _, cov, cols, alphas, bg, *_ = inputs_of(w)
    got = forward(w)
    assert not (got == SENTINEL).any()
    want = cr.forward(tmp_path, cov, cols, alphas, bg, True)
    same(got, want, f"composite, {shape}")  # (every frame's words at once)
    assert np.array_equal(forward(w), got), "a second launch differs"


@pytest.mark.parametrize("shape", SHAPES)
def test_composite_grad_beyond_the_cap(worlds, tmp_path, shape):
    w = worlds(shape)
    _, cov, cols, alphas, bg, gout, *_ = inputs_of(w)
    gc, ga, gb = backward(w)
    rc, ra, rb = cr.grad(tmp_path, cov, cols, alphas, gout, bg, True)
    for name, got, want in [(f"gcolor{k}", gc[k], rc[k]) for k in range(N_LAYERS)] + [(f"galpha{k}", ga[k], ra[k]) for k in range(N_LAYERS)] + \
            [("gbg", gb, rb)]:
        assert not (got == SENTINEL).any(), name
        same(got, want, f"composite_grad {name}, {shape}")  # (every frame's words at once)
    again = backward(w)
    for p, q in zip(gc + ga + [gb], again[0] + again[1] + [again[2]]):
        assert np.array_equal(p, q), "a second launch differs"
