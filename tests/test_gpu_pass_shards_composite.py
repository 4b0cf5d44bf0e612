"""-m gpu: srz_frameset_composite and _composite_grad on band shards whose local bands are not the frame's (tests/shardkit.py's two
geometries and three layouts, the rank without a band among them).  shardkit.hold_pass: the unsharded call against
tests/compositeref.py on the whole frame, word for word; then every rank on its rows of the whole-frame inputs — three peeled
layers, the colours, an alpha plane and a scalar, the background, the gradient —, NaN in every float plane and the sentinel in every
id plane outside its bands, and the sentinel in every output there: the owned rows are the whole frame's words, the padding is
untouched, with SRZ_FUSED_CLEAR in `flags` and without (it changes nothing in this pass)."""
import numpy as np
import pytest
import torch

import compositeref as cr
import shardkit
from shardkit import GEOMETRIES, hold_pass
from srz import abi
from srz import visibility as V
from support import SENTINEL, ctx, stream, words  # noqa: F401
from walkkit import dev

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
N_LAYERS, C = 3, 3
OPACITY = 0.625  # layer 1's scalar alpha


@pytest.fixture(scope="module")
def geos(ctx):
    yield from shardkit.make_geos(ctx)


def done(**outs):
    torch.cuda.synchronize()
    return {k: words(t) for k, t in outs.items()}


def inputs_of(g):
    """the whole frame's three layers (words), their coverage, colours and alphas with NaN where the layer does not cover, bg, gout"""
    def make(g):
        lay = V.layers(g.fs, N_LAYERS)
        torch.cuda.synchronize()
        lw = [words(t) for t in lay]
        cov = [((w[:, 1] & np.uint32(0x7fffffff)) - np.uint32(1)) < np.uint32(g.n_tris)[:, None, None] for w in lw]  # (Geo.own's test)
        for k in range(N_LAYERS):  # every layer owns pixels in every frame, and all three share some
            assert cov[k].reshape(g.n, -1).any(1).all(), (g.name, k)
        assert (cov[0] & cov[1] & cov[2]).any() and (~cov[0] & ~cov[1] & ~cov[2]).any(), g.name
        cols = [g.planes(60 + k, C, nan=~cov[k]) for k in range(N_LAYERS)]
        alphas = [np.abs(g.planes(70, 1, nan=~cov[0])), OPACITY, g.planes(72, 1, scale=0.5, nan=~cov[2])]
        return lw, cov, cols, alphas, g.planes(80, C), g.planes(81, C + 1)
    return g.memo("composite", make)


def shard_layers(g, S):
    """the rank's rows of the whole frame's layers, by hand: NaN in the padding's float planes, the sentinel in its id plane"""
    if not hasattr(S, "comp_layers"):
        S.comp_layers = []
        for w in inputs_of(g)[0]:
            hand = S.local(w.view(np.float32))
            hand[:, 1][:, S.is_pad] = np.uint32(SENTINEL).view(np.float32)
            S.comp_layers.append(dev(hand))
    return S.comp_layers


def layer_args(g, S):
    _, _, cols, alphas, bg, gout = inputs_of(g)
    lay = shard_layers(g, S)
    cd = [S.dev(c) for c in cols]
    ad = [None if np.isscalar(a) else S.dev(a) for a in alphas]
    tup = [(lay[k].data_ptr(), cd[k].data_ptr(), None if ad[k] is None else ad[k].data_ptr(), alphas[k] if ad[k] is None else 0.0)
           for k in range(N_LAYERS)]
    return tup, (lay, cd, ad), S.dev(bg), S.dev(gout)


def run_composite(tmp, g, S, fused):
    tup, keep, bg, _ = layer_args(g, S)
    out = S.out(C + 1)
    S.fs.composite(tup, C, bg.data_ptr(), True, out.data_ptr(), out.numel() * 4, F if fused else 0, stream())
    return done(out=out), {}


def ref_composite(tmp, g, rows, fused):
    _, cov, cols, alphas, bg, _ = inputs_of(g)
    return {"out": cr.forward(tmp, cov, cols, alphas, bg, True)}, {}


def run_composite_grad(tmp, g, S, fused):
    tup, keep, bg, gout = layer_args(g, S)
    gc, ga, gb = [S.out(C) for _ in range(N_LAYERS)], [S.out(1) for _ in range(N_LAYERS)], S.out(C)
    S.fs.composite_grad(tup, C, bg.data_ptr(), True, gout.data_ptr(), [t.data_ptr() for t in gc], [t.data_ptr() for t in ga], gb.data_ptr(),
                        F if fused else 0, stream())
    return done(gbg=gb, **{f"gcolor{k}": gc[k] for k in range(N_LAYERS)}, **{f"galpha{k}": ga[k] for k in range(N_LAYERS)}), {}


def ref_composite_grad(tmp, g, rows, fused):
    _, cov, cols, alphas, bg, gout = inputs_of(g)
    gc, ga, gb = cr.grad(tmp, cov, cols, alphas, gout, bg, True)
    return dict(gbg=gb, **{f"gcolor{k}": gc[k] for k in range(N_LAYERS)}, **{f"galpha{k}": ga[k] for k in range(N_LAYERS)}), {}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_composite_on_every_shard(geos, tmp_path_factory, name):
    hold_pass(tmp_path_factory.getbasetemp(), geos(name), "composite", run_composite, ref_composite, (True, False))


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_composite_grad_on_every_shard(geos, tmp_path_factory, name):
    hold_pass(tmp_path_factory.getbasetemp(), geos(name), "composite_grad", run_composite_grad, ref_composite_grad, (True, False))
