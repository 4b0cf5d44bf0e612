"""-m gpu: k_tex_set and k_tex_set_grad beyond the tile-grid cap, on tests/walkkit.py's two sets (many, large), where workgroups go
round the walk's loop a second time with the gradient's LDS table from the tile before.  The sets' frames have one batch: the map
sends batch 0 to slot 1 of two.  Slot 0 is a decoy of another size whose texels are NaN and whose d_gtex must stay zero.  The
expected values are tests/texsetref.py's (the composition of tests/texref.py) on the GPU's own buffers, with the bounds of
tests/test_gpu_pass_walk.py: forward and guv bit for bit, gtex within gamma_n * sum |w g|."""
import numpy as np
import pytest
import torch

import texref
import texsetref
import walkkit
from srz import abi
from support import ctx, filled, stream, words  # noqa: F401
from walkkit import F, SHAPES, TEX_H, TEX_W, check_nobody, check_sum, dev, pre, same

pytestmark = pytest.mark.gpu

DECOY_W, DECOY_H = 5, 3
BATCH_SLOT = (1,)


@pytest.fixture(scope="module")
def worlds(ctx):
    yield from walkkit.make_worlds(ctx)


def slots_of(w, mode, gtex=(None, None)):
    """(the slot tuples for FrameSet.texture_set, the two textures as arrays, the map on the device)"""
    t, t_dev, _, _ = w.tex
    decoy = w.memo("texset decoy", lambda w: (lambda d: (d, dev(d)))(np.full((DECOY_H, DECOY_W, w.C), np.nan, np.float32)))
    m = w.memo("texset map", lambda w: torch.tensor(BATCH_SLOT, dtype=torch.uint8, device="cuda"))
    tup = [(decoy[1].data_ptr(), gtex[0], DECOY_W, DECOY_H, 1, abi.TEX_WRAP), (t_dev.data_ptr(), gtex[1], TEX_W, TEX_H, 1, mode)]
    return tup, [decoy[0], t], m


def run_texture_set(tmp, w, fused, mode=texref.CLAMP):
    fs, C = w.fs, w.C
    uv, _, uvw, _ = w.uv
    tup, texs, m = slots_of(w, mode)
    out = filled(w.shape(C))
    fs.texture_set(w.vis.data_ptr(), uv.data_ptr(), tup, m.data_ptr(), len(BATCH_SLOT), C, out.data_ptr(), fs.interpolate_bytes(C),
                   F if fused else 0, stream())
    torch.cuda.synchronize()
    got = words(out)
    want = [texsetref.forward(tmp, w.frames[i], texs, [texref.WRAP, mode], BATCH_SLOT, w.v[i, 1], uvw[i], fused, pre(w, C)) for i in range(w.n)]
    same(got, np.stack(want), "texture_set")
    check_nobody(w, got, fused, "texture_set")
    assert not np.isnan(got.view(np.float32)[np.broadcast_to(w.own[:, None], got.shape)]).any()  # nothing came from the decoy


def run_texture_set_grad(tmp, w, fused, mode=texref.WRAP):  # (CLAMP would add every uv beyond 1 into one texel)
    fs, C = w.fs, w.C
    (uv, _, uvw, _), (gout, g) = w.uv, w.gout
    t_dev = w.tex[1]
    g0, g1, gu = torch.zeros((DECOY_H, DECOY_W, C), dtype=torch.float32, device="cuda"), torch.zeros_like(t_dev), filled(w.shape(2))
    tup, texs, m = slots_of(w, mode, (g0.data_ptr(), g1.data_ptr()))
    fs.texture_set_grad(w.vis.data_ptr(), uv.data_ptr(), g.data_ptr(), tup, m.data_ptr(), len(BATCH_SLOT), C, gu.data_ptr(), F if fused else 0,
                        stream())
    torch.cuda.synchronize()
    accs = [texref.Grad(t.shape) for t in texs]
    want = [texsetref.grad(tmp, w.frames[i], texs, [texref.WRAP, mode], BATCH_SLOT, w.v[i, 1], uvw[i], gout[i], accs, True, fused, pre(w, 2))
            for i in range(w.n)]
    got = words(gu)
    same(got, np.stack(want), "texture_set guv")
    check_nobody(w, got, fused, "texture_set guv")
    check_sum(g1.cpu().numpy(), accs[1].gtex, accs[1].gabs, accs[1].count[:, :, None], "texture_set gtex")
    assert accs[0].count.sum() == 0 and (g0.cpu().numpy().view(np.uint32) == 0).all()  # the decoy's gradient: not one add, not a -0


PASSES = {"texture_set": run_texture_set, "texture_set_grad": run_texture_set_grad}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", list(PASSES))
def test_more_tiles_than_workgroups(worlds, tmp_path, name, shape):
    """(many: with and without the fused clear; large: without it, the stricter of the two — nobody's words must survive)"""
    w = worlds(shape)
    for fused in ((False, True) if shape == "many" else (False,)):
        PASSES[name](tmp_path, w, fused)
