"""-m gpu: k_tex_set and k_tex_set_grad on every shard layout of tests/shardkit.py (hold_pass, check_rank_sum), the rank without a
band included: a rank's owned rows are the whole frame's words, its padding keeps what it held, and the ranks' parts of the texel
gradient add up to the whole frame's within the whole frame's bound.  The frames have one batch: the map sends batch 0 to slot 1 of
two.  Slot 0 is a decoy of another size whose texels are NaN and whose d_gtex must stay as it was.  Expected values:
tests/texsetref.py's composition of tests/texref.py on the whole frame, as tests/test_gpu_pass_shards.py has them for texture."""
import numpy as np
import pytest
import torch

import shardkit
import texref
import texsetref
from shardkit import GEOMETRIES, hold_pass, owner_pass
from srz import abi
from support import SENTINEL, ctx, stream, words  # noqa: F401
from walkkit import dev

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
C = 5  # a full register chunk of channels and a tail
TEX = 8
DECOY_W, DECOY_H = 3, 5
UV_SCALE = 12.0  # the frame repeats the texture a dozen times: every band reaches every texel
BATCH_SLOT = (1,)
BOTH = (False, True)


@pytest.fixture(scope="module")
def geos(ctx):
    yield from shardkit.make_geos(ctx)


def pre(g, k):
    return np.full((k, g.H, g.W), SENTINEL, np.uint32)


def uv_of(g):
    """[n, 2, H, W]: the GPU's own interpolate of the frames' uv, scaled; NaN at nobody's pixels"""
    def make(g):
        a = np.zeros((g.n, g.T, 3, 2), np.float32)
        for i, f in enumerate(g.frames):
            a[i, :f.n_tris] = texref.frame_uv(f) * np.float32(UV_SCALE)
        a_dev, out = dev(a), torch.zeros(g.fs.interpolate_shape(2), dtype=torch.float32, device="cuda")
        g.fs.interpolate(g.vis.data_ptr(), a_dev.data_ptr(), 2, g.n, g.T, out.data_ptr(), g.fs.interpolate_bytes(2), F, stream())
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        o[np.broadcast_to(~g.own[:, None], o.shape)] = np.nan
        return o
    return g.memo("uv", make)


def texs_of(g):
    """([the decoy, the texture] as arrays, their copies on the device, the map on the device)"""
    def make(g):
        texs = [np.full((DECOY_H, DECOY_W, C), np.nan, np.float32), texref.make_tex(3, TEX, TEX, C)]
        return texs, [dev(t) for t in texs], torch.tensor(BATCH_SLOT, dtype=torch.uint8, device="cuda")
    return g.memo("texs", make)


def slots(g, mode, gtex=(None, None)):
    _, (d, t), _ = texs_of(g)
    return [(d.data_ptr(), gtex[0], DECOY_W, DECOY_H, 1, abi.TEX_WRAP), (t.data_ptr(), gtex[1], TEX, TEX, 1, mode)]


def run_texture_set(tmp, g, S, fused, mode=texref.CLAMP):
    uv, m, out = S.dev(uv_of(g)), texs_of(g)[2], S.out(C)
    S.fs.texture_set(S.vis_in.data_ptr(), uv.data_ptr(), slots(g, mode), m.data_ptr(), len(BATCH_SLOT), C, out.data_ptr(), S.fs.interpolate_bytes(C),
                     F if fused else 0, stream())
    torch.cuda.synchronize()
    return {"out": words(out)}, {}


def ref_texture_set(tmp, g, v, fused, mode=texref.CLAMP):
    uv, texs = uv_of(g), texs_of(g)[0]
    out = [texsetref.forward(tmp, g.frames[i], texs, [texref.WRAP, mode], BATCH_SLOT, v[i, 1], uv[i], fused, pre(g, C)) for i in range(g.n)]
    return {"out": np.stack(out)}, {}


def gout_of(g):
    return g.memo("gout", lambda g: g.planes(2, C, 2.0, nan=~g.own))


def run_texture_set_grad(tmp, g, S, fused, mode=texref.WRAP):  # (CLAMP would add every uv beyond 1 into one texel)
    uv, (_, (d, t), m), go = S.dev(uv_of(g)), texs_of(g), S.dev(gout_of(g))
    g0, g1, gu = S.acc(d.shape), S.acc(t.shape), S.out(2)
    S.fs.texture_set_grad(S.vis_in.data_ptr(), uv.data_ptr(), go.data_ptr(), slots(g, mode, (g0.data_ptr(), g1.data_ptr())), m.data_ptr(),
                          len(BATCH_SLOT), C, gu.data_ptr(), F if fused else 0, stream())
    torch.cuda.synchronize()
    return {"guv": words(gu)}, {"gtex1": g1.cpu().numpy(), "gtex0": g0.cpu().numpy()}


def ref_texture_set_grad(tmp, g, v, fused, mode=texref.WRAP):
    uv, texs, go = uv_of(g), texs_of(g)[0], gout_of(g)
    accs = [texref.Grad(t.shape) for t in texs]
    gu = [texsetref.grad(tmp, g.frames[i], texs, [texref.WRAP, mode], BATCH_SLOT, v[i, 1], uv[i], go[i], accs, True, fused, pre(g, 2))
          for i in range(g.n)]
    assert accs[0].count.sum() == 0  # the decoy: nobody maps to it
    return {"guv": np.stack(gu)}, {f"gtex{s}": (a.gtex, a.gabs, a.count[:, :, None], 0) for s, a in enumerate(accs)}


PASSES = {"texture_set": (run_texture_set, ref_texture_set), "texture_set_grad": (run_texture_set_grad, ref_texture_set_grad)}


@pytest.mark.parametrize("geo", list(GEOMETRIES))
@pytest.mark.parametrize("name", list(PASSES))
def test_every_shard_gives_the_whole_frames_words(geos, tmp_path, name, geo):
    run, ref = PASSES[name]
    hold_pass(tmp_path, geos(geo), name, run, owner_pass(ref), BOTH)
