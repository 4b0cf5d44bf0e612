"""-m gpu: srz.visibility's cube_prefilter, cube_irradiance and cube_prefilter_pyramid as torch.autograd Functions: the gradient
autograd leaves is the plain cube_prefilter_grad's, the pyramid and its backward are the composition of the references (the box
pyramid, the GGX prefilter per level; the prefilter's transpose per level, the fold) bit for bit, and the chain into
texture_cube_mip carries a gradient back to the environment cube."""
import numpy as np
import pytest
import torch

import cubemipref
import mipref
import prefilterref as P
from srz import abi
from srz import visibility as V
from support import ccw, ctx, frame, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def same(got, ref, what):
    got, ref = words(got.detach()), np.ascontiguousarray(ref, np.float32).view(np.uint32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} of {ref.size} words differ"


@pytest.mark.parametrize("shape,n_out,kind,r,cmin", [((6, 5, 5, 3), 8, abi.PREFILTER_GGX, 0.3, 0.0), ((2, 6, 8, 8, 5), 3, abi.PREFILTER_COSINE, 1.0, 0.5)])
def test_autograd_leaves_the_plain_backward(ctx, tmp_path, shape, n_out, kind, r, cmin):  # noqa: F811
    rng = np.random.default_rng(21)
    cube_n = rng.uniform(0, 1, shape).astype(np.float32)
    w_n = rng.uniform(-1, 1, shape[:-3] + (n_out, n_out, shape[-1])).astype(np.float32)
    cube = dev(cube_n).requires_grad_(True)
    out = V.cube_prefilter(ctx, cube, n_out, kind, r, cmin)
    ref_out, ref_den, _ = P.forward(tmp_path, cube_n, n_out, kind, r, cmin)
    same(out, ref_out, "forward")
    (out * dev(w_n)).sum().backward()
    torch.cuda.synchronize()
    plain = V.cube_prefilter_grad(ctx, dev(w_n), dev(ref_den), shape[-2], kind, r, cmin)
    assert torch.equal(cube.grad.view(torch.int32), plain.view(torch.int32))
    same(cube.grad, P.grad(tmp_path, w_n, ref_den, shape[-2], kind, r, cmin), "cube.grad")
    assert not V.cube_prefilter(ctx, cube.detach(), n_out, kind, r, cmin).requires_grad


def test_irradiance_is_the_cosine_call(ctx, tmp_path):  # noqa: F811
    cube_n = np.random.default_rng(22).uniform(0, 1, (6, 8, 8, 3)).astype(np.float32)
    same(V.cube_irradiance(ctx, dev(cube_n), 4), P.forward(tmp_path, cube_n, 4, P.COSINE)[0], "irradiance")


def test_the_pyramid_and_its_backward_are_the_references_composed(ctx, tmp_path):  # noqa: F811
    N, C, rough, cmin = 8, 3, (0.25, 0.75), 0.0  # three levels: 8, 4, 2
    L = len(rough) + 1
    rng = np.random.default_rng(23)
    cube_n = rng.uniform(0, 1, (6, N, N, C)).astype(np.float32)
    box = cubemipref.build(cube_n, L)
    ref = [P.forward(tmp_path, box[l], N >> l, P.GGX, rough[l - 1], cmin) for l in range(1, L)]
    cube = dev(cube_n).requires_grad_(True)
    mip = V.cube_prefilter_pyramid(ctx, cube, rough, cmin)
    same(mip, cubemipref.flat([r[0] for r in ref]), "mip")
    w_n = rng.uniform(-1, 1, mip.shape).astype(np.float32)
    (mip * dev(w_n)).sum().backward()
    torch.cuda.synchronize()
    gbox, off = [], 0
    for l in range(1, L):
        k = 6 * (N >> l) ** 2 * C
        gbox.append(P.grad(tmp_path, w_n[off:off + k].reshape(6, N >> l, N >> l, C), ref[l - 1][1], N >> l, P.GGX, rough[l - 1], cmin))
        off += k
    want = mipref.fold(tmp_path, cubemipref.flat(gbox), (6, N, N, C), L, np.zeros((6, N, N, C), np.float32))
    same(cube.grad, want, "cube.grad")
    assert (want != 0).any()


def test_the_chain_into_texture_cube_mip_reaches_the_environment(ctx):  # noqa: F811
    """README's chain on a 64 x 64 one-triangle set: env -> cube_prefilter_pyramid -> texture_cube_mip(mip=) -> a loss, and
    env -> cube_irradiance -> texture_cube"""
    fs = ctx.frameset([frame(ccw((4, 4), (60, 8), (20, 58)), 64, 64)])
    vis = visibility(fs)
    rng = np.random.default_rng(24)
    env = dev(rng.uniform(0, 1, (6, 8, 8, 3))).requires_grad_(True)
    dirs = dev(rng.normal(size=fs.interpolate_shape(3)))
    rough = dev(rng.uniform(0, 1, fs.interpolate_shape(1)))
    mip = V.cube_prefilter_pyramid(ctx, env, [0.25, 0.5, 1.0])
    spec = V.texture_cube_mip(fs, vis, env, dirs, rough * 3, mip=mip)
    diff = V.texture_cube(fs, vis, V.cube_irradiance(ctx, env, 4), dirs)
    (spec + diff).sum().backward()
    torch.cuda.synchronize()
    g = env.grad.cpu().numpy()
    assert np.isfinite(g).all() and (g != 0).any() and float(spec.detach().abs().sum()) > 0
    fs.close()
