"""-m gpu: srz.visibility.texture_set as a torch.autograd.Function, against the torch composition of the existing passes on the
device that it replaces: sum_s where(mask_s, texture(fs, vis, tex_s, uv, wrap_s), 0), mask_s from decode and batch_of.  Forward:
torch.equal.  uv.grad: equal as values.  Each tex.grad: within TWICE tests/texsetref.py's bound for that slot — both sides are atomic
sums that each lie within the bound of the exact sum.  Only textures that require grad get one; the chain
texture_set(interpolate(...)) reaches the uv attribute."""
import numpy as np
import pytest
import torch

import texref
import texsetref
from srz import visibility
from support import SENTINEL, ctx, visibility as render_visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

BATCH_SLOT = texsetref.HOLES_MAP  # (1, 0, None, 2) over five batches: a batch without a slot, a batch beyond the map
WRAPS = (False, True, True)


def dev(a, grad=False):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda().requires_grad_(grad)


@pytest.fixture(scope="module")
def scene(ctx):
    frames = [texsetref.holes_frame(), texsetref.holes_frame()]
    fs = ctx.frameset(frames)
    vis = render_visibility(fs)
    T = frames[0].n_tris
    attr = np.stack([texref.frame_uv(f) for f in frames])
    texs = [texref.make_tex(1, 5, 7, 3), texref.make_tex(2, 33, 1, 3, frames=2), texref.make_tex(3, 64, 64, 3)]
    tri = visibility.decode(vis).tri
    batch = torch.stack([visibility.batch_of(f, tri[i]) for i, f in enumerate(frames)])
    yield fs, vis, frames, T, attr, texs, batch
    fs.close()


def composed(fs, vis, texs, uv, batch):
    """what a caller had to write before: one full-frame texture() per material, masks from an int64 round trip, torch.where"""
    out = None
    for b, s in enumerate(BATCH_SLOT):
        if s is None:
            continue
        term = torch.where((batch == b)[:, None], visibility.texture(fs, vis, texs[s], uv, WRAPS[s]), torch.zeros((), device="cuda"))
        out = term if out is None else out + term
    return out


def test_forward_and_gradients_against_the_composition_of_existing_passes(scene, tmp_path):
    fs, vis, frames, T, attr, texs, batch = scene
    uv0 = visibility.interpolate(fs, vis, dev(attr)).detach()
    gout = torch.as_tensor(np.random.default_rng(3).normal(0, 2, tuple(fs.interpolate_shape(3))).astype(np.float32)).cuda()
    res = []
    for fn in ("set", "composed"):
        t = [dev(x, True) for x in texs]
        uv = uv0.clone().requires_grad_(True)
        out = visibility.texture_set(fs, vis, t, uv, BATCH_SLOT, WRAPS) if fn == "set" else composed(fs, vis, t, uv, batch)
        out.backward(gout)
        res.append((out.detach(), uv.grad, [x.grad for x in t]))
    (o1, gu1, gt1), (o2, gu2, gt2) = res
    assert torch.equal(o1, o2)
    assert bool((gu1 == gu2).all()) and bool((gu1 != 0).any())  # (equal as values: a sum with zeros may turn a -0 into +0)
    v, uvw = words(vis), uv0.cpu().numpy()
    accs, _ = texsetref.grad_set(tmp_path, frames, v, uvw, gout.cpu().numpy(), texs, [int(w) for w in WRAPS], BATCH_SLOT, True, SENTINEL)
    for s in range(3):
        bound = np.stack([a.bound() for a in accs.acc[s]]).reshape(texs[s].shape)
        ref = np.stack([a.gtex for a in accs.acc[s]]).reshape(texs[s].shape)
        a, b = gt1[s].cpu().numpy().astype(np.float64), gt2[s].cpu().numpy().astype(np.float64)
        assert (np.abs(a - ref) <= bound).all() and (np.abs(a - b) <= 2 * bound).all() and (a != 0).any(), s
        print(f"slot {s}: max |set - composed| / (2 bound) {np.max(np.abs(a - b)[bound > 0] / (2 * bound[bound > 0])):.3f}")


def test_only_the_textures_that_require_grad_get_one(scene):
    fs, vis, frames, T, attr, texs, batch = scene
    uv = visibility.interpolate(fs, vis, dev(attr)).detach()
    t = [dev(texs[0], True), dev(texs[1]), dev(texs[2], True)]
    out = visibility.texture_set(fs, vis, t, uv, BATCH_SLOT, WRAPS)
    out.sum().backward()
    assert t[0].grad is not None and t[1].grad is None and t[2].grad is not None and uv.grad is None
    assert bool((t[0].grad != 0).any()) and bool((t[2].grad != 0).any())
    # uv alone
    uv2 = uv.clone().requires_grad_(True)
    visibility.texture_set(fs, vis, [dev(x) for x in texs], uv2, BATCH_SLOT, WRAPS).sum().backward()
    assert uv2.grad is not None and bool((uv2.grad != 0).any())
    # nothing requires grad: no graph
    assert not visibility.texture_set(fs, vis, [dev(x) for x in texs], uv, BATCH_SLOT, WRAPS).requires_grad
    # the map as a tensor gives the same words
    m = torch.tensor([texsetref.NONE if s is None else s for s in BATCH_SLOT], dtype=torch.uint8, device="cuda")
    assert torch.equal(visibility.texture_set(fs, vis, [dev(x) for x in texs], uv, m, WRAPS), out.detach())


def test_the_chain_reaches_the_uv_attribute(scene):
    fs, vis, frames, T, attr, texs, batch = scene
    res = []
    for fn in ("set", "composed"):
        a = dev(attr, True)
        uv = visibility.interpolate(fs, vis, a)
        t = [dev(x) for x in texs]
        out = visibility.texture_set(fs, vis, t, uv, BATCH_SLOT, WRAPS) if fn == "set" else composed(fs, vis, t, uv, batch)
        (out * out).sum().backward()
        res.append(a.grad)
    assert res[0] is not None and bool((res[0] != 0).any()) and bool(torch.isfinite(res[0]).all())
    # interpolate's backward is a float-atomic sum on both sides: equal to rounding, not to the bit
    assert torch.allclose(res[0], res[1], rtol=1e-4, atol=1e-3 * float(res[1].abs().max()))
