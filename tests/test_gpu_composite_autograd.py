"""-m gpu: srz.visibility.composite_layers under autograd — layers(fs, 3) with interpolated colours, a learnable alpha plane, a
learnable scalar opacity and background(...) behind everything: the Function's gradients are composite_grad's words, needs_input_grad
selects what the one backward call asks for, the chain backpropagates to the attributes and the environment, and the gradients agree
with autograd through the torch composite within the binary32 error tests/test_composite_ref.py measured (compositeref.GRAD_ERR)."""
import numpy as np
import pytest
import torch

import compositeref as cr
from srz import visibility as V
from support import ccw, ctx, frame, soup  # noqa: F401

pytestmark = pytest.mark.gpu

W = H = 64
ZS = np.float32([1, 2, 3, 4])
U = 2.0 ** -24


def dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


@pytest.fixture(scope="module")
def scene(ctx):
    """two frames: a small soup in front of four staggered triangles over the lower right → (fs, the three layers, their coverage as
    bool tensors [n, 1, H, W], the largest triangle count)"""
    frames = []
    for seed in (5, 6):
        back = [ccw((W + 8, H + 8), (-16 - 9 * i - seed, H + 8), (W + 8, -19 - 8 * i), z=10.0 * (i + 1)) for i in range(4)]
        frames.append(frame(np.concatenate([soup(seed, 8, W, H, ZS)] + back), W, H))
    fs = ctx.frameset(frames)
    lay = V.layers(fs, 3)
    cov = [(V.decode(t).tri >= 0)[:, None] for t in lay]
    torch.cuda.synchronize()
    for k in range(3):
        assert bool(cov[k].flatten(1).any(1).all()), k
    assert bool((cov[0] & cov[1] & cov[2]).any()) and bool((~cov[0]).any())
    yield fs, lay, cov, max(f.n_tris for f in frames)
    fs.close()


def make_leaves(fs, T, seed):
    rng = np.random.default_rng(seed)
    attrs = [dev(rng.uniform(0, 1, (fs.n_frames, T, 3, 3))).requires_grad_(True) for _ in range(3)]
    a0 = dev(rng.uniform(0, 1, fs.interpolate_shape(1))).requires_grad_(True)
    s = torch.tensor(0.625, requires_grad=True)  # (a 0-dim tensor on the host: the layer's opacity)
    a2 = dev(rng.uniform(0, 1, fs.interpolate_shape(1)))
    env = dev(rng.uniform(0, 1, (6, 4, 4, 3))).requires_grad_(True)
    rays = dev([[-0.5, -0.5, 1.0, 1.0 / W, 0, 0, 0, 1.0 / H, 0]])
    g = dev(rng.uniform(0, 1, fs.interpolate_shape(4)))
    return attrs, a0, s, a2, env, rays, g


def test_the_function_is_the_plain_call_and_asks_for_what_is_needed(scene, monkeypatch):
    import srz
    fs, lay, cov, T = scene
    calls = []
    real = srz.FrameSet.composite_grad
    monkeypatch.setattr(srz.FrameSet, "composite_grad", lambda self, *a, **k: (calls.append(a), real(self, *a, **k))[1])
    attrs, a0, s, a2, env, rays, g = make_leaves(fs, T, 1)
    cols = [V.interpolate(fs, lay[k], attrs[k]).detach().requires_grad_(True) for k in range(3)]
    bg = V.background(fs, None, env, rays, "all").detach().requires_grad_(True)
    out = V.composite_layers(fs, lay, cols, [a0, s, a2], bg, through=True)
    assert out.shape == tuple(fs.interpolate_shape(4))
    (out * g).sum().backward()
    assert len(calls) == 1
    # (layers, n_ch, bg, through, gout, gcolor pointers, galpha pointers, gbg): every colour, the two learnable alphas, the background
    assert [bool(p) for p in calls[0][5]] == [True] * 3 and [bool(p) for p in calls[0][6]] == [True, True, False] and bool(calls[0][7])
    gcol, galpha, gbg = V.composite_grad(fs, lay, cols, [a0.detach(), 0.625, a2], g, bg.detach(), True)
    for k in range(3):
        assert torch.equal(cols[k].grad, gcol[k])
    assert torch.equal(a0.grad, galpha[0]) and torch.equal(bg.grad, gbg) and a2.grad is None
    assert s.grad.shape == () and s.grad.device.type == "cpu" and float(s.grad) == float(galpha[1].sum())
    # only one input needs a gradient: the call asks for that plane alone; none: no call
    a0.grad = None
    n0 = len(calls)  # (the plain call above went through FrameSet.composite_grad too)
    V.composite_layers(fs, lay, [c.detach() for c in cols], [a0, 0.625, a2], bg.detach()).sum().backward()
    assert len(calls) == n0 + 1 and not any(calls[-1][5]) and [bool(p) for p in calls[-1][6]] == [True, False, False] and not calls[-1][7]
    assert not V.composite_layers(fs, lay, [c.detach() for c in cols], [0.5, 0.625, a2]).requires_grad and len(calls) == n0 + 1
    # nothing but the inputs is kept for the backward: the output is the only new tensor of the forward
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    keep = V.composite_layers(fs, lay, cols, [a0, s, a2], bg, through=True)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - before <= keep.numel() * 4 + 4096


def test_the_chain_agrees_with_autograd_through_the_torch_composite(scene):
    fs, lay, cov, T = scene
    attrs, a0, s, a2, env, rays, g = make_leaves(fs, T, 2)
    # ---- the fused chain
    cols = [V.interpolate(fs, lay[k], attrs[k]) for k in range(3)]
    for c in cols:
        c.retain_grad()
    bg = V.background(fs, None, env, rays, "all")
    bg.retain_grad()
    out = V.composite_layers(fs, lay, cols, [a0, s, a2], bg, through=True)
    (out * g).sum().backward()
    torch.cuda.synchronize()
    for name, t in [("env", env)] + [(f"attr{k}", a) for k, a in enumerate(attrs)]:
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any()), name
    fused = dict(a0=a0.grad.clone(), s=s.grad.clone(), bg=bg.grad.clone(), **{f"col{k}": cols[k].grad.clone() for k in range(3)},
                 **{f"attr{k}": attrs[k].grad.clone() for k in range(3)}, env=env.grad.clone())
    for t in (a0, s, env, *attrs):
        t.grad = None
    # ---- the torch chain: coverage folded into the alphas (interpolate writes zeros where nobody owns the pixel)
    cols_t = [V.interpolate(fs, lay[k], attrs[k]) for k in range(3)]
    for c in cols_t:
        c.retain_grad()
    bg_t = V.background(fs, None, env, rays, "all")
    bg_t.retain_grad()
    sd = s.cuda()
    eff = [a0 * cov[0], sd * cov[1], a2 * cov[2]]
    T_ = torch.ones_like(eff[0])
    for e in eff:
        T_ = T_ * (1 - e)
    ref = torch.cat([V.composite(cols_t, eff) + T_ * bg_t, T_], dim=1)
    assert torch.equal(ref, out.detach())  # (the forward: float values, +-0 alike)
    (ref * g).sum().backward()
    torch.cuda.synchronize()
    E = cr.GRAD_ERR[3]

    def within(name, got, want, kind):
        err, mag = float((got - want).abs().max()), float(want.abs().max())
        print(f"{name}: max err {err:.3e} of max |value| {mag:.3e}: {err / mag:.3e} relative, bound {8 * E[kind]:.3e}")
        assert mag > 0 and err <= 8 * E[kind] * mag, name
    for k in range(3):
        within(f"gcolor{k}", fused[f"col{k}"], cols_t[k].grad, "gcolor")
    within("galpha0", fused["a0"], a0.grad, "galpha")
    within("gbg", fused["bg"], bg_t.grad, "gbg")
    # the scalar: two binary32 sums over the layer's pixels of planes that differ by at most the plane bound at every pixel
    n = int(cov[1].sum())
    plane = V.composite_grad(fs, lay, [c.detach() for c in cols], [a0.detach(), 0.625, a2], g, bg.detach(), True, False, [False, True, False],
                             False)[1][1]
    mag, total = float(plane.abs().max()), float(plane.abs().double().sum())
    bound = n * 8 * E["galpha"] * mag + 2 * (n * U / (1 - n * U)) * total
    err = abs(float(fused["s"]) - float(s.grad))
    print(f"scalar opacity: {float(fused['s']):.9g} against {float(s.grad):.9g}: err {err:.3e}, bound {bound:.3e} over {n} pixels")
    assert n * U < 1 and err <= bound
    # what lies behind the composite gets the same planes up to that error: the leaves' gradients are close
    for name in ("attr0", "attr1", "attr2", "env"):
        leaf = env if name == "env" else attrs[int(name[-1])]
        assert torch.allclose(fused[name], leaf.grad, rtol=1e-3, atol=1e-3 * float(leaf.grad.abs().max())), name
