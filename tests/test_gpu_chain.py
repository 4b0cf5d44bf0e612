"""-m gpu: the scenes of tests/test_chain_ref.py through the real pipeline and srz.visibility's autograd — render_visibility →
interpolate_geo [→ texture] [+ depth] → antialias → loss → pos.grad — held to tests/chainref.py, the same chain composed from the CPU
references over the oracle's renders, and to frames RENDERED AGAIN with the geometry moved.  One FrameSet holds the base frame and
P + h d, P - h d of up to 32 probes; gout is zero on every frame but the base one, so one backward gives the base frame's pos.grad
and the other frames serve the forward losses only.  The losses are summed in float64 on the host from the downloaded planes."""
import numpy as np
import pytest
import torch

import chainref as cr
from srz import abi
from srz.visibility import antialias, depth, interpolate_geo, texture
from support import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

K_MAX = 32


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def same(got, want, what):
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def chain(fs, positions, attr, tex=None, with_depth=False, silhouette=True, stream=None, pad=1):
    """one visibility render of the set and the autograd chain over it, every pass (and the render) on `stream` (a raw handle; None:
    torch's current stream) → (out [n, planes, rows, W], pos [n, T, 3, 3], the leaf whose .grad a backward fills).  positions:
    [n, T0, 3, 3], padded here with `pad` triangles of zeros; attr [T0, 3, C]; silhouette False: antialias is not given pos, so
    pos.grad is the interior term alone."""
    n, T0 = positions.shape[:2]
    pos = torch.zeros((n, T0 + pad, 3, 3), dtype=torch.float32, device="cuda")
    pos[:, :T0] = dev(positions)
    pos.requires_grad_(True)
    a = torch.zeros((T0 + pad, 3, attr.shape[2]), dtype=torch.float32, device="cuda")
    a[:T0] = dev(attr)
    vis = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, torch.cuda.current_stream().cuda_stream if stream is None else stream)
    planes = interpolate_geo(fs, vis, a, pos, stream=stream)
    if tex is not None:
        planes = texture(fs, vis, dev(tex), planes, stream=stream)
    if with_depth:
        planes = torch.cat([planes, depth(fs, vis, pos, stream=stream)], 1)
    return antialias(fs, vis, planes, pos if silhouette else None, stream=stream), pos


def run_scene(ctx, s, silhouette=True, side=None, first_set_only=False):
    """every probe of scene s (a chainref.evaluate namespace) in sets of K_MAX, on torch's current stream or (side: a
    torch.cuda.Stream, the current one while this runs) with that stream's handle given to the render and every pass and nothing but
    that stream synchronised → (outs: per probe the planes of (hi, lo), base_outs: the base frame's planes of every set, grads: the
    whole pos.grad of every set, as numpy)"""
    outs, base_outs, grads = [], [], []
    for at in range(0, len(s.dirs), K_MAX):
        ks = range(at, min(at + K_MAX, len(s.dirs)))
        positions = np.stack([s.P] + [p for k in ks for p in (s.hi[k], s.lo[k])])
        fs = ctx.frameset([cr.frame_of(p) for p in positions])
        gout = np.zeros((len(positions),) + s.gout.shape, np.float32)
        gout[0] = s.gout
        out, pos = chain(fs, positions, s.attr, s.tex, s.depth, silhouette, None if side is None else side.cuda_stream)
        (out * dev(gout)).sum().backward()
        side.synchronize() if side is not None else torch.cuda.synchronize()
        out, grad = out.detach().cpu().numpy(), pos.grad.cpu().numpy()
        base_outs.append(out[0])
        outs += [(out[1 + 2 * i], out[2 + 2 * i]) for i in range(len(ks))]
        grads.append(grad)
        fs.close()
        if first_set_only:
            break
    return outs, base_outs, grads


def loss64(gout, out):
    return float((gout.astype(np.float64) * out.astype(np.float64)).sum())


@pytest.mark.parametrize("variant", cr.VARIANTS)
def test_chain_against_the_cpu_chain_and_re_rendered_frames(ctx, tmp_path, orc, variant):
    """(a) every frame's planes equal chainref's bit for bit — the composition of the forward passes; (b) the base frame's pos.grad
    lies within bound_interior + bound_silhouette of chainref's float64 sums (each term's own gamma_n * sum |term|; autograd's one
    float32 add of the two terms is covered: each bound counts n roundings for n adds, and the first add, into a zero, is exact), is
    exactly zero for the padded triangle, for every other frame and, without the depth plane, in the z column; (c) on the probes
    chainref classifies as quiet the device's own central difference against <pos.grad, d> stays under the CPU tolerance of
    tests/test_chain_ref.py; (d) neither term can be left out, from the device's numbers: the interior term alone (antialias not given
    pos) misses the differences by more than ten tolerances, and equals zero exactly in the flat-colour scene.  (The shares of the
    sum of |term| need the sums of |term|, which only the reference has: tests/test_chain_ref.py.)"""
    s = cr.evaluate(tmp_path, orc, variant)
    T0 = len(s.P)
    outs, base_outs, grads = run_scene(ctx, s)
    # ---- (a)
    for b in base_outs:
        same(b, s.base.out, f"{variant} base frame")
    for k, ((hi, lo), (ehi, elo)) in enumerate(zip(outs, s.ends)):
        same(hi, ehi.out, f"{variant} probe {s.names[k]} +")
        same(lo, elo.out, f"{variant} probe {s.names[k]} -")
    # ---- (b)
    bound = s.base.interior.bound() + s.base.silhouette.bound()
    for g in grads:
        err = np.abs(g[0, :T0].astype(np.float64) - s.base.total)
        print(f"{variant}: pos.grad max err {err.max():.3e}, max err / bound {(err[bound > 0] / bound[bound > 0]).max():.3f}")
        assert (err <= bound).all(), (np.argwhere(err > bound)[:4].tolist(), float((err - bound).max()))
        assert not g[0, T0:].any() and not g[1:].any()
        if not s.depth:
            assert not g[..., 2].any()
    # ---- (c)
    g = grads[0][0, :T0].astype(np.float64)
    d_l = [loss64(s.gout, hi) - loss64(s.gout, lo) for hi, lo in outs]
    scale = [float((s.base.gabs * np.abs(step)).sum()) for step in s.steps]
    gap = np.array([abs(d - float((g * step).sum())) / sc for d, step, sc in zip(d_l, s.steps, scale)])
    q = s.quiet
    print(f"{variant}: {int(q.sum())} quiet probes of {len(q)}: worst gap on the device {gap[q].max():.3e} (CPU chain {s.gap[q, 0].max():.3e}), "
          f"tolerance {cr.TOL:.3e}")
    assert q.sum() >= 24 and (gap[q] <= cr.TOL).all(), [(s.names[i], float(gap[i])) for i in np.flatnonzero(q & (gap > cr.TOL))[:6]]
    # ---- (d)
    _, _, inner = run_scene(ctx, s, silhouette=False, first_set_only=True)
    gi = inner[0][0, :T0].astype(np.float64)
    ibound = s.base.interior.bound()
    assert (np.abs(gi - s.base.interior.gpos) <= ibound).all()
    no_sil = np.array([abs(d - float((gi * step).sum())) / sc for d, step, sc in zip(d_l, s.steps, scale)])
    no_int = np.array([abs(d - float(((g - gi) * step).sum())) / sc for d, step, sc in zip(d_l, s.steps, scale)])
    print(f"{variant}: silhouette term left out: worst gap {no_sil[q].max():.3f}; interior term left out: {no_int[q].max():.3f}")
    assert no_sil[q].max() > 10 * cr.TOL
    if variant == "flat":
        assert not gi.any() and np.array_equal(no_int, gap)
    else:
        assert no_int[q].max() > 10 * cr.TOL and np.abs(g - gi).sum() > 0


def test_chain_on_a_stream_of_its_own(ctx, tmp_path, orc):
    """the attribute chain with the render and every pass given a non-default torch.cuda.Stream as stream=; only that stream is
    synchronised.  The planes of every frame are the bits of the run on the current stream (which the test above holds to the CPU
    chain), and pos.grad stays within the same bound."""
    s = cr.evaluate(tmp_path, orc, "attr")
    T0 = len(s.P)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    with torch.cuda.stream(side):
        outs, base_outs, grads = run_scene(ctx, s, side=side)
    for b in base_outs:
        same(b, s.base.out, "base frame on a side stream")
    for k, ((hi, lo), (ehi, elo)) in enumerate(zip(outs, s.ends)):
        same(hi, ehi.out, f"probe {s.names[k]} + on a side stream")
        same(lo, elo.out, f"probe {s.names[k]} - on a side stream")
    bound = s.base.interior.bound() + s.base.silhouette.bound()
    for g in grads:
        assert (np.abs(g[0, :T0].astype(np.float64) - s.base.total) <= bound).all()
        assert not g[0, T0:].any() and not g[1:].any() and not g[..., 2].any()
    torch.cuda.synchronize()


@pytest.mark.parametrize("seed", cr.POSE_SEEDS)
def test_pose_recovery_on_the_device(ctx, tmp_path, orc, seed):
    """tests/test_chain_ref.py's pose recovery with every step on the device: a fresh FrameSet at the current translation, the
    autograd chain, the loss 0.5 * sum (out - target)^2; the same lr, step count and seeds.  Float atomics reorder the sums, so the
    trajectory need not be the CPU chain's bit for bit: the final error is held to the CPU bound (twice the worst final error of
    the CPU chain), the interior term alone leaves it above 0.95 pixel, and pos.grad is finite at every step (descend asserts it)."""
    P, attr = cr.pose_scene(seed)

    def forward(Q, silhouette=True, target=None):
        fs = ctx.frameset([cr.frame_of(Q)])
        out, pos = chain(fs, Q[None], attr, silhouette=silhouette)
        grad = None
        if target is not None:
            (0.5 * (out - target).square()).sum().backward()
            grad = pos.grad[0, :len(Q)].cpu().numpy()
        torch.cuda.synchronize()
        fs.close()
        return out.detach(), grad
    target, _ = forward(cr.translated(P, cr.POSE_OFFSET))
    want = cr.loss_and_grad(tmp_path, orc, cr.translated(P, cr.POSE_OFFSET), attr, np.zeros((3, cr.H, cr.W), np.float32), want_grad=False).out
    same(target[0].cpu().numpy(), want, "the target frame")
    full = cr.descend(lambda Q: forward(Q, True, target)[1], P)
    inner = cr.descend(lambda Q: forward(Q, False, target)[1], P)
    print(f"seed {seed}: error {full[0]:.4f} -> {full[-1]:.4f} pixel on the device (CPU chain {cr.POSE_FINAL[seed]:.4f}, bound {cr.POSE_BOUND:.4f}); "
          f"interior term alone -> {inner[-1]:.4f}")
    assert inner[-1] > 0.95
    assert full[-1] < cr.POSE_BOUND
