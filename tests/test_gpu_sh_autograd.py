"""-m gpu: srz.visibility.sh_light and cube_sh as torch.autograd.Functions, against tests/shref.py's float64 torch rules run ON THE
DEVICE (torch ops, autograd's own derivative).  The forward is compared as values within the binary32 rule's rounding bound against
binary64 (tests/test_sh_ref.py derives it: 33 u 2 Kmax sum_k |sh_k| for sh_light; cube_bound for cube_sh).  Gradients lie within
TWICE the propagated bound:
  gsh    every term g_c e_k carries 25 u |g_c| 2 Kmax (e_k's roundings and the product's), and the fixed tree adds gamma_n sum |term|;
  gnrm   (C + 64) u 4 24 G inl, G = Kmax sum |g_c| |sh_kc| (test_sh_ref's derivation);
  gsrc   a texel's nine terms w_k q_k: (16 + n + 44) u 1.1 2 FOURPI sum_k |gsh_k| / den for its own roundings, plus what an error
         d(gsh) of the incoming gradient becomes: 1.1 2 FOURPI sum_k d(gsh_k) / den (|w_k| <= 1.1 2 jac, jac <= 1).
The chain cube_sh -> sh_light -> a linear loss leaves an env.grad that matches the float64 composition within that bound; only the
inputs that require a gradient get one, and the backward asks the library for nothing else; sh_light's output is accepted as ibl's
irr."""
import numpy as np
import pytest
import torch

import shref
import srz
from srz import abi
from srz import visibility as V
from support import ctx, frame, soup  # noqa: F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
KMAX = float(shref.YC.max())
W, H, N_FR = 70, 50, 2
KINDS = {"irradiance": shref.IRRADIANCE, "radiance": shref.RADIANCE}


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


@pytest.fixture(scope="module")
def scene(ctx):
    """a two-frame set with a hand-written visibility buffer: every pixel owned but one in ten"""
    fs = ctx.frameset([frame(soup(1, 20, W, H, np.float32([1, 2, 3, 4])), W, H) for _ in range(N_FR)])
    rng = np.random.default_rng(71)
    ids = rng.integers(1, 21, (N_FR, H, W)).astype(np.uint32)
    ids[rng.random(ids.shape) < 0.1] = 0
    v = np.zeros((N_FR, 4, H, W), np.float32)
    v[:, 1] = ids.view(np.float32)
    yield fs, torch.as_tensor(v).cuda(), ids != 0
    fs.close()


def gamma(n):
    return n * U / (1 - n * U)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n_ch,per_frame", [(1, False), (3, True), (7, False)])
def test_sh_light_against_the_float64_rule(scene, kind, n_ch, per_frame):
    fs, vis, own = scene
    per = [shref.make_planes(72 + i, (H, W), n_ch) for i in range(N_FR)]
    nw, gw = np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
    nw[:, :, 3, 5] = 0  # not lit
    shw = shref.make_sh(73, n_ch, frames=N_FR if per_frame else None)
    sh, nrm = dev(shw).requires_grad_(True), dev(nw).requires_grad_(True)
    out = V.sh_light(fs, vis, sh, nrm, kind)
    assert tuple(out.shape) == (N_FR, n_ch, H, W) and out.requires_grad
    out.backward(dev(gw))
    sh64, nrm64 = dev(shw, torch.float64).requires_grad_(True), dev(nw, torch.float64).requires_grad_(True)
    mask = dev(own[:, None], torch.float64)
    ref = shref.torch_rule(sh64, nrm64, KINDS[kind]) * mask
    ref.backward(dev(gw, torch.float64))
    torch.cuda.synchronize()
    got, want = out.detach().cpu().numpy().astype(np.float64), ref.detach().cpu().numpy()
    S = np.abs(np.float64(shw)).sum(-2)  # [C] or [frames, C]
    S = S[:, :, None, None] if per_frame else S[None, :, None, None]
    assert (np.abs(got - want) <= 33 * U * 2 * KMAX * S).all() and (got[:, :, 3, 5] == 0).all() and (got[~np.broadcast_to(own[:, None], got.shape)] == 0).all()
    # gnrm
    g64, s64 = np.abs(np.float64(gw)), np.abs(np.float64(shw))
    G = KMAX * (np.einsum("fcyx,fkc->fyx", g64, s64) if per_frame else np.einsum("fcyx,kc->fyx", g64, s64))
    with np.errstate(divide="ignore"):
        inl = 1.0 / np.sqrt((np.float64(nw) ** 2).sum(1))
    inl[:, 3, 5] = 0
    err = np.abs(nrm.grad.cpu().numpy().astype(np.float64) - nrm64.grad.cpu().numpy())
    bound = (n_ch + 64) * U * 4 * 24 * G * inl
    print(f"gnrm: max err / bound {np.max(err[:, 0][bound > 0] / bound[bound > 0]):.3f}")
    assert (err <= 2 * bound[:, None]).all()
    # gsh
    lit = own.copy()
    lit[:, 3, 5] = False
    gm = g64 * lit[:, None]
    n = lit.sum((1, 2)) if per_frame else np.full(1, lit.sum())
    sum_g = gm.sum((2, 3)) if per_frame else gm.sum((0, 2, 3))[None]  # [rows, C]
    # sum |term| <= 2 Kmax sum |g|: the bound needs no per-pixel e_k (|e_k| <= 2 Kmax)
    bound = (gamma(n + (0 if per_frame else N_FR))[:, None] + 25 * U) * 2 * KMAX * sum_g
    err = np.abs(sh.grad.cpu().numpy().astype(np.float64) - sh64.grad.cpu().numpy()).reshape(len(n), 9, n_ch)
    print(f"gsh: max err / bound {np.max(err / bound[:, None]):.3f}")
    assert (err <= 2 * bound[:, None]).all() and (sh.grad != 0).all()


def cube_bounds(cube, n, gsh, d_gsh=0.0):
    """(the forward's bound [frames, C] — test_sh_ref's cube_bound —, the backward's [frames, C] per texel)"""
    _, jac = shref.cube_geometry(n)
    den = jac.sum()
    depth = -(-n // 64) + n + 12
    fwd = (16 + 2 * depth + 4) * U * shref.FOURPI * 1.1 * 2 * np.einsum("fyx,bfyxc->bc", jac, np.abs(np.float64(cube))) / den
    bwd = 1.1 * 2 * shref.FOURPI / den * ((16 + n + 44) * U * np.abs(np.float64(gsh)).sum(1) + np.broadcast_to(d_gsh, gsh.shape).sum(1))
    return fwd, bwd


@pytest.mark.parametrize("n,n_ch,frames", [(3, 7, 1), (8, 3, 2), (65, 1, 1)])
def test_cube_sh_against_the_float64_rule(ctx, n, n_ch, frames):
    cw = shref.make_cube(74, n, n_ch, frames)
    gw = np.random.default_rng(75).normal(0, 1, (frames, 9, n_ch)).astype(np.float32)
    for batched in ((True,) if frames > 1 else (True, False)):
        c32 = dev(cw if batched else cw[0]).requires_grad_(True)
        c64 = dev(cw if batched else cw[0], torch.float64).requires_grad_(True)
        sh = V.cube_sh(ctx, c32)
        assert tuple(sh.shape) == ((frames, 9, n_ch) if batched else (9, n_ch))
        sh.backward(dev(gw if batched else gw[0]))
        ref = shref.torch_cube_rule(c64)
        ref.backward(dev(gw if batched else gw[0], torch.float64))
        torch.cuda.synchronize()
        fwd, bwd = cube_bounds(cw, n, gw)
        err = np.abs(sh.detach().cpu().numpy().astype(np.float64) - ref.detach().cpu().numpy()).reshape(frames, 9, n_ch)
        assert (err <= fwd[:, None]).all()
        gerr = np.abs(c32.grad.cpu().numpy().astype(np.float64) - c64.grad.cpu().numpy()).reshape(cw.shape)
        print(f"cube_sh n {n}: forward err / bound {np.max(err / fwd[:, None]):.4f}, gsrc err / bound {np.max(gerr / bwd[:, None, None, None]):.4f}")
        assert (gerr <= 2 * bwd[:, None, None, None]).all() and (c32.grad != 0).any()


def test_the_chain_from_the_environment(scene, monkeypatch):
    """env -> cube_sh -> sh_light -> a linear loss: env.grad against the float64 composition; the normals get no gradient when they
    do not ask, and then the library is asked for d_gsh alone; nothing asks: no backward at all"""
    fs, vis, own = scene
    n, n_ch = 8, 3
    cw = shref.make_cube(76, n, n_ch, 1)[0]
    per = [shref.make_planes(77 + i, (H, W), n_ch) for i in range(N_FR)]
    nw, ww = np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
    calls = []
    real = srz.FrameSet.sh_grad
    monkeypatch.setattr(srz.FrameSet, "sh_grad", lambda self, *a, **k: (calls.append(a), real(self, *a, **k))[1])
    env, nrm = dev(cw).requires_grad_(True), dev(nw)
    out = V.sh_light(fs, vis, V.cube_sh(fs, env), nrm)
    (out * dev(ww)).sum().backward()
    torch.cuda.synchronize()
    assert nrm.grad is None and len(calls) == 1
    assert calls[0][7] is None and calls[0][8] is not None  # (d_gnrm_ptr, d_gsh_ptr): the coefficients' gradient alone
    env64 = dev(cw, torch.float64).requires_grad_(True)
    mask = dev(own[:, None], torch.float64)
    ref = shref.torch_rule(shref.torch_cube_rule(env64), dev(nw, torch.float64), shref.IRRADIANCE) * mask
    (ref * dev(ww, torch.float64)).sum().backward()
    # the loss is linear in out, so gsh = sum w e does not depend on the coefficients' own rounding: the propagated bound is gsh's, through
    # the gather
    gm = np.abs(np.float64(ww)) * own[:, None]
    d_gsh = (gamma(own.sum() + N_FR) + 25 * U) * 2 * KMAX * gm.sum((0, 2, 3))  # [C]
    gsh_abs = 2 * KMAX * gm.sum((0, 2, 3))  # |gsh_k| <= 2 Kmax sum |w|
    _, bwd = cube_bounds(cw[None], n, np.broadcast_to(gsh_abs, (1, 9, n_ch)), np.broadcast_to(d_gsh, (1, 9, n_ch)))
    err = np.abs(env.grad.cpu().numpy().astype(np.float64) - env64.grad.cpu().numpy())
    print(f"chain: env.grad max err {err.max():.3e}, err / bound {np.max(err / bwd[0]):.4f}")
    assert (err <= 2 * bwd[0]).all() and (env.grad != 0).all()
    # the normals ask too: one launch for both; nobody asks: no graph
    env2, nrm2 = dev(cw).requires_grad_(True), dev(nw).requires_grad_(True)
    V.sh_light(fs, vis, V.cube_sh(fs, env2), nrm2).sum().backward()
    assert len(calls) == 2 and calls[1][7] is not None and calls[1][8] is not None and nrm2.grad is not None and env2.grad is not None
    plain = V.sh_light(fs, vis, V.cube_sh(fs, dev(cw)), nrm)
    assert not plain.requires_grad and plain.grad_fn is None
    only = dev(nw).requires_grad_(True)
    V.sh_light(fs, vis, dev(shref.make_sh(78, n_ch)), only).sum().backward()
    assert len(calls) == 3 and calls[2][7] is not None and calls[2][8] is None and only.grad is not None


def test_sh_light_is_accepted_as_ibls_irradiance(scene):
    """sh = cube_sh(env); irr = sh_light(fs, vis, sh, nrm); out = ibl(..., irr, ...): the chain runs, and with metallic 0, a zero
    specular cube and base ones, ibl's output IS irr; the gradient reaches the environment"""
    fs, vis, own = scene
    env = dev(shref.make_cube(79, 8, 3, 1)[0]).requires_grad_(True)
    nrm = dev(np.stack([shref.make_planes(80 + i, (H, W), 3)[0] for i in range(N_FR)]))
    irr = V.sh_light(fs, vis, V.cube_sh(fs, env), nrm)
    shape = fs.interpolate_shape
    mat = torch.zeros(shape(2), device="cuda")
    mat[:, 0] = 0.5
    nv = torch.full(shape(1), 0.7, device="cuda")
    spec = torch.zeros(shape(3), device="cuda")
    tab = V.brdf_table(fs, 8, 16)
    out = V.ibl(fs, vis, None, mat, nv, irr, spec, tab)
    assert torch.equal(out, irr.detach() * 1.0) and bool((out != 0).any())
    out.sum().backward()
    assert env.grad is not None and bool(torch.isfinite(env.grad).all()) and bool((env.grad != 0).any())
    # and against the all-pairs path it replaces: texture_cube(cube_irradiance(env, 8), nrm) on a smooth environment, within the
    # truncation tests/test_sh_ref.py measured between the two references (1.52e-3 of the largest value) plus the lookup's bilinear
    # interpolation on an 8 x 8 cube, which is second order in the texel (1 / 8)^2 of the irradiance's curvature: <= 2 % here
    (x, y, z), _ = shref.cube_geometry(32)
    smooth = dev(np.stack([np.exp(1.5 * (0.6 * x + 0.3 * y + 0.74 * z)), 1.0 + 0.3 * z ** 3 + 0.2 * x, np.exp(-2 * (1 - y))], -1))
    a = V.sh_light(fs, vis, V.cube_sh(fs, smooth), nrm)
    b = V.texture_cube(fs, vis, V.cube_irradiance(fs, smooth, 8), nrm)
    diff = float((a - b).abs().max() / b.abs().max())
    print(f"sh_light(cube_sh(env)) against texture_cube(cube_irradiance(env, 8)): {diff:.4f} of the largest value")
    assert diff <= 0.02
