"""-m gpu: the environment-lit chain through srz.visibility's autograd on a 64 x 64 frame of one mesh — cube_irradiance and
cube_prefilter_pyramid of an 8 x 8 environment → reflect → texture_cube (irradiance, at the normal) and texture_cube_mip (the GGX
levels, at R and roughness * (levels - 1)) → ibl → a squared loss — held to THE SAME CHAIN with reflect and ibl replaced by their torch
float64 restatements (tests/iblref.py's torch_reflect and torch_ibl, pinned to the CPU reference by tests/test_ibl_ref.py): the
gradients to the environment, base colour, material, normals, positions, eye and table.  The margin is the one tests/test_ibl_ref.py
measured for binary32 against binary64 on the CPU (8 x iblref.MEASURED_IBL, of the gradient's largest magnitude).  Also: the two
autograd Functions against the plain calls, and the eye's gradient against minus the summed position gradient."""
import numpy as np
import pytest
import torch

import iblref as ib
import vgkit
from srz import abi
from srz import visibility as V
from support import ctx, scene_pair, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

W = H = 64
SLOT = 3
ROUGHS = (0.35, 0.7, 1.0)  # the GGX levels 1 .. 3 of the 8 x 8 environment
MARGIN = 8 * max(ib.MEASURED_REFLECT, ib.MEASURED_IBL)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def scene(ctx):
    """one frame of one mesh (a 16 x 16 grid under a perspective matrix) → (fs, vis, the leaves' values: nrm, pos [1, 3, H, W] as the
    chain's own passes give them, base, mat, env, eye, tab)"""
    ident = np.eye(4, dtype=np.float32).reshape(16)
    posn, faces = vgkit.grid(16, 16, 3, extra=1)
    mvp = vgkit.perspective(50.0, 46.0, 5.0, 6.0)
    faces = vgkit.oriented(posn, faces, mvp)
    sf, f = scene_pair([(vgkit.verts8(posn), faces, abi.SHADER_NORMAL, -1, mvp, ident)], W, H, (0.0, 0.0, 1.0), [], 1.75, 0.5, ctx=ctx, slots=[SLOT])
    fs = ctx.frameset([sf])
    vis = visibility(fs)
    verts = dev(posn)
    nrm = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: V.mesh_normals(ctx, SLOT, verts)}, pos_tris=f.n_tris))
    pos = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: verts}, pos_tris=f.n_tris))
    own = ((words(vis)[0, 1] & 0x7fffffff) - np.uint32(1)) < f.n_tris
    assert own.sum() > 500
    # the eye on the side the normals face, off the axis: nv well inside (0, 1) over the mesh
    side = float(np.sign(nrm[0, 2].sum().item()))
    eye = dev(posn.mean(0) + np.float32([0.35, -0.3, 2.0 * side]))
    rng = np.random.default_rng(23)
    base = dev(rng.uniform(0.2, 1.0, (1, 3, H, W)))
    mat = dev(rng.uniform(0.15, 0.9, (1, 2, H, W)))
    env = dev(rng.uniform(0.1, 2.0, (6, 8, 8, 3)))
    return fs, vis, own, [nrm.detach(), pos.detach(), base, mat, env, eye, V.brdf_table(ctx, 8, 32)]


def chain(fs, vis, leaves, library):
    """the chain on fresh leaves → (loss, the leaves); library: reflect and ibl are the library's passes, else their torch float64
    restatements between the same float32 lookups"""
    nrm, pos, base, mat, env, eye, tab = leaves = [t.clone().requires_grad_(True) for t in leaves]
    L = len(ROUGHS) + 1
    irr_cube, pyramid = V.cube_irradiance(fs, env, 8), V.cube_prefilter_pyramid(fs, env, ROUGHS)
    if library:
        rf = V.reflect(fs, vis, nrm, pos, eye)
    else:
        rf = ib.torch_reflect(nrm.double(), pos.double(), eye.double()).float()
    lam = (mat[:, :1] * (L - 1)).contiguous()
    spec = V.texture_cube_mip(fs, vis, env, rf[:, :3].contiguous(), lam, n_levels=L, mip=pyramid)
    irr = V.texture_cube(fs, vis, irr_cube, nrm)
    if library:
        out = V.ibl(fs, vis, base, mat, rf[:, 3:].contiguous(), irr, spec, tab)
    else:
        out = ib.torch_ibl(base.double(), mat.double(), rf[:, 3:].double(), irr.double(), spec.double(), tab.double())
    return out, leaves


def test_the_environment_lit_chain_against_its_float64_restatement(ctx):
    fs, vis, own, values = scene(ctx)
    mask = dev(own[None, None].astype(np.float32))
    grads = {}
    for library in (True, False):
        out, leaves = chain(fs, vis, values, library)
        assert out.shape == (1, 3, H, W)
        (out * mask.to(out.dtype)).square().sum().backward()  # (the restatement takes every pixel as owned: nobody's are masked out)
        torch.cuda.synchronize()
        grads[library] = [t.grad.double().cpu().numpy() for t in leaves]
        if library:
            lib_out = out.detach().cpu().numpy()
            assert not lib_out[0][:, ~own].any() and np.isfinite(lib_out).all() and (lib_out[0][:, own] > 0).mean() > 0.95
        else:
            err = np.abs(out.detach().cpu().numpy()[0][:, own] - lib_out[0][:, own]).max() / np.abs(lib_out).max()
            print(f"forward: {err:.3g} of the frame's max (margin {MARGIN:.3g})")
            assert err <= MARGIN
    worst = {}
    for name, a, b in zip(("normals", "positions", "base colour", "material", "environment", "eye", "table"), grads[True], grads[False]):
        assert np.isfinite(a).all() and np.isfinite(b).all() and (b != 0).sum() > b.size // 20, name
        worst[name] = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"gradient to the {name}: {worst[name]:.3g} of its largest magnitude (margin {MARGIN:.3g})")
    bad = {k: v for k, v in worst.items() if not v <= MARGIN}
    assert not bad, bad
    fs.close()


def test_the_autograd_functions_are_the_plain_calls(ctx, monkeypatch):
    """reflect and ibl under autograd: the forward's words and every gradient are the plain calls', one backward launch each that asks
    only for what is needed; the eye's gradient is minus the owned pixels' position gradient summed per frame, or over all frames for a
    shared eye: translation invariance"""
    import srz
    fs, vis, own, (nrm, pos, base, mat, env, eye, tab) = scene(ctx)
    calls = []
    for name in ("reflect_grad", "ibl_grad"):
        real = getattr(srz.FrameSet, name)
        monkeypatch.setattr(srz.FrameSet, name, lambda self, *a, _r=real, _n=name, **k: (calls.append((_n, a)), _r(self, *a, **k))[1])
    for e0 in (eye, eye.reshape(1, 3)):
        nt, pt, et = (t.clone().requires_grad_(True) for t in (nrm, pos, e0))
        rf = V.reflect(fs, vis, nt, pt, et)
        g = dev(np.random.default_rng(3).normal(0, 1, (1, 4, H, W)))
        n0 = len(calls)
        (rf * g).sum().backward()
        assert len(calls) == n0 + 1
        gn, gp = V.reflect_grad(fs, vis, nrm, pos, eye, g)
        assert torch.equal(nt.grad, gn) and torch.equal(pt.grad, gp) and et.grad.shape == e0.shape
        assert torch.equal(et.grad.reshape(3), -gp.sum(dim=(2, 3)).sum(0)) and bool((et.grad != 0).all())
        assert not gp[0][:, torch.as_tensor(~own).cuda()].any()
    # only the eye needs a gradient: the launch asks for gpos alone (the pointers after d_gout: gnrm, gpos)
    et = eye.clone().requires_grad_(True)
    V.reflect(fs, vis, nrm, pos, et).sum().backward()
    assert [bool(p) for p in calls[-1][1][6:8]] == [False, True]
    rf = V.reflect(fs, vis, nrm, pos, eye)
    assert not rf.requires_grad
    nv, irr, spec = rf[:, 3:].contiguous(), dev(np.random.default_rng(4).uniform(0, 2, (1, 3, H, W))), dev(np.random.default_rng(5).uniform(0, 2, (1, 3, H, W)))
    ins = [t.clone().requires_grad_(True) for t in (base, mat, nv, irr, spec, tab)]
    out = V.ibl(fs, vis, *ins)
    g = dev(np.random.default_rng(6).normal(0, 1, (1, 3, H, W)))
    n0 = len(calls)
    (out * g).sum().backward()
    assert len(calls) == n0 + 1 and calls[-1][0] == "ibl_grad"
    plain = V.ibl_grad(fs, vis, base, mat, nv, irr, spec, tab, g)
    for name, t, p in zip(("base", "mat", "nv", "irr", "spec"), ins[:5], plain[:5]):
        assert torch.equal(t.grad, p), name
    scale = float(plain[5].abs().max())
    assert float((ins[5].grad - plain[5]).abs().max()) <= 1e-4 * scale and scale > 0  # (float adds in another order)
    # base None, and one input alone: the launch asks for that output alone (after d_gout: gbase, gmat, gnv, girr, gspec, gtab)
    tt = tab.clone().requires_grad_(True)
    V.ibl(fs, vis, None, mat, nv, irr, spec, tt).sum().backward()
    assert [bool(p) for p in calls[-1][1][9:15]] == [False, False, False, False, False, True] and bool((tt.grad != 0).any())
    with pytest.raises(ValueError):
        V.ibl(fs, vis, base, base, nv, irr, spec, tab)  # (a three-plane material)
    with pytest.raises(ValueError):
        V.ibl(fs, vis, base, mat, nv, irr, spec, tab[:, :, :1])
    with pytest.raises(ValueError):
        V.reflect(fs, vis, nrm, pos, dev(np.zeros((3, 3))))
    fs.close()
