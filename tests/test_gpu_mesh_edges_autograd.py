"""-m gpu: srz.visibility.mesh_edge_counts, mesh_edge_lengths, mesh_normal_consistency and the two losses over them, against a binary64
restatement in torch ops on the device (edgeref.torch_terms over a host-built edge table, differentiated by torch).  Tolerances:
tests/edgeref.py's DERIVED bounds, carried through the chain below — not measured."""
import inspect

import numpy as np
import pytest
import torch

import edgeref as er
import vgkit
from srz import visibility as V
from support import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

SLOT = 9
MESHES = {k: v for k, v in er.meshes().items() if k in ("book", "octa", "fan", "grid257", "flat")}
U = er.U


def setup(c, name):
    pos, faces = MESHES[name]()
    c.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    return pos, faces, torch.as_tensor(faces.astype(np.int64)).cuda(), torch.as_tensor(er.pair_table(faces)).cuda()


def sets_of(pos):
    moved = (pos + np.random.default_rng(271).uniform(-0.01, 0.01, pos.shape)).astype(np.float32)
    return np.stack([pos, moved])


@pytest.mark.parametrize("name", list(MESHES))
def test_counts(ctx, tmp_path, name):
    pos, faces, _, _ = setup(ctx, name)
    L = er.Lists(tmp_path, faces, len(pos))
    n = V.mesh_edge_counts(ctx, SLOT)
    assert n.shape == (len(faces), 3) and n.dtype == torch.float32 and not n.requires_grad and n.grad_fn is None
    assert np.array_equal(n.cpu().numpy(), er.forward(tmp_path, L, None, "count"))


@pytest.mark.parametrize("kind", ["length", "dihedral"])
@pytest.mark.parametrize("name", list(MESHES))
def test_values_and_gradients_of_the_functions(ctx, tmp_path, name, kind):
    """y = f(pos), two sets in one call, within edgeref.bound of the binary64 restatement; the gradient of (y * g).sum() for a fixed
    binary32 g — gout is g itself on both sides — within TWICE edgeref.grad_bound(g): the bound holds the binary32 backward to the
    binary64 rule, the factor 2 covers torch's own binary64 evaluation and is about nine times the worst ratio measured on an MI355X
    (0.21)"""
    pos, faces, d_faces, d_pairs = setup(ctx, name)
    L = er.Lists(tmp_path, faces, len(pos))
    fn = V.mesh_edge_lengths if kind == "length" else V.mesh_normal_consistency
    ps = sets_of(pos)
    g = np.random.default_rng([len(name), 277]).uniform(-1, 1, (2, len(faces), 3)).astype(np.float32)
    x = torch.as_tensor(ps).cuda().requires_grad_(True)
    y = fn(ctx, SLOT, x)
    assert y.shape == (2, len(faces), 3) and y.dtype == torch.float32 and y.requires_grad
    (y * torch.as_tensor(g).cuda()).sum().backward()
    torch.cuda.synchronize()
    assert x.grad is not None and x.grad.shape == x.shape
    for s in range(2):
        x64 = torch.as_tensor(ps[s].astype(np.float64)).cuda().requires_grad_(True)
        y64 = er.torch_terms(x64, d_faces, d_pairs, kind)
        (y64 * torch.as_tensor(g[s].astype(np.float64)).cuda()).sum().backward()
        e_y = er.bound(tmp_path, L, ps[s], kind)
        err = np.abs(y[s].detach().cpu().numpy().astype(np.float64) - y64.detach().cpu().numpy())
        assert np.isfinite(e_y).all() and (err <= e_y + 1e-14).all(), (s, np.argwhere(err > e_y)[:4].tolist())
        e_g = er.grad_bound(tmp_path, L, ps[s], kind, g[s])
        want = x64.grad.cpu().numpy()
        gerr = np.abs(x.grad[s].cpu().numpy().astype(np.float64) - want)
        some = e_g > 0
        print(f"{name} {kind} set {s}: max |y| {np.abs(y64.detach().cpu().numpy()).max():.3e} err / bound "
              f"{(err[e_y > 0] / e_y[e_y > 0]).max() if (e_y > 0).any() else 0:.3f}; max |grad| {np.abs(want).max():.3e} err / bound "
              f"{(gerr[some] / e_g[some]).max() if some.any() else 0:.3f}")
        assert np.isfinite(e_g).all() and (gerr <= 2 * e_g + 1e-13).all(), (s, np.argwhere(gerr > 2 * e_g)[:4].tolist())
    # an x that does not require a gradient gets none; one [V, 3] set is the first of the two, bit for bit
    plain = fn(ctx, SLOT, x.detach())
    assert not plain.requires_grad and torch.equal(plain, y.detach())
    assert torch.equal(fn(ctx, SLOT, x.detach()[0]), y.detach()[0])


@pytest.mark.parametrize("name", list(MESHES))
def test_the_losses(ctx, tmp_path, name):
    """mesh_edge_loss and mesh_normal_loss against the same means over the binary64 restatement.  Values: the terms' bounds through the
    mean; the sums are torch's, in no stated order: an element passes at most n adds of its sum and the divisor W = sum 1 / count as
    many, n the number of elements, and a term and the division eight roundings more — gamma_(2n+8) of the sum of absolute terms.
    The target is a binary fraction, the same number on both sides.  Gradients: gout is 2 w (len - target) / W (resp. 1 / P), off by
    the length's bound and the same gamma — carried through grad_bound's e_gout — within twice the bound, as above"""
    pos, faces, d_faces, d_pairs = setup(ctx, name)
    L = er.Lists(tmp_path, faces, len(pos))
    count = er.forward(tmp_path, L, None, "count").astype(np.float64)
    w, W, P = 1.0 / count, (1.0 / count).sum(), (count - 1.0).sum()
    n_el = count.size
    target = 0.0625
    g_sum = er.gamma(2 * n_el + 8)
    x = torch.as_tensor(pos).cuda().requires_grad_(True)
    x64 = torch.as_tensor(pos.astype(np.float64)).cuda().requires_grad_(True)
    d_w = torch.as_tensor(w).cuda()
    for which in ("edge", "normal"):
        x.grad = x64.grad = None
        if which == "edge":
            loss = V.mesh_edge_loss(ctx, SLOT, x, target)
            y64 = er.torch_terms(x64, d_faces, d_pairs, "length")
            loss64 = (d_w * (y64 - target) ** 2).sum() / W
            e_y = er.bound(tmp_path, L, pos, "length")
            d = np.abs(y64.detach().cpu().numpy() - target)
            terms, e_terms = w * d * d, w * (2 * d * e_y + e_y * e_y)
            gout32 = (2 * w * (y64.detach().cpu().numpy() - target) / W).astype(np.float32)
            e_gout = 2 * w * e_y / W * (1 + g_sum) + g_sum * np.abs(gout32)
            bound_of, total = "length", W
        else:
            loss = V.mesh_normal_loss(ctx, SLOT, x)
            y64 = er.torch_terms(x64, d_faces, d_pairs, "dihedral")
            loss64 = y64.sum() / max(P, 1.0)
            e_y = er.bound(tmp_path, L, pos, "dihedral")
            terms, e_terms = np.abs(y64.detach().cpu().numpy()), e_y
            gout32 = np.full(count.shape, 1.0 / max(P, 1.0)).astype(np.float32)
            e_gout = U * np.abs(gout32) * 2
            bound_of, total = "dihedral", max(P, 1.0)
        assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
        loss.backward()
        loss64.backward()
        torch.cuda.synchronize()
        e_loss = (e_terms.sum() * (1 + g_sum) + g_sum * terms.sum()) / total
        err = abs(float(loss) - float(loss64))
        e_g = er.grad_bound(tmp_path, L, pos, bound_of, gout32, e_gout)
        want = x64.grad.cpu().numpy()
        gerr = np.abs(x.grad.cpu().numpy().astype(np.float64) - want)
        some = e_g > 0
        print(f"{name} {which}: loss {float(loss64):.6e} err / bound {err / max(e_loss, 1e-300):.3f}; max |grad| {np.abs(want).max():.3e} "
              f"err / bound {(gerr[some] / e_g[some]).max() if some.any() else 0:.3f}")
        assert err <= e_loss + 1e-14, (which, err, e_loss)
        assert np.isfinite(e_g).all() and (gerr <= 2 * e_g + 1e-13).all(), (which, np.argwhere(gerr > 2 * e_g)[:4].tolist())
    # two sets give a loss per set
    two = V.mesh_edge_loss(ctx, SLOT, torch.as_tensor(sets_of(pos)).cuda(), target)
    assert two.shape == (2,) and abs(float(two[0]) - float(V.mesh_edge_loss(ctx, SLOT, x.detach(), target))) <= g_sum * float(two[0])


def test_the_chain_from_a_solve_runs(ctx):
    """mesh_normal_consistency(mesh_solve(u)): the backward runs through both and u.grad is finite, of u's shape, and not zero"""
    pos, faces, _, _ = setup(ctx, "grid257")
    u = torch.as_tensor(pos).cuda().requires_grad_(True)
    y = V.mesh_normal_consistency(ctx, SLOT, V.mesh_solve(ctx, SLOT, u, 2.0, "graph", iters=16))
    (y * torch.as_tensor(np.random.default_rng(281).uniform(0, 1, (len(faces), 3)).astype(np.float32)).cuda()).sum().backward()
    torch.cuda.synchronize()
    assert u.grad.shape == u.shape and torch.isfinite(u.grad).all() and u.grad.abs().max() > 0


def test_the_layer_adds_no_refusal_of_its_own(ctx):
    """a tensor the layer cannot pass on is _sets_arg's to refuse, naming the function; the rest is the library's"""
    import srz
    pos, faces, _, _ = setup(ctx, "fan")
    x = torch.as_tensor(pos).cuda()
    for fn, who in ((V.mesh_edge_lengths, "mesh_edge_lengths"), (V.mesh_normal_consistency, "mesh_normal_consistency")):
        for bad in (None, x.cpu(), x.double(), x[:-1], x.reshape(-1), x[None, None], torch.zeros((len(pos), 4), device="cuda")):
            with pytest.raises(ValueError, match=who + ": pos must be a CUDA float32 tensor"):
                fn(ctx, SLOT, bad)
    for fn in (V._face_field, V.mesh_edge_counts, V._MeshEdges, V.mesh_edge_lengths, V.mesh_normal_consistency, V.mesh_edge_loss, V.mesh_normal_loss):
        assert "raise " not in inspect.getsource(fn)
    with pytest.raises(srz.SrzError, match="srz_mesh_edges: no mesh in that slot"):
        ctx.mesh_sizes[200] = (3, 1)
        try:
            V.mesh_edge_counts(ctx, 200)
        finally:
            del ctx.mesh_sizes[200]
