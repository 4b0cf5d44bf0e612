"""-m gpu: srz.visibility.mesh_laplacian and mesh_solve as torch.autograd.Functions, against a binary64 restatement of the operator in
torch ops on the device (gathers and index_add, differentiated by torch) and a dense binary64 solve.  Tolerances: tests/lapref.py's
DERIVED bounds, carried through the chain below — not measured."""
import numpy as np
import pytest
import torch

import lapref as lr
import vgkit
from srz import visibility as V
from support import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

SLOT = 9
KINDS = ("umbrella", "graph", "cotan")
MESHES = {"grid257": lambda: vgkit.grid(16, 16, 3, extra=1), "fan": lambda: vgkit.fan(70, 2), "octa": lr.octahedron4}
LAM, TOL = 10.0, 1e-5


def laplacian64(x, faces, kind, wpos):
    """the rule restated in binary64 torch ops: x [V, C] float64 on the device, faces [F, 3] int64, wpos [V, 3] float64"""
    V_ = x.shape[0]
    out = torch.zeros_like(x)
    if kind == "cotan":
        p = wpos[faces]  # [F, 3, 3]
        N = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
        d2 = (N * N).sum(1)
        ok = (d2 > 0) & (d2 <= torch.finfo(torch.float32).max)
        ia = torch.where(ok, 1.0 / torch.sqrt(torch.where(ok, d2, torch.ones_like(d2))), torch.zeros_like(d2))
        cot = [((p[:, (m + 1) % 3] - p[:, m]) * (p[:, (m + 2) % 3] - p[:, m])).sum(1) * ia for m in range(3)]
        for k in range(3):
            v, a, b = faces[:, k], faces[:, (k + 1) % 3], faces[:, (k + 2) % 3]
            term = cot[(k + 2) % 3][:, None] * (x[v] - x[a]) + cot[(k + 1) % 3][:, None] * (x[v] - x[b])
            out = out.index_add(0, v[ok], 0.5 * term[ok])
        return out
    n = torch.zeros(V_, dtype=x.dtype, device=x.device)
    for k in range(3):
        v, a, b = faces[:, k], faces[:, (k + 1) % 3], faces[:, (k + 2) % 3]
        out = out.index_add(0, v, x[a] + x[b])
        n = n.index_add(0, v, torch.full_like(v, 2, dtype=x.dtype))
    n = n[:, None]
    if kind == "graph":
        return n * x - out
    return torch.where(n > 0, x - out / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(x))


def setup(c, name):
    pos, faces = MESHES[name]()
    c.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    return pos, faces, torch.as_tensor(faces.astype(np.int64)).cuda(), torch.as_tensor(pos).cuda()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(MESHES))
def test_values_and_the_gradient_of_the_penalty(ctx, tmp_path, name, kind):
    """y = mesh_laplacian(x) within lapref.bound of the binary64 restatement; the gradient of (y ** 2).sum() = L^T (2 y) within TWICE
    the propagated bound: e_y = bound(x) on y; the backward is the binary32 transpose over 2 y32 (the doubling is exact), off by
    bound_T(2 y32), and it carries the forward's error on as |L|^T (2 e_y) with |L| the matrix of absolute entries"""
    pos, faces, d_faces, d_pos = setup(ctx, name)
    L = lr.Lists(tmp_path, faces, len(pos))
    xs = np.random.default_rng([len(name), 197]).uniform(-1, 1, (2, len(pos), 5)).astype(np.float32)
    x = torch.as_tensor(xs).cuda().requires_grad_(True)
    wpos = d_pos.clone().requires_grad_(True)
    y = V.mesh_laplacian(ctx, SLOT, x, kind, wpos if kind == "cotan" else None)
    assert y.shape == x.shape and y.dtype == torch.float32 and y.requires_grad
    (y ** 2).sum().backward()
    torch.cuda.synchronize()
    assert x.grad is not None and x.grad.shape == x.shape and wpos.grad is None, "wpos is held: only x gets a gradient"
    absM = np.abs(lr.dense(tmp_path, L, kind, pos))
    for s in range(2):
        x64 = torch.as_tensor(xs[s].astype(np.float64)).cuda().requires_grad_(True)
        y64 = laplacian64(x64, d_faces, kind, d_pos.double())
        (y64 ** 2).sum().backward()
        e_y = lr.bound(L, xs[s], kind, pos)
        err = np.abs(y[s].detach().cpu().numpy().astype(np.float64) - y64.detach().cpu().numpy())
        assert np.isfinite(e_y).all() and (err <= e_y + 1e-13).all(), (s, np.argwhere(err > e_y)[:4].tolist())
        y32 = y[s].detach().cpu().numpy()
        e_g = lr.bound(L, 2 * y32, kind, pos, transpose=True) + absM.T @ (2 * e_y)
        gerr = np.abs(x.grad[s].cpu().numpy().astype(np.float64) - x64.grad.cpu().numpy())
        print(f"{name} {kind} set {s}: max |y| {np.abs(y32).max():.3e} err / bound {(err / np.maximum(e_y, 1e-300)).max():.3f}; "
              f"max |grad| {np.abs(x64.grad.cpu().numpy()).max():.3e} err / bound {(gerr / np.maximum(e_g, 1e-300)).max():.3f}")
        assert (gerr <= 2 * e_g + 1e-12).all(), (s, np.argwhere(gerr > 2 * e_g)[:4].tolist())
        assert np.median(e_g) < 1e-4 * np.abs(x64.grad.cpu().numpy()).max(), "the bound says nothing"
    # an x that does not require a gradient gets none, and neither does its output
    plain = V.mesh_laplacian(ctx, SLOT, x.detach(), kind, d_pos)
    assert not plain.requires_grad and torch.equal(plain, y.detach())
    # one [V, C] field is the first of the two sets
    assert torch.equal(V.mesh_laplacian(ctx, SLOT, x.detach()[0], kind, d_pos), y.detach()[0])


@pytest.mark.parametrize("kind", ["graph", "cotan"])
@pytest.mark.parametrize("name", list(MESHES))
def test_solve_against_a_dense_binary64_solve(ctx, tmp_path, name, kind):
    """verts = mesh_solve(u, 10, tol = 1e-5) and u.grad of (verts * g).sum() — the solve of g — against numpy's solve of the binary64
    matrix A = I + 10 L: |u - u*| <= |b - A u| (A >= I, the residual taken in binary64), and the true residual within 2 tol |b|
    (tests/test_lap_ref.py holds the loop to the same two on the CPU)"""
    pos, faces, _, d_pos = setup(ctx, name)
    L = lr.Lists(tmp_path, faces, len(pos))
    A = np.eye(len(pos)) + LAM * lr.dense(tmp_path, L, kind, pos)
    rng = np.random.default_rng([len(name), 199])
    b, g = (rng.uniform(-1, 1, (len(pos), 3)).astype(np.float32) for _ in range(2))
    u = torch.as_tensor(b).cuda().requires_grad_(True)
    verts = V.mesh_solve(ctx, SLOT, u, LAM, kind, d_pos if kind == "cotan" else None, iters=200, tol=TOL)
    assert verts.shape == u.shape and verts.requires_grad
    (verts * torch.as_tensor(g).cuda()).sum().backward()
    torch.cuda.synchronize()
    for what, rhs, got in (("forward", b, verts.detach()), ("u.grad", g, u.grad)):
        got = got.cpu().numpy().astype(np.float64)
        star = np.linalg.solve(A, rhs.astype(np.float64))
        res, nb = np.linalg.norm(rhs - A @ got), np.linalg.norm(rhs.astype(np.float64))
        print(f"{name} {kind} {what}: |u - u*| {np.linalg.norm(got - star):.3e}, true residual {res:.3e} = {res / (TOL * nb):.3f} tol |b|")
        assert np.linalg.norm(got - star) <= res and res <= 2 * TOL * nb, what


def test_without_a_tolerance_the_solve_applies_the_operator_iters_times(ctx, monkeypatch):
    """a counting wrapper on the plain call: exactly `iters` applications forward, as many backward, none elsewhere"""
    pos, faces, _, _ = setup(ctx, "grid257")
    calls = []
    plain = ctx.mesh_laplacian
    monkeypatch.setattr(ctx, "mesh_laplacian", lambda *a, **kw: (calls.append(a[5]), plain(*a, **kw))[1], raising=False)
    u = torch.as_tensor(np.random.default_rng(211).uniform(-1, 1, (2, len(pos), 3)).astype(np.float32)).cuda().requires_grad_(True)
    verts = V.mesh_solve(ctx, SLOT, u, LAM, iters=7)
    assert len(calls) == 7 and set(calls) == {1}
    verts.sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == 14 and torch.isfinite(u.grad).all()
    # the same arguments give the same bits (every step is deterministic), and a tolerance already met stops before the first step
    assert torch.equal(V.mesh_solve(ctx, SLOT, u.detach(), LAM, iters=7), verts.detach())
    calls.clear()
    assert not V.mesh_solve(ctx, SLOT, u.detach(), LAM, iters=7, tol=2.0).any() and not calls


def test_a_stream_handle_carries_the_whole_solve(ctx, monkeypatch):
    """mesh_solve(stream=handle): the loop's torch ops and the operator's launches share the handle's stream — torch's current stream
    is the handle's at every application, forward and backward, and the caller's afterwards — and the bits are the default stream's"""
    pos, faces, _, d_pos = setup(ctx, "grid257")
    b = torch.as_tensor(np.random.default_rng(227).uniform(-1, 1, (len(pos), 3)).astype(np.float32)).cuda()
    want = V.mesh_solve(ctx, SLOT, b, LAM, "cotan", iters=9)
    torch.cuda.synchronize()
    seen = []
    plain = ctx.mesh_laplacian
    monkeypatch.setattr(ctx, "mesh_laplacian", lambda *a, **kw: (seen.append((torch.cuda.current_stream().cuda_stream, a[-1])), plain(*a, **kw))[1],
                        raising=False)
    side, before = torch.cuda.Stream(), torch.cuda.current_stream().cuda_stream
    assert side.cuda_stream != before
    u = b.clone().requires_grad_(True)
    torch.cuda.synchronize()
    got = V.mesh_solve(ctx, SLOT, u, LAM, "cotan", iters=9, stream=side.cuda_stream)
    assert torch.cuda.current_stream().cuda_stream == before
    side.synchronize()
    assert torch.equal(got.detach(), want)
    with torch.cuda.stream(side):
        got.sum().backward()
    side.synchronize()
    assert len(seen) == 18 and set(seen) == {(side.cuda_stream, side.cuda_stream)}, set(seen)
    assert torch.isfinite(u.grad).all() and u.grad.abs().max() > 0


def test_the_chain_to_the_normals_runs(ctx):
    """mesh_normals(mesh_solve(u)): the backward runs through both and u.grad is finite, of u's shape, and not zero"""
    pos, faces, _, d_pos = setup(ctx, "grid257")
    u = d_pos.clone().requires_grad_(True)
    nrm = V.mesh_normals(ctx, SLOT, V.mesh_solve(ctx, SLOT, u, 2.0, "cotan", iters=16))
    (nrm * torch.as_tensor(np.random.default_rng(223).uniform(-1, 1, pos.shape).astype(np.float32)).cuda()).sum().backward()
    torch.cuda.synchronize()
    assert u.grad.shape == u.shape and torch.isfinite(u.grad).all() and u.grad.abs().max() > 0
