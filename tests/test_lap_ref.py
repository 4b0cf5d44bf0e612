"""not-gpu: the reference of the mesh Laplacian (tests/lapref.py, tests/lap_ref.c) is itself held to what the operator must be — the
backward is the transpose, UMBRELLA on a closed mesh is the uniform Laplacian, COTAN has linear precision and a matrix that is
symmetric in the bits, GRAPH and COTAN are positive semidefinite — and its binary32 evaluation to its binary64 one under the rounding
bounds DERIVED in lapref (gamma_n * sum |term|, not measured).  Also here: srz.visibility._cg, the loop of mesh_solve, over the binary32
reference operator against a dense binary64 solve."""
import numpy as np
import pytest

import lapref as lr
import vgkit

KINDS = ("umbrella", "graph", "cotan")


def flat_grid():
    pos, faces = vgkit.grid(8, 7, 4, jitter=0)
    pos[:, 2] = 0.5
    return pos, faces


MESHES = {"grid257": lambda: vgkit.grid(16, 16, 3, extra=1), "flat": flat_grid, "fan": lambda: vgkit.fan(70, 2)}


def field(seed, shape):
    return np.random.default_rng([seed, 167]).uniform(-1, 1, shape).astype(np.float32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(MESHES))
def test_the_backward_is_the_transpose(tmp_path, name, kind):
    """<L x, g> = <x, L^T g> in binary64: both sides are sums of V C products of magnitude <= |L x| |g|, so they agree to a few
    V C u64 of sum |L x| |g| + sum |x| |L^T g|"""
    pos, faces = MESHES[name]()
    L = lr.Lists(tmp_path, faces, len(pos))
    x, g = field(1, (len(pos), 3)).astype(np.float64), field(2, (len(pos), 3)).astype(np.float64)
    Lx = lr.apply(tmp_path, L, x, kind, pos, dtype=np.float64)
    Ltg = lr.apply(tmp_path, L, g, kind, pos, transpose=True, dtype=np.float64)
    lhs, rhs = (Lx * g).sum(), (x * Ltg).sum()
    scale = (np.abs(Lx) * np.abs(g)).sum() + (np.abs(x) * np.abs(Ltg)).sum()
    print(f"{name} {kind}: <Lx, g> {lhs:.6e}, relative difference {abs(lhs - rhs) / scale:.2e}")
    assert abs(lhs) > 1e-3 * scale / len(pos) and abs(lhs - rhs) <= 200 * 2.0 ** -53 * scale
    if kind != "umbrella":  # the symmetric kinds: the transposed call is the call
        assert np.array_equal(Ltg, lr.apply(tmp_path, L, g, kind, pos, dtype=np.float64))


def test_umbrella_on_a_closed_mesh_is_the_uniform_laplacian(tmp_path):
    """the octahedron with each face split in four (18 vertices, 32 faces): every edge has two faces, so a neighbour is counted twice
    and n_v is twice the valence — x[v] minus the mean over the EDGE SET's neighbours"""
    pos, faces = lr.octahedron4()
    edges = {tuple(sorted((int(f[i]), int(f[(i + 1) % 3])))) for f in faces for i in range(3)}
    assert len(pos) - len(edges) + len(faces) == 2  # (Euler: closed, genus 0)
    x = field(3, (18, 4)).astype(np.float64)
    want = np.zeros_like(x)
    for v in range(18):
        nb = [a if b == v else b for a, b in edges if v in (a, b)]
        assert len(nb) in (4, 6)
        want[v] = x[v] - x[nb].mean(0)
    got = lr.apply(tmp_path, lr.Lists(tmp_path, faces, 18), x, "umbrella", dtype=np.float64)
    assert np.abs(got - want).max() <= 16 * 2.0 ** -53 * 2.0


def test_cotan_has_linear_precision_inside_a_flat_mesh(tmp_path):
    """an affine field over a planar triangulation: zero at the interior vertices (to binary64 rounding: the terms are O(1)), the
    boundary's conormal flux on the boundary"""
    pos, faces = flat_grid()
    L = lr.Lists(tmp_path, faces, len(pos))
    p = pos.astype(np.float64)
    x = np.stack([p[:, 0] + 0.5 * p[:, 1] + 0.25, -0.3 * p[:, 0] + p[:, 1] - 1.0], 1)
    out = lr.apply(tmp_path, L, x, "cotan", pos, dtype=np.float64)
    j, i = np.divmod(np.arange(56), 8)
    inner = (i > 0) & (i < 7) & (j > 0) & (j < 6)
    assert inner.sum() == 30 and np.abs(out[inner]).max() <= 1e-13, np.abs(out[inner]).max()
    assert (np.abs(out[~inner]).max(1) > 1e-2).all(), np.abs(out[~inner]).max(1).min()
    # and the binary32 evaluation is zero there to its derived bound
    out32 = lr.apply(tmp_path, L, x.astype(np.float32), "cotan", pos)
    b = lr.bound(L, x.astype(np.float32), "cotan", pos)
    assert np.isfinite(b).all() and (np.abs(out32[inner]) <= b[inner] + 1e-13).all() and b.max() < 1e-4


@pytest.mark.parametrize("name", list(MESHES))
def test_the_cotan_matrix_is_symmetric_in_the_bits(tmp_path, name):
    """assembled from the binary32 reference: an off-diagonal entry is -0.5 times a sum of the shared faces' weights — the same words
    from both sides whenever the two lists meet the shared faces in the same order (they do: both are increasing in the face)"""
    pos, faces = MESHES[name]()
    M = lr.dense(tmp_path, lr.Lists(tmp_path, faces, len(pos)), "cotan", pos, dtype=np.float32)
    assert np.array_equal(M.view(np.uint32), np.ascontiguousarray(M.T).view(np.uint32)) and np.abs(M).max() > 0.1
    G = lr.dense(tmp_path, lr.Lists(tmp_path, faces, len(pos)), "graph", dtype=np.float32)
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize("kind", ["graph", "cotan"])
@pytest.mark.parametrize("name", list(MESHES))
def test_the_symmetric_kinds_are_positive_semidefinite(tmp_path, name, kind):
    """both are sums over the faces of positive semidefinite forms (GRAPH: (x_a - x_b)^2 per edge of a face; COTAN: the Dirichlet
    energy of the face's linear interpolant).  eigvalsh of a symmetric binary64 matrix is backward stable: an eigenvalue is off by a
    small multiple of V u64 |M|"""
    pos, faces = MESHES[name]()
    M = lr.dense(tmp_path, lr.Lists(tmp_path, faces, len(pos)), kind, pos)
    assert np.abs(M - M.T).max() <= 8 * 2.0 ** -53 * np.abs(M).max()
    ev = np.linalg.eigvalsh(0.5 * (M + M.T))
    print(f"{name} {kind}: eigenvalues {ev[0]:.3e} .. {ev[-1]:.3e}")
    assert ev[0] >= -len(pos) * 2.0 ** -52 * ev[-1] and ev[-1] > 1.0
    assert np.abs(M.sum(1)).max() <= 1e-12 * np.abs(M).max()  # (constants are in the kernel)


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(MESHES) + ["octa"])
def test_binary32_stays_within_the_derived_bounds(tmp_path, name, kind, transpose):
    pos, faces = lr.octahedron4() if name == "octa" else MESHES[name]()
    L = lr.Lists(tmp_path, faces, len(pos))
    x = field(5, (len(pos), 5))
    got = lr.apply(tmp_path, L, x, kind, pos, transpose=transpose)
    want = lr.apply(tmp_path, L, x, kind, pos, transpose=transpose, dtype=np.float64)
    b = lr.bound(L, x, kind, pos, transpose=transpose)
    err = np.abs(got.astype(np.float64) - want)
    fin = np.isfinite(b)
    ratio = err[fin & (b > 0)] / b[fin & (b > 0)]
    print(f"{name} {kind} T={transpose}: max |out| {np.abs(want).max():.3e}, max err {err.max():.3e}, max err / bound {ratio.max():.3f}, "
          f"median bound {np.median(b[fin]):.3e}, finite {int(fin.sum())} of {fin.size}")
    assert fin.mean() > 0.95 and (err[fin] <= b[fin]).all(), np.argwhere(fin & (err > b))[:4].tolist()
    assert np.median(b[fin]) < 1e-4 * np.abs(want).max(), "the bound says nothing"
    # two sets in one call are the two calls
    two = lr.apply(tmp_path, L, np.stack([x, x[::-1]]), kind, pos, transpose=transpose)
    assert np.array_equal(two[0].view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_reaches_the_vertex_and_its_neighbours_only(tmp_path, kind):
    pos, faces = vgkit.grid(6, 5, 8)
    L = lr.Lists(tmp_path, faces, len(pos))
    at = 14  # (an interior vertex)
    near = np.zeros(len(pos), bool)
    near[np.unique(faces[(faces == at).any(1)])] = True
    assert 5 <= near.sum() <= 9
    x = field(6, (len(pos), 2))
    x[at, 1] = np.nan
    for transpose in (False, True):
        out = lr.apply(tmp_path, L, x, kind, pos, transpose=transpose)
        assert not np.isnan(out[:, 0]).any() and np.array_equal(np.isnan(out[:, 1]), near), (kind, transpose)


def test_a_zero_area_face_under_cotan_contributes_nothing(tmp_path):
    """vertex 0 belongs to a good face (0, 1, 2) and to a collinear one (0, 3, 4) whose cross product is exactly zero, with an
    INFINITE x behind it: the face is skipped, never multiplied by zero — out[0] is the good face's alone, 3 and 4 get +0"""
    pos = np.float32([[0, 0, 0], [1, 0, 0.25], [0.25, 1, 0], [1, 1, 1], [2, 2, 2]])
    faces = np.array([[0, 1, 2], [0, 3, 4]], np.uint32)
    x = np.float32([[0.5], [-1.0], [3.0], [np.inf], [-np.inf]])
    out = lr.apply(tmp_path, lr.Lists(tmp_path, faces, 5), x, "cotan", pos)
    alone = lr.apply(tmp_path, lr.Lists(tmp_path, faces[:1], 5), x, "cotan", pos)
    assert np.isfinite(out).all() and np.array_equal(out.view(np.uint32), alone.view(np.uint32)) and out[0, 0] != 0
    assert not out[3:].view(np.uint32).any()
    assert not np.isfinite(lr.apply(tmp_path, lr.Lists(tmp_path, faces, 5), x, "graph")[0, 0])  # (the other kinds do read it)


# ------------------------------------------------------------------------------------------------ the loop of mesh_solve
LAM, TOL = 10.0, 1e-5


@pytest.mark.parametrize("kind", ["graph", "cotan"])
@pytest.mark.parametrize("name", list(MESHES))
def test_cg_against_a_dense_binary64_solve(tmp_path, name, kind):
    """srz.visibility._cg over the binary32 reference operator, A = I + 10 L, tol 1e-5, against numpy's solve of the binary64 matrix.
    A >= I (L is positive semidefinite), so |u - u*| = |A^-1 (b - A u)| <= |b - A u| with the residual taken in binary64; and the
    true residual is within 2 tol |b|: the recursive one is <= tol |b| at the stop, the factor 2 covers its drift from the true
    one (binary32 rounding of the operator and of the updates)"""
    import torch
    from srz import visibility as V
    pos, faces = MESHES[name]()
    L = lr.Lists(tmp_path, faces, len(pos))
    A = np.eye(len(pos)) + LAM * lr.dense(tmp_path, L, kind, pos)
    b = field(7, (len(pos), 3))
    calls = []

    def op(p):
        calls.append(1)
        return p + LAM * torch.as_tensor(lr.apply(tmp_path, L, p.numpy(), kind, pos))
    u = V._cg(op, torch.as_tensor(b), 200, TOL).numpy().astype(np.float64)
    star = np.linalg.solve(A, b.astype(np.float64))
    res = np.linalg.norm(b - A @ u)
    nb = np.linalg.norm(b.astype(np.float64))
    print(f"{name} {kind}: {len(calls)} iterations, |u - u*| {np.linalg.norm(u - star):.3e}, true residual {res:.3e} = {res / (TOL * nb):.3f} tol |b|")
    assert 3 < len(calls) < 200
    assert np.linalg.norm(u - star) <= res
    assert res <= 2 * TOL * nb
    # tol None: exactly `iters` applications, and more of them do not make it worse
    calls.clear()
    u8 = V._cg(op, torch.as_tensor(b), 8, None).numpy()
    assert len(calls) == 8 and np.isfinite(u8).all()


def test_cg_takes_a_zero_step_where_it_would_divide_by_zero():
    """b = 0: r . r and p . Ap are zero from the start; the result is zero, never NaN"""
    import torch
    from srz import visibility as V
    u = V._cg(lambda p: 11.0 * p, torch.zeros(5, 3), 4, None)
    assert not u.numpy().view(np.uint32).any()
    u = V._cg(lambda p: 2.0 * p, torch.ones(5, 3), 4, None)  # (exact after one step: the later ones are zero steps)
    assert np.array_equal(u.numpy(), np.full((5, 3), 0.5, np.float32))
