"""not-gpu: the reference of the mesh edge terms (tests/edgeref.py, tests/edge_ref.c) is itself held to what the terms must be — the
neighbour walk over the corner lists finds the adjacency an edge dictionary has, the binary64 rules agree with a numpy restatement over
that dictionary and with torch's autograd of a restatement in torch ops, the pair's term is one word from both sides — and its binary32
evaluation to its binary64 one under the rounding bounds DERIVED in edgeref (gamma_n * sum |term|, not measured)."""
import numpy as np
import pytest

import edgeref as er
import vgkit

MESHES = er.meshes()
U64 = 2.0 ** -53


def field(seed, shape):
    return np.random.default_rng([seed, 229]).uniform(-1, 1, shape).astype(np.float32)


@pytest.mark.parametrize("name", list(MESHES))
def test_the_walk_finds_the_edge_dictionarys_adjacency(tmp_path, name):
    """the entries of every (f, j), in order, are the dictionary's other faces on the edge in face order, and COUNT is 1 + their
    number; what each mesh is here for is checked too"""
    pos, faces = MESHES[name]()
    L = er.Lists(tmp_path, faces, len(pos))
    E = er.entries(tmp_path, L)
    pairs = er.pair_table(faces)
    assert np.array_equal(np.stack([E.f, E.j, E.g, E.jp], 1), pairs)
    count = er.forward(tmp_path, L, None, "count")
    assert np.array_equal(count, 1.0 + E.n) and count.dtype == np.float32
    assert np.array_equal(er.forward(tmp_path, L, None, "count", np.float64), count)
    values = set(count.ravel().tolist())
    want = {"single": {1.0}, "pair": {1.0, 2.0}, "pair-flipped": {1.0, 2.0}, "book": {1.0, 3.0}, "octa": {2.0}, "fan": {1.0, 2.0},
            "grid257": {1.0, 2.0}, "flat": {1.0, 2.0}}[name]
    assert values == want, values
    # the relation is mutual between faces of three distinct vertices
    mutual = {(f, j, g, jp) for f, j, g, jp in pairs.tolist()}
    assert all((g, jp, f, j) in mutual for f, j, g, jp in mutual)
    if name == "fan":  # the degenerate face (1, 1, 3) follows the rule as written: no entries, three boundary edges
        assert faces[70].tolist() == [1, 1, 3] and count[70].tolist() == [1.0, 1.0, 1.0]


@pytest.mark.parametrize("name", list(MESHES))
def test_binary64_against_a_numpy_restatement(tmp_path, name):
    """LENGTH: both sides take a sum of three squares and a root: within gamma_6 (of binary64) of each other twice over.  DIHEDRAL: a
    term passes the normals' roundings (below 16 in all: edges, cross, dot3, root, division, product), dot3 and the subtraction, and at
    most m adds; numpy's restatement as many: 2 gamma_(24+m) of sum (1 + |dot|)"""
    pos, faces = MESHES[name]()
    L = er.Lists(tmp_path, faces, len(pos))
    p = pos.astype(np.float64)
    q = p[faces.astype(np.int64)]
    want = np.stack([np.linalg.norm(q[:, (j + 2) % 3] - q[:, (j + 1) % 3], axis=1) for j in range(3)], 1)
    got = er.forward(tmp_path, L, p, "length", np.float64)
    assert (np.abs(got - want) <= 2 * 6 * U64 * want).all()
    N = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
    ln = np.linalg.norm(N, axis=1)
    ok = ln > 0
    n = N / np.where(ok, ln, 1.0)[:, None]
    want, mag = np.zeros((len(faces), 3)), np.zeros((len(faces), 3))
    for f, j, g, _ in er.pair_table(faces):
        if ok[f] and ok[g]:
            want[f, j] += 1.0 - n[f] @ n[g]
            mag[f, j] += 1.0 + np.abs(n[f] * n[g]).sum()
    got = er.forward(tmp_path, L, p, "dihedral", np.float64)
    m = er.entries(tmp_path, L).n
    assert (np.abs(got - want) <= 2 * (24 + m) * U64 * mag).all(), np.abs(got - want).max()
    if name == "pair-flipped":
        assert got[0, 2] > 1.5 and got[1, 2] == got[0, 2]
    if name in ("pair", "octa"):  # (consistently wound and gently folded: every angle is below a right one)
        assert 0 < got.max() < 1.0


def test_flipped_and_coplanar_the_term_is_two(tmp_path):
    """two coplanar faces wound against each other: n_g = -n_f exactly (the same products with the factors' roles swapped), so the
    term is 1 + |n|^2: 2 to dot3's three roundings of a unit vector's squares and the normal's own error"""
    pos = np.float32([[0, 0, 0.5], [1, 0, 0.5], [0.25, 1, 0.5], [0.5, -1, 0.5]])
    faces = np.array([[0, 1, 2], [0, 1, 3]], np.uint32)
    L = er.Lists(tmp_path, faces, 4)
    out = er.forward(tmp_path, L, pos, "dihedral")
    assert out[0].tolist()[:2] == [0.0, 0.0] and out[0, 2] == out[1, 2] and abs(out[0, 2] - 2.0) <= er.dihedral_bound(tmp_path, L, pos)[0, 2]
    faces[1] = [1, 0, 3]  # consistently wound: 1 - 1
    L = er.Lists(tmp_path, faces, 4)
    assert abs(er.forward(tmp_path, L, pos, "dihedral")[0, 2]) <= er.dihedral_bound(tmp_path, L, pos)[0, 2] < 1e-5


@pytest.mark.parametrize("name", ["pair", "pair-flipped", "book", "octa", "grid257"])
def test_the_pairs_term_is_one_word_from_both_sides(tmp_path, name):
    """binary32: the two-face mesh (f, g) gives the pair's term at (f, j) and at (g, j'), bit for bit, and the same in the order (g, f)"""
    pos, faces = MESHES[name]()
    pairs = er.pair_table(faces)
    for f, j, g, jp in pairs[:: max(1, len(pairs) // 40)]:
        two = er.forward(tmp_path, er.Lists(tmp_path, faces[[f, g]], len(pos)), pos, "dihedral")
        owt = er.forward(tmp_path, er.Lists(tmp_path, faces[[g, f]], len(pos)), pos, "dihedral")
        words = {two[0, j].tobytes(), two[1, jp].tobytes(), owt[1, j].tobytes(), owt[0, jp].tobytes()}
        assert len(words) == 1 and two[0, j] > 0, (f, j, g, jp)
    if name == "octa":  # closed: every out[f][j] IS the pair's term
        out = er.forward(tmp_path, er.Lists(tmp_path, faces, len(pos)), pos, "dihedral")
        assert all(out[f, j].tobytes() == out[g, jp].tobytes() for f, j, g, jp in pairs)
    if name == "book":  # two entries per side: the sum's order is the entry order
        out = er.forward(tmp_path, er.Lists(tmp_path, faces, len(pos)), pos, "dihedral")
        t = {(f, g): er.forward(tmp_path, er.Lists(tmp_path, faces[[f, g]], len(pos)), pos, "dihedral")[0, 2] for f in range(3) for g in range(3) if f != g}
        assert out[0, 2] == np.float32(np.float32(0) + t[0, 1]) + t[0, 2] and out[2, 2] == np.float32(np.float32(0) + t[2, 0]) + t[2, 1]


def test_the_flat_grid_is_within_its_bound_of_zero(tmp_path):
    pos, faces, collapsed = er.flat_collapsed()
    L = er.Lists(tmp_path, faces, len(pos))
    w = er.normals64(L, pos)
    assert not w.ok[collapsed] and w.zero[collapsed] and w.ok.sum() == len(faces) - 1
    for dtype in (np.float32, np.float64):
        out = er.forward(tmp_path, L, pos, "dihedral", dtype)
        b = er.dihedral_bound(tmp_path, L, pos)
        assert np.isfinite(b).all() and (np.abs(out) <= b).all() and b.max() < 1e-5
        assert not out[collapsed].view(np.uint32 if dtype == np.float32 else np.uint64).any()
    assert (er.forward(tmp_path, L, pos, "length")[collapsed] == 0).sum() == 1


@pytest.mark.parametrize("kind", ["length", "dihedral"])
@pytest.mark.parametrize("name", list(MESHES))
def test_the_binary64_backward_against_torch_autograd(tmp_path, name, kind):
    """gpos of the binary64 reference against torch.autograd of er.torch_terms in float64 on the CPU.  Both are exact gradients of the
    same function evaluated in binary64; they differ by the two evaluations' roundings, which the binary32 bound scaled by
    2^-29 covers twice over (the same count of roundings, u64 for u).  And <gout, J d> = <J^T gout, d> with J d torch's jvp"""
    import torch
    pos, faces = MESHES[name]()
    L = er.Lists(tmp_path, faces, len(pos))
    gout = field(11, (len(faces), 3)).astype(np.float64)
    got = er.backward(tmp_path, L, pos.astype(np.float64), kind, gout, np.float64)
    tf, tp = torch.as_tensor(faces.astype(np.int64)), torch.as_tensor(er.pair_table(faces))
    x = torch.as_tensor(pos.astype(np.float64)).requires_grad_(True)
    y = er.torch_terms(x, tf, tp, kind)
    assert np.abs(y.detach().numpy() - er.forward(tmp_path, L, pos.astype(np.float64), kind, np.float64)).max() < 1e-13
    (y * torch.as_tensor(gout)).sum().backward()
    b = er.grad_bound(tmp_path, L, pos, kind, gout) * 2.0 ** -29
    err = np.abs(got - x.grad.numpy())
    fin = np.isfinite(b)
    ratio = float((err[fin & (b > 0)] / b[fin & (b > 0)]).max()) if (fin & (b > 0)).any() else 0.0
    print(f"{name} {kind}: max |gpos| {np.abs(got).max():.3e}, max err {err.max():.3e}, err / (2^-29 bound) {ratio:.3f}")
    assert fin.all() and (err <= 2 * b).all(), np.argwhere(err > 2 * b)[:4].tolist()
    assert not got[b == 0].any()
    d = field(12, pos.shape).astype(np.float64)
    _, Jd = torch.autograd.functional.jvp(lambda t: er.torch_terms(t, tf, tp, kind), x.detach(), torch.as_tensor(d))
    lhs, rhs = (gout * Jd.numpy()).sum(), (got * d).sum()
    scale = (np.abs(gout) * np.abs(Jd.numpy())).sum() + (np.abs(got) * np.abs(d)).sum()
    # (1 - cos is stationary on a flat mesh and a single face has no neighbour: both sides are zero there)
    assert abs(lhs - rhs) <= 1e-12 * (scale + 1.0) and (name in ("single", "flat") and kind == "dihedral" or abs(lhs) > 0)


@pytest.mark.parametrize("kind", ["length", "dihedral"])
@pytest.mark.parametrize("name", list(MESHES))
def test_binary32_stays_within_the_derived_bounds(tmp_path, name, kind):
    pos, faces = MESHES[name]()
    L = er.Lists(tmp_path, faces, len(pos))
    got, want = er.forward(tmp_path, L, pos, kind), er.forward(tmp_path, L, pos, kind, np.float64)
    b = er.bound(tmp_path, L, pos, kind)
    err = np.abs(got.astype(np.float64) - want)
    some = b > 0
    print(f"{name} {kind}: max |out| {np.abs(want).max():.3e}, max err {err.max():.3e}, max err / bound "
          f"{(err[some] / b[some]).max() if some.any() else 0:.3f}, max bound {b.max():.3e}")
    assert np.isfinite(b).all() and (err <= b).all(), np.argwhere(err > b)[:4].tolist()
    assert b.max() <= 1e-5 * max(1.0, np.abs(want).max()), "the bound says nothing"
    gout = field(13, (len(faces), 3))
    got, want = er.backward(tmp_path, L, pos, kind, gout), er.backward(tmp_path, L, pos, kind, gout, np.float64)
    b = er.grad_bound(tmp_path, L, pos, kind, gout)
    err = np.abs(got.astype(np.float64) - want)
    some = b > 0
    print(f"{name} {kind} backward: max |gpos| {np.abs(want).max():.3e}, max err {err.max():.3e}, max err / bound "
          f"{(err[some] / b[some]).max() if some.any() else 0:.3f}, max bound {b.max():.3e}")
    assert np.isfinite(b).all() and (err <= b).all(), np.argwhere(err > b)[:4].tolist()
    # (the scale of DIHEDRAL's terms before they cancel: |s| <= 2 |gout| per entry, times 1 / |N| and the edge phase 2 crosses with)
    natural = (er.normals64(L, pos).R * er.entries(tmp_path, L).n.sum(1)).max() * 2 * np.abs(gout).max() * er._edge_vectors(L, pos)[1].max()
    assert b.max() <= 1e-4 * max(1.0, np.abs(want).max(), natural if kind == "dihedral" else 0.0), "the bound says nothing"
    # two sets in one call are the two calls
    two = er.backward(tmp_path, L, np.stack([pos, pos[::-1]]), kind, np.stack([gout, gout]))
    assert np.array_equal(two[0].view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("kind", ["length", "dihedral"])
def test_a_nan_position_reaches_its_faces_and_their_edge_neighbours_only(tmp_path, kind):
    pos, faces = vgkit.grid(6, 5, 8)
    L = er.Lists(tmp_path, faces, len(pos))
    at = 14  # (an interior vertex)
    own = (faces == at).any(1)
    pairs = er.pair_table(faces)
    near = own.copy()
    near[pairs[own[pairs[:, 2]], 0]] = True
    assert own.sum() >= 4 and near.sum() > own.sum() and not near.all()
    pos[at, 1] = np.nan
    out = er.forward(tmp_path, L, pos, kind)
    hit = np.isnan(out).any(1)
    assert not hit[~near].any()
    if kind == "length":  # an edge's length reads its two ends alone
        assert hit[own].all()
        assert np.array_equal(np.isnan(out), np.stack([(faces[:, [(j + 1) % 3, (j + 2) % 3]] == at).any(1) for j in range(3)], 1))
    else:  # a face whose normal is NaN is not ok: +0 on its own edges, skipped by its neighbours
        assert not hit.any() and not out[own].any() and (out[~near] > 0).any()
    gpos = er.backward(tmp_path, L, pos, kind, field(14, (len(faces), 3)))
    touched = np.zeros(len(pos), bool)
    touched[np.unique(faces[near])] = True
    assert np.isfinite(gpos[~touched]).all()


def test_a_zero_area_face_with_an_infinite_vertex_behind_it_contributes_nothing(tmp_path):
    """face 1 = (0, 1, 3) shares the edge (0, 1) with a good face 0 and is collinear — its cross product exactly zero —, and face 2 =
    (3, 3, 4) names an INFINITE vertex 4 behind it: both are skipped, never multiplied by zero.  DIHEDRAL of face 0 is that of the
    face alone (+0: no live neighbour) and its backward is finite; the count still sees face 1"""
    pos = np.float32([[0, 0, 0], [1, 1, 1], [0.25, 1, 0], [2, 2, 2], [np.inf, 0, 0]])
    faces = np.array([[0, 1, 2], [1, 0, 3], [3, 3, 4]], np.uint32)
    L = er.Lists(tmp_path, faces, 5)
    assert er.forward(tmp_path, L, None, "count")[:2, 2].tolist() == [2.0, 2.0]
    out = er.forward(tmp_path, L, pos, "dihedral")
    assert not out.view(np.uint32).any()
    gout = field(15, (3, 3))
    gpos = er.backward(tmp_path, L, pos, "dihedral", gout)
    assert not gpos[[0, 1, 2, 4]].view(np.uint32).any()  # (vertex 3: phase 2 crosses the infinite edge of ITS face with a zero G, as IEEE has it)
    # LENGTH: the edges to the infinite vertex are infinite and not live; the others' gradient is finite
    ln = er.forward(tmp_path, L, pos, "length")
    assert np.isinf(ln[2, :2]).all() and ln[2, 2] == 0 and np.isfinite(ln[:2]).all()
    assert np.isfinite(er.backward(tmp_path, L, pos, "length", gout)).all()
