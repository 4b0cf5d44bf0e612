"""-m gpu: the mesh edge terms on the device — srz_mesh_edges and srz_mesh_edges_grad (k_mesh_edges, k_mesh_edges_grad).  Expected
values: tests/edgeref.py's binary32 functions (the rules of include/srz.h, pinned on the CPU by tests/test_edge_ref.py), BIT FOR BIT —
both passes are gathers without atomics; a NaN on one side must be a NaN on the other (its sign and payload are the machine's).  The
meshes are the smallest on which each branch can go wrong: boundary edges only (single), one shared edge wound both ways (pair), a
non-manifold edge whose sum has an order (book), a closed mesh (octa), a hub list longer than a wave with a degenerate face and a
vertex no face names (fan), more than one block of faces and of vertices (grid257: 451 and 257), a face of zero area (flat)."""
import numpy as np
import pytest
import torch

import edgeref as er
import normalsref as nr
import vgkit
from srz import abi
from srz import visibility as V
from support import SENTINEL, ctx, filled, stream, words  # noqa: F401

pytestmark = pytest.mark.gpu

SLOT, GUARD = 9, 5
KINDS = (abi.EDGE_COUNT, abi.EDGE_LENGTH, abi.EDGE_DIHEDRAL)
MESHES = er.meshes()


def i32(a):
    """a float32 / uint32 numpy array's words as an int32 tensor on the device"""
    return torch.as_tensor(np.ascontiguousarray(a).view(np.int32)).cuda()


def differing(got_words, want):
    return nr.same_or_nan(np.ascontiguousarray(got_words).view(np.float32), want)


def sets_of(pos, n_sets, seed):
    """n_sets position sets [n_sets, V, 3]: the mesh's own, then copies moved a little"""
    rng = np.random.default_rng([seed, 233])
    return np.stack([pos] + [(pos + rng.uniform(-0.01, 0.01, pos.shape)).astype(np.float32) for _ in range(n_sets - 1)]).astype(np.float32)


def guarded(n):
    """a buffer of n words between guards, all sentinel -> (tensor, address of word 0)"""
    buf = filled((n + 2 * GUARD,))
    return buf, buf.data_ptr() + 4 * GUARD


def inner(buf, n):
    """the n words between the guards, which are checked"""
    w = words(buf)
    assert (w[:GUARD] == SENTINEL).all() and (w[GUARD + n:] == SENTINEL).all(), "a guard word was written"
    return w[GUARD:GUARD + n]


def forward_packed(c, d_pos, n_sets, kind, n_faces, st=None):
    buf, at = guarded(n_sets * n_faces * 3)
    torch.cuda.synchronize()
    c.mesh_edges(SLOT, d_pos, 3, n_sets, kind, at, 3, stream() if st is None else st)
    torch.cuda.synchronize()
    return inner(buf, n_sets * n_faces * 3).reshape(n_sets, n_faces, 3)


def forward_strided(c, p, kind, n_faces):
    """positions in records of 5 floats (from float 1), the output in records of 6 (from float 2), all sentinel-filled"""
    n_sets, nv, _ = p.shape
    pin = filled((n_sets * nv, 5))
    pin[:, 1:4] = i32(p).view(-1, 3)
    buf, at = guarded(n_sets * n_faces * 6)
    torch.cuda.synchronize()
    c.mesh_edges(SLOT, pin.data_ptr() + 4, 5, n_sets, kind, at + 8, 6, stream())
    torch.cuda.synchronize()
    r = inner(buf, n_sets * n_faces * 6).reshape(n_sets, n_faces, 6)
    assert (r[:, :, :2] == SENTINEL).all() and (r[:, :, 5:] == SENTINEL).all(), "a record's other floats were written"
    pi = words(pin)
    assert (pi[:, 0] == SENTINEL).all() and (pi[:, 4] == SENTINEL).all() and np.array_equal(pi[:, 1:4].reshape(p.shape), p.view(np.uint32))
    return r[:, :, 2:5]


def backward_packed(c, d_pos, n_sets, kind, d_gout, n_verts, n_faces, st=None, strided_gout=False):
    """-> gpos' words [n_sets, n_verts, 3]; the workspace (DIHEDRAL; LENGTH gets none) and the output sit between guards"""
    gbuf, gat = guarded(n_sets * n_verts * 3)
    wbuf, wat = guarded(max(1, n_sets * n_faces * 3))
    torch.cuda.synchronize()
    c.mesh_edges_grad(SLOT, d_pos, 3, n_sets, kind, d_gout + (4 if strided_gout else 0), 5 if strided_gout else 3,
                      wat if kind == abi.EDGE_DIHEDRAL else None, gat, stream() if st is None else st)
    torch.cuda.synchronize()
    inner(wbuf, max(1, n_sets * n_faces * 3))
    return inner(gbuf, n_sets * n_verts * 3).reshape(n_sets, n_verts, 3)


@pytest.mark.parametrize("n_sets", [1, 3])
@pytest.mark.parametrize("name", list(MESHES))
def test_edges_against_the_reference(ctx, tmp_path, name, n_sets):
    """every kind, forward and backward: packed and strided, bit for bit; two launches bit-equal"""
    pos, faces = MESHES[name]()
    ctx.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    nv, nf = len(pos), len(faces)
    L = er.Lists(tmp_path, faces, nv)
    p = sets_of(pos, n_sets, len(name))
    d_p = i32(p)
    gout = np.random.default_rng([len(name), n_sets, 239]).uniform(-1, 1, (n_sets, nf, 3)).astype(np.float32)
    d_gout = i32(gout)
    gin = filled((n_sets * nf, 5))
    gin[:, 1:4] = d_gout.view(-1, 3)
    for kind in KINDS:
        what = (name, n_sets, kind)
        if kind == abi.EDGE_COUNT:
            if n_sets != 1:
                continue
            want = er.forward(tmp_path, L, None, kind)[None]
        else:
            want = er.forward(tmp_path, L, p, kind)
        fwd = forward_packed(ctx, d_p.data_ptr(), n_sets, kind, nf)
        bad = differing(fwd, want)
        assert not bad.any(), (what, "forward", np.argwhere(bad)[:4].tolist())
        assert np.array_equal(forward_packed(ctx, d_p.data_ptr(), n_sets, kind, nf), fwd), (what, "two runs")
        assert np.array_equal(forward_strided(ctx, p, kind, nf), fwd), (what, "strided")
        if kind == abi.EDGE_COUNT:
            continue
        want = er.backward(tmp_path, L, p, kind, gout)
        bwd = backward_packed(ctx, d_p.data_ptr(), n_sets, kind, d_gout.data_ptr(), nv, nf)
        bad = differing(bwd, want)
        assert not bad.any(), (what, "backward", np.argwhere(bad)[:4].tolist())
        assert np.array_equal(backward_packed(ctx, d_p.data_ptr(), n_sets, kind, d_gout.data_ptr(), nv, nf), bwd), (what, "two runs")
        assert np.array_equal(backward_packed(ctx, d_p.data_ptr(), n_sets, kind, gin.data_ptr(), nv, nf, strided_gout=True), bwd), (what, "strided")
        if name in ("octa", "grid257", "book"):
            assert np.isfinite(want).all() and (want != 0).any(axis=2).mean() > 0.9, "the test shows nothing"
    gi = words(gin)
    assert (gi[:, 0] == SENTINEL).all() and (gi[:, 4] == SENTINEL).all()


def test_a_slot_with_no_faces(ctx):
    """not an error: the forward launches nothing (the buffer keeps its words), the backward writes zeros to gpos"""
    pos = vgkit.grid(3, 3, 5)[0]
    ctx.mesh_upload(SLOT, vgkit.verts8(pos), np.zeros((0, 3), np.uint32))
    d_p, d_g = i32(pos), filled((8,))
    for kind in KINDS:
        buf, at = guarded(4)
        ctx.mesh_edges(SLOT, d_p.data_ptr(), 3, 1, kind, at, 3, stream())
        torch.cuda.synchronize()
        assert (inner(buf, 4) == SENTINEL).all()
        if kind != abi.EDGE_COUNT:
            assert not backward_packed(ctx, d_p.data_ptr(), 1, kind, d_g.data_ptr(), len(pos), 0).any()


def test_on_a_side_stream(ctx, tmp_path):
    pos, faces = MESHES["grid257"]()
    ctx.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    L = er.Lists(tmp_path, faces, len(pos))
    p = sets_of(pos, 2, 241)
    gout = np.random.default_rng(251).uniform(-1, 1, (2, len(faces), 3)).astype(np.float32)
    d_p, d_gout = i32(p), i32(gout)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for kind in (abi.EDGE_LENGTH, abi.EDGE_DIHEDRAL):
        got = forward_packed(ctx, d_p.data_ptr(), 2, kind, len(faces), side.cuda_stream)
        assert not differing(got, er.forward(tmp_path, L, p, kind)).any(), kind
        got = backward_packed(ctx, d_p.data_ptr(), 2, kind, d_gout.data_ptr(), len(pos), len(faces), side.cuda_stream)
        assert not differing(got, er.backward(tmp_path, L, p, kind, gout)).any(), kind
    got = forward_packed(ctx, None, 1, abi.EDGE_COUNT, len(faces), side.cuda_stream)
    assert np.array_equal(got.view(np.float32)[0], er.forward(tmp_path, L, None, "count"))


def test_the_null_form_is_the_slots_own_positions(ctx, tmp_path):
    """after mesh_update: a null d_pos is the moved positions (stride 8 inside the records), forward and backward — and not the
    positions the slot was uploaded with"""
    pos, faces = MESHES["grid257"]()
    ctx.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    L = er.Lists(tmp_path, faces, len(pos))
    moved = (pos + np.random.default_rng(257).uniform(-0.02, 0.02, pos.shape)).astype(np.float32)
    V.mesh_update(ctx, SLOT, torch.as_tensor(vgkit.verts8(moved)).cuda())
    d_moved = i32(moved)
    gout = np.random.default_rng(263).uniform(-1, 1, (len(faces), 3)).astype(np.float32)
    d_gout = i32(gout)
    for kind in (abi.EDGE_LENGTH, abi.EDGE_DIHEDRAL):
        own = forward_packed(ctx, None, 1, kind, len(faces))
        assert not differing(own[0], er.forward(tmp_path, L, moved, kind)).any(), kind
        assert np.array_equal(forward_packed(ctx, d_moved.data_ptr(), 1, kind, len(faces)), own), kind
        assert differing(own[0], er.forward(tmp_path, L, pos, kind)).any(), "the test shows nothing"
        back = backward_packed(ctx, None, 1, kind, d_gout.data_ptr(), len(pos), len(faces))
        assert not differing(back[0], er.backward(tmp_path, L, moved, kind, gout)).any(), kind
        assert np.array_equal(backward_packed(ctx, d_moved.data_ptr(), 1, kind, d_gout.data_ptr(), len(pos), len(faces)), back), kind


def test_hand_written_values(ctx, tmp_path):
    """a 5 x 4 grid in seven position sets of one call — all zeros, subnormal coordinates, coordinates whose squares are subnormal, huge
    ones whose products overflow, an infinite vertex, a NaN vertex, a -0 and a 1e-45 — the reference's bits in both directions, and
    every non-finite output is at a face that names such a vertex, at one across an edge from it, or (gpos) at their vertices"""
    pos, faces = vgkit.grid(5, 4, 11)
    ctx.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    nv, nf = len(pos), len(faces)
    L = er.Lists(tmp_path, faces, nv)
    p = np.stack([pos] * 7).astype(np.float32)
    p[0] = 0.0
    p[1] *= np.float32(1e-41)
    p[2] *= np.float32(1e-20)
    p[3] *= np.float32(3e37)
    p[4, 6, 0], p[4, 13, 2] = np.inf, -np.inf
    p[5, 7, 1] = np.nan
    p[6, 0], p[6, 19, 2] = -0.0, np.float32(1e-45)
    assert (np.abs(p[1]) < np.finfo(np.float32).tiny).all() and p[1].any()
    hot = {4: [6, 13], 5: [7]}
    gout = np.random.default_rng(269).uniform(-1, 1, (7, nf, 3)).astype(np.float32)
    d_p, d_gout = i32(p), i32(gout)
    pairs = er.pair_table(faces)
    for kind in (abi.EDGE_LENGTH, abi.EDGE_DIHEDRAL):
        fwd = forward_packed(ctx, d_p.data_ptr(), 7, kind, nf)
        bad = differing(fwd, er.forward(tmp_path, L, p, kind))
        assert not bad.any(), (kind, "forward", np.argwhere(bad)[:4].tolist())
        bwd = backward_packed(ctx, d_p.data_ptr(), 7, kind, d_gout.data_ptr(), nv, nf)
        bad = differing(bwd, er.backward(tmp_path, L, p, kind, gout))
        assert not bad.any(), (kind, "backward", np.argwhere(bad)[:4].tolist())
        f, g = fwd.view(np.float32), bwd.view(np.float32)
        assert not fwd[0].any() and not bwd[0].any(), "a mesh of zeros does not give +0 everywhere"
        assert np.isfinite(f[[0, 1, 2, 6]]).all() and np.isfinite(g[[0, 1, 2, 6]]).all()
        if kind == abi.EDGE_LENGTH:
            # (subnormal coordinates: the squares underflow, every length is +0 and no edge is live; squares that are subnormal: a
            # length per edge; huge coordinates: the squares overflow, every length is inf and no edge is live)
            assert not fwd[1].any() and not bwd[1].any() and f[2].all() and g[2].any() and np.isinf(f[3]).all() and not bwd[3].any()
        for s, at in hot.items():
            own = np.isin(faces, at).any(1)
            near = own.copy()
            near[pairs[own[pairs[:, 2]], 0]] = True
            touched = np.zeros(nv, bool)
            touched[np.unique(faces[near])] = True
            assert np.isfinite(f[s][~near]).all() and np.isfinite(g[s][~touched]).all(), (kind, s)
            if kind == abi.EDGE_LENGTH:
                assert not np.isfinite(f[s][own]).all(axis=1).any(), (kind, s)
