"""-m gpu: vertex tangents and handedness on the device — srz_mesh_tangents (k_mesh_tangents), srz_mesh_tangents_grad
(k_mesh_tangents_grad) — and srz.visibility.mesh_tangents.  Expected values: tests/tangentref.py's binary32 build (the rules of
include/srz.h, pinned on the CPU by tests/test_tangent_ref.py), BIT FOR BIT — both passes are gathers without atomics; a NaN on one
side must be a NaN on the other (its sign and payload are the machine's)."""
import numpy as np
import pytest
import torch

import tangentref as tr
import vgkit
from srz import visibility as V
from support import SENTINEL, ctx, filled, stream, words  # noqa: F401

pytestmark = pytest.mark.gpu

SLOT, GUARD = 9, 5
# (mesh, the uv the test makes for it): one face; a fan around a hub of valence 70 (a corner list longer than a wave), uv independent
# of the positions (mirrored on about half the faces); 257 vertices (crosses the 256-thread block), sheared; 700 vertices, u folded
# back over the right half; a slot no face of which exists
MESHES = {"single": (vgkit.single, "affine"), "fan": (lambda: vgkit.fan(70, 2), "random"),
          "grid257": (lambda: vgkit.grid(16, 16, 3, extra=1), "sheared"), "grid700": (lambda: vgkit.grid(28, 25, 4), "folded"),
          "no-faces": (lambda: (vgkit.grid(3, 3, 5)[0], np.zeros((0, 3), np.uint32)), "affine")}


def i32(a):
    """a float32 / uint32 numpy array's words as an int32 tensor on the device"""
    return torch.as_tensor(np.ascontiguousarray(a).view(np.int32)).cuda()


def sets_of(name, n_sets):
    """(positions [n_sets, V, 3] float32 — set 0 the mesh lifted off its plane, the others jittered —, faces, uv [V, 2] with one
    degenerate uv face where there is a third face)"""
    make, kind = MESHES[name]
    pos, faces = make()
    pos = pos.copy()
    pos[:, 2] += (0.2 * np.sin(5.0 * pos[:, 0]) * np.cos(4.0 * pos[:, 1])).astype(np.float32)
    rng = np.random.default_rng([len(name), n_sets, 199])
    p = np.stack([pos] + [(pos + rng.uniform(-0.03, 0.03, pos.shape)).astype(np.float32) for _ in range(n_sets - 1)])
    uv = tr.make_uv(pos, kind, 3)
    if len(faces) > 2:
        uv = tr.degenerate_face(uv, faces, 2)
    return np.ascontiguousarray(p, np.float32), faces, uv


def upload(c, name, n_sets=1):
    """the slot's records carry set 0's positions and the uv"""
    p, faces, uv = sets_of(name, n_sets)
    v8 = vgkit.verts8(p[0])
    v8[:, 6:8] = uv
    c.mesh_upload(SLOT, v8, faces)
    return p, faces, uv


def differing(got_words, want):
    return tr.same_or_nan(np.ascontiguousarray(got_words).view(np.float32), want)


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """per (mesh, n_sets): positions, faces, uv, the gradient fed in, and the reference's tangents and gpos — computed once"""
    tmp = tmp_path_factory.mktemp("tangents")
    out = {}
    for name in MESHES:
        for n_sets in (1, 3):
            p, faces, uv = sets_of(name, n_sets)
            L = tr.Lists(tmp, faces, p.shape[1])
            g = np.random.default_rng([len(name), n_sets, 211]).uniform(-1, 1, p.shape[:2] + (4,)).astype(np.float32)
            out[(name, n_sets)] = dict(p=p, faces=faces, uv=uv, g=g, tan=tr.tangents(tmp, L, p, uv), gpos=tr.tangents_grad(tmp, L, p, uv, g),
                                       cls=tr.tangents_classify(tmp, L, p[0], uv))
    return out


def test_the_meshes_meet_every_branch(refs):
    """mirrored and unmirrored faces around one vertex, both handednesses, a degenerate uv face, a vertex no face names"""
    cls = refs[("fan", 1)]["cls"]
    assert ((cls & tr.NAMED) == 0).any()
    for name in ("fan", "grid700"):
        c = refs[(name, 1)]["cls"]
        assert (c & tr.W_NEG).any() and not (c & tr.W_NEG).all(), name
    r = refs[("grid700", 1)]
    assert ((r["cls"] & tr.NORMALISED) != 0).mean() > 0.95 and np.isfinite(r["gpos"]).all() and (r["gpos"] != 0).mean() > 0.95
    assert not refs[("no-faces", 1)]["tan"][..., :3].any() and (refs[("no-faces", 3)]["tan"][..., 3] == 1).all()


# ------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("n_sets", [1, 3])
@pytest.mark.parametrize("name", list(MESHES))
def test_tangents_against_the_reference(ctx, refs, name, n_sets):
    """packed (stride 4) into the middle of a buffer of sentinel words, on the ctx's stream and on a side stream; at a stride of 6 (the
    two floats behind every tangent and the guards untouched); with one set also from the slot's own positions and uv (null pointers)"""
    r = refs[(name, n_sets)]
    p, uv, want = r["p"], r["uv"], r["tan"]
    upload(ctx, name, n_sets)
    nv = p.shape[1]
    n = n_sets * nv * 4
    d_pos, d_uv = i32(p), i32(uv)
    side = torch.cuda.Stream()
    for st in (None, stream(), side.cuda_stream):
        buf = filled((n + 2 * GUARD,))
        torch.cuda.synchronize()
        ctx.mesh_tangents(SLOT, d_pos.data_ptr(), 3, n_sets, d_uv.data_ptr(), 2, buf.data_ptr() + 4 * GUARD, 4, st)
        if st is None:
            ctx.sync()  # (the ctx's own stream)
        torch.cuda.synchronize()
        w = words(buf)
        bad = differing(w[GUARD:GUARD + n].reshape(want.shape), want)
        assert not bad.any(), (name, n_sets, st, np.argwhere(bad)[:4].tolist())
        assert (w[:GUARD] == SENTINEL).all() and (w[GUARD + n:] == SENTINEL).all()
    packed = w[GUARD:GUARD + n].reshape(n_sets * nv, 4)
    rec = filled((GUARD + n_sets * nv * 6 + GUARD,))
    torch.cuda.synchronize()
    ctx.mesh_tangents(SLOT, d_pos.data_ptr(), 3, n_sets, d_uv.data_ptr(), 2, rec.data_ptr() + 4 * GUARD, 6, stream())
    torch.cuda.synchronize()
    w = words(rec)
    body = w[GUARD:GUARD + n_sets * nv * 6].reshape(n_sets * nv, 6)
    assert np.array_equal(body[:, :4], packed) and (body[:, 4:] == SENTINEL).all()
    assert (w[:GUARD] == SENTINEL).all() and (w[-GUARD:] == SENTINEL).all()
    # uv at a stride of 5 behind one float of padding; positions in records of 8
    uv5 = filled((nv, 5))
    uv5[:, 1:3] = d_uv.view(nv, 2)
    p8 = filled((n_sets * nv, 8))
    p8[:, 0:3] = d_pos.view(-1, 3)
    out = filled((n,))
    torch.cuda.synchronize()
    ctx.mesh_tangents(SLOT, p8.data_ptr(), 8, n_sets, uv5.data_ptr() + 4, 5, out.data_ptr(), 4, stream())
    torch.cuda.synchronize()
    assert np.array_equal(words(out).reshape(-1, 4), packed)
    if n_sets == 1:
        for a, b in ((None, d_uv.data_ptr()), (d_pos.data_ptr(), None), (None, None)):
            own = filled((n,))
            torch.cuda.synchronize()
            ctx.mesh_tangents(SLOT, a, 3 if a else 0, 1, b, 2 if b else 0, own.data_ptr(), 4, stream())
            torch.cuda.synchronize()
            assert np.array_equal(words(own).reshape(-1, 4), packed), (name, a is None, b is None)


# ------------------------------------------------------------------------------------------------------ backward
def grad_call(c, d_pos, pos_stride, n_sets, d_uv, uv_stride, d_g, g_stride, n, st=None):
    """one srz_mesh_tangents_grad into the middle of a buffer of sentinel words -> (gpos words [n], guard words before, after)"""
    buf, work = filled((n + 2 * GUARD,)), filled((n,))
    torch.cuda.synchronize()
    c.mesh_tangents_grad(SLOT, d_pos, pos_stride, n_sets, d_uv, uv_stride, d_g, g_stride, work.data_ptr(), buf.data_ptr() + 4 * GUARD,
                         stream() if st is None else st)
    torch.cuda.synchronize()
    w = words(buf)
    return w[GUARD:GUARD + n], w[:GUARD], w[GUARD + n:]


@pytest.mark.parametrize("n_sets", [1, 3])
@pytest.mark.parametrize("name", list(MESHES))
def test_tangents_grad_against_the_reference(ctx, refs, name, n_sets):
    """every element of d_gpos written (no sentinel left), the guards intact, two runs bit-equal, on a side stream too; the gradient of
    the tangents once packed and once in records of six floats with NaN in w (never read); with one set also from the slot's own
    positions and uv"""
    r = refs[(name, n_sets)]
    p, uv, g, want = r["p"], r["uv"], r["g"], r["gpos"]
    upload(ctx, name, n_sets)
    n = p.size
    d_pos, d_uv, d_g = i32(p), i32(uv), i32(g)
    got, before, after = grad_call(ctx, d_pos.data_ptr(), 3, n_sets, d_uv.data_ptr(), 2, d_g.data_ptr(), 4, n)
    bad = differing(got.reshape(p.shape), want)
    assert not bad.any(), (name, n_sets, np.argwhere(bad)[:4].tolist())
    assert not (got == SENTINEL).any()
    assert (before == SENTINEL).all() and (after == SENTINEL).all()
    side = torch.cuda.Stream()
    again, _, _ = grad_call(ctx, d_pos.data_ptr(), 3, n_sets, d_uv.data_ptr(), 2, d_g.data_ptr(), 4, n, side.cuda_stream)
    assert np.array_equal(again, got), "two runs differ"
    g6 = filled((p.shape[0] * p.shape[1], 6))
    g6[:, 1:4] = d_g.view(-1, 4)[:, 0:3]
    g6[:, 4] = i32(np.full(1, np.nan, np.float32))[0]
    strided, _, _ = grad_call(ctx, d_pos.data_ptr(), 3, n_sets, d_uv.data_ptr(), 2, g6.data_ptr() + 4, 6, n)
    assert np.array_equal(strided, got)
    if n_sets == 1:
        own, _, _ = grad_call(ctx, None, 0, 1, None, 0, d_g.data_ptr(), 4, n)
        assert np.array_equal(own, got)


@pytest.mark.parametrize("batched", [False, True])
def test_autograd_is_the_plain_call(ctx, refs, batched):
    """mesh_tangents(ctx, slot, pos, uv) returns the reference's tangents [.., 4]; backward gives pos.grad = the plain call's d_gpos;
    uv None takes the slot's own"""
    n_sets = 3 if batched else 1
    r = refs[("fan", n_sets)]
    upload(ctx, "fan", n_sets)
    p = r["p"] if batched else r["p"][0]
    g = r["g"] if batched else r["g"][0]
    for uv in (torch.as_tensor(r["uv"]).cuda(), None):
        pos = torch.as_tensor(p).cuda().requires_grad_(True)
        tan = V.mesh_tangents(ctx, SLOT, pos, uv)
        assert tan.shape == pos.shape[:-1] + (4,) and not differing(words(tan.detach()), r["tan"].reshape(tan.shape)).any()
        tan.backward(torch.as_tensor(g).cuda())
        torch.cuda.synchronize()
        assert not differing(words(pos.grad), r["gpos"].reshape(p.shape)).any()
    with pytest.raises(ValueError):
        V.mesh_tangents(ctx, SLOT, pos[..., :2])
    with pytest.raises(ValueError):
        V.mesh_tangents(ctx, SLOT, pos, torch.zeros((3, 2), device="cuda"))
