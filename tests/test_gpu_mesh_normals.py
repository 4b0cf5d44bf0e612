"""-m gpu: vertex normals on the device — srz_mesh_normals (k_mesh_normals), srz_mesh_normals_grad (k_mesh_normals_grad) — and
srz.visibility.mesh_normals / refresh_normals.  Expected values: tests/normalsref.py (the rules of include/srz.h, pinned on the CPU by
tests/test_normals_ref.py), BIT FOR BIT — both passes are gathers without atomics; a NaN on one side must be a NaN on the other (its
sign and payload are the machine's).  The in-place form is held end to end: a PHONG render and the G-buffer's normals of a live
sceneset after mesh_update + refresh_normals equal the oracle's render and tests/gbufref.py's planes of the mesh carrying the
reference's normals."""
import numpy as np
import pytest
import torch

import gbufref
import normalsref as nr
import srz
import vgkit
from srz import abi
from srz import visibility as V
from support import SENTINEL, ctx, filled, same, scene_pair, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

W = H = 64
SLOT, GUARD = 7, 5
IDENT = np.eye(4, dtype=np.float32).reshape(16)
MESHES = {"single": vgkit.single, "fan": lambda: vgkit.fan(70, 2), "grid257": lambda: vgkit.grid(16, 16, 3, extra=1),
          "grid700": lambda: vgkit.grid(28, 25, 4), "edge": lambda: nr.edge_mesh()[:2],
          "no-faces": lambda: (vgkit.grid(3, 3, 5)[0], np.zeros((0, 3), np.uint32))}


def i32(a):
    """a float32 / uint32 numpy array's words as an int32 tensor on the device"""
    return torch.as_tensor(np.ascontiguousarray(a).view(np.int32)).cuda()


def sets_of(name, n_sets):
    """(positions [n_sets, V, 3] float32 — set 0 the mesh as made, the others jittered —, faces)"""
    pos, faces = MESHES[name]()
    rng = np.random.default_rng([len(name), n_sets, 149])
    p = np.stack([pos] + [(pos + rng.uniform(-0.03, 0.03, pos.shape) * (np.abs(pos) < 1e3)).astype(np.float32) for _ in range(n_sets - 1)])
    return np.ascontiguousarray(p, np.float32), faces


def upload(c, name, n_sets=1):
    p, faces = sets_of(name, n_sets)
    c.mesh_upload(SLOT, vgkit.verts8(p[0]), faces)
    return p, faces


def differing(got_words, want):
    return nr.same_or_nan(np.ascontiguousarray(got_words).view(np.float32), want)


# ------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("n_sets", [1, 3])
@pytest.mark.parametrize("name", list(MESHES))
def test_normals_against_the_reference(ctx, tmp_path, name, n_sets):
    """packed (stride 3) into the middle of a buffer of sentinel words, once more on a non-default stream; then the interleaved record
    form d_nrm = d_pos + 3, strides 8: floats 3..5 of every record are the normals, the positions, floats 6..7 and the guard words
    before and after are untouched"""
    p, faces = upload(ctx, name, n_sets)
    nv = p.shape[1]
    want = nr.normals(tmp_path, nr.Lists(tmp_path, faces, nv), p)
    if name in ("no-faces",):
        assert not want.any()
    n = n_sets * nv * 3
    d_pos = i32(p)
    side = torch.cuda.Stream()
    for st in (None, side.cuda_stream):
        buf = filled((n + 2 * GUARD,))
        torch.cuda.synchronize()
        ctx.mesh_normals(SLOT, d_pos.data_ptr(), 3, n_sets, buf.data_ptr() + 4 * GUARD, 3, stream() if st is None else st)
        torch.cuda.synchronize()
        w = words(buf)
        bad = differing(w[GUARD:GUARD + n].reshape(p.shape), want)
        assert not bad.any(), (name, n_sets, st, np.argwhere(bad)[:4].tolist())
        assert (w[:GUARD] == SENTINEL).all() and (w[GUARD + n:] == SENTINEL).all()
    rec = filled((GUARD + n_sets * nv * 8 + GUARD,))
    body = rec[GUARD:GUARD + n_sets * nv * 8].view(n_sets * nv, 8)
    body[:, 0:3] = d_pos.view(-1, 3)
    base = rec.data_ptr() + 4 * GUARD
    torch.cuda.synchronize()
    ctx.mesh_normals(SLOT, base, 8, n_sets, base + 12, 8, stream())
    torch.cuda.synchronize()
    w = words(rec)
    r = w[GUARD:GUARD + n_sets * nv * 8].reshape(n_sets, nv, 8)
    assert not differing(r[:, :, 3:6], want).any(), (name, n_sets, "records")
    assert np.array_equal(r[:, :, 0:3], p.view(np.uint32)) and (r[:, :, 6:8] == SENTINEL).all()
    assert (w[:GUARD] == SENTINEL).all() and (w[-GUARD:] == SENTINEL).all()


def test_refresh_renders_the_normals_of_the_moved_mesh(ctx, tmp_path, orc):
    """mesh_update with moved vertices (their records carry the OLD flat normals), refresh_normals, then the live set's PHONG render and
    its G-buffer's normals: bit-identical to the oracle's render and the G-buffer reference's planes of the moved mesh carrying
    normalsref's normals — and not to the render before the refresh"""
    pos, faces = vgkit.grid(16, 16, 3, extra=1)
    m = vgkit.perspective(50.0, 46.0, 5.0, 6.0)
    faces = vgkit.oriented(pos, faces, m)
    lights = [[[-20.0, -15.0, 300.0], [14.0, 14.0, 14.0]], [[89.0, 10.0, 250.0], [9.0, 9.0, 9.0]], [[32.0, 70.0, -300.0], [11.0, 11.0, 11.0]]]
    eye = (0.0, 0.0, 1.0)  # (vgkit.oriented's eye: the winding that survives the cull)
    pair = lambda v8, c=None: scene_pair([(v8, faces, abi.SHADER_PHONG, -1, m, IDENT)], W, H, eye, lights, 1.75, 0.5, ctx=c, slots=[SLOT])  # noqa: E731
    sframe, _ = pair(vgkit.verts8(pos), ctx)
    fs = ctx.frameset([sframe])
    moved = (pos + np.random.default_rng(151).uniform(-0.02, 0.02, pos.shape)).astype(np.float32)
    moved[:, 2] = (moved[:, 2] + 0.3 * np.sin(6.0 * moved[:, 0])).astype(np.float32)  # (a wave: normals that tilt)
    out = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")

    def render():
        out.fill_(-1.0)
        fs.render(out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
        torch.cuda.synchronize()
        return out[0].cpu().numpy()
    V.mesh_update(ctx, SLOT, torch.as_tensor(vgkit.verts8(moved)).cuda())
    stale = render()
    V.refresh_normals(ctx, SLOT)
    got = render()
    v8 = vgkit.verts8(moved)
    v8[:, 3:6], mask = nr.normals(tmp_path, nr.Lists(tmp_path, faces, len(pos)), moved, want_mask=True)
    assert mask.all()
    _, f = pair(v8)
    rc, ref, _ = orc.draw(f)
    assert rc == 0
    same(got, ref, "PHONG render after refresh_normals")
    assert not np.array_equal(stale[1:], got[1:]), "the refresh changed no colour: the test shows nothing"
    vis = visibility(fs)
    gb = torch.zeros(fs.gbuffer_shape(abi.GB_NORMAL), dtype=torch.float32, device="cuda")
    fs.gbuffer(vis.data_ptr(), gb.data_ptr(), fs.gbuffer_bytes(abi.GB_NORMAL), abi.GB_NORMAL, abi.FUSED_CLEAR, stream())
    torch.cuda.synchronize()
    want = gbufref.expected(tmp_path, f, {}, words(vis)[0])[gbufref.planes_of(abi.GB_NORMAL)]
    assert (words(vis)[0, 1] != 0).sum() > 500
    assert not differing(words(gb)[0], want.view(np.float32)).any(), "G-buffer normals after refresh_normals"
    fs.close()


# ------------------------------------------------------------------------------------------------------ backward
def grad_call(c, d_pos, pos_stride, n_sets, d_gnrm, gnrm_stride, n):
    """one srz_mesh_normals_grad into the middle of a buffer of sentinel words -> (gpos words [n], guard words before, after)"""
    buf, work = filled((n + 2 * GUARD,)), filled((n,))
    torch.cuda.synchronize()
    c.mesh_normals_grad(SLOT, d_pos, pos_stride, n_sets, d_gnrm, gnrm_stride, work.data_ptr(), buf.data_ptr() + 4 * GUARD, stream())
    torch.cuda.synchronize()
    w = words(buf)
    return w[GUARD:GUARD + n], w[:GUARD], w[GUARD + n:]


@pytest.mark.parametrize("n_sets", [1, 3])
@pytest.mark.parametrize("name", list(MESHES))
def test_normals_grad_against_the_reference(ctx, tmp_path, name, n_sets):
    """every element of d_gpos, the guards intact, two runs bit-equal; the gradient of the normals once packed and once in records of
    five floats; with one set also from the slot's own vertices (a null d_pos)"""
    p, faces = upload(ctx, name, n_sets)
    nv, n = p.shape[1], p.size
    g = np.random.default_rng([len(name), n_sets, 157]).uniform(-1, 1, p.shape).astype(np.float32)
    want = nr.normals_grad(tmp_path, nr.Lists(tmp_path, faces, nv), p, g)
    if name == "grid700":
        assert np.isfinite(want).all() and (want != 0).all()
    d_pos, d_g = i32(p), i32(g)
    got, before, after = grad_call(ctx, d_pos.data_ptr(), 3, n_sets, d_g.data_ptr(), 3, n)
    bad = differing(got.reshape(p.shape), want)
    assert not bad.any(), (name, n_sets, np.argwhere(bad)[:4].tolist())
    assert (before == SENTINEL).all() and (after == SENTINEL).all()
    again, _, _ = grad_call(ctx, d_pos.data_ptr(), 3, n_sets, d_g.data_ptr(), 3, n)
    assert np.array_equal(again, got), "two runs differ"
    g5 = filled((n_sets * nv, 5))
    g5[:, 1:4] = d_g.view(-1, 3)
    strided, _, _ = grad_call(ctx, d_pos.data_ptr(), 3, n_sets, g5.data_ptr() + 4, 5, n)
    assert np.array_equal(strided, got)
    if n_sets == 1:
        own, _, _ = grad_call(ctx, None, 0, 1, d_g.data_ptr(), 3, n)
        assert np.array_equal(own, got)


@pytest.mark.parametrize("batched", [False, True])
def test_autograd_is_the_plain_call(ctx, tmp_path, batched):
    """mesh_normals(ctx, slot, pos) returns the reference's normals in pos's shape; backward gives pos.grad = the plain call's d_gpos"""
    p, faces = upload(ctx, "fan", 3 if batched else 1)
    L = nr.Lists(tmp_path, faces, p.shape[1])
    p = p if batched else p[0]
    g = np.random.default_rng(163).uniform(-1, 1, p.shape).astype(np.float32)
    pos = torch.as_tensor(p).cuda().requires_grad_(True)
    nrm = V.mesh_normals(ctx, SLOT, pos)
    assert nrm.shape == pos.shape and not differing(words(nrm.detach()), nr.normals(tmp_path, L, p)).any()
    nrm.backward(torch.as_tensor(g).cuda())
    torch.cuda.synchronize()
    assert not differing(words(pos.grad), nr.normals_grad(tmp_path, L, p, g)).any()
    with pytest.raises(ValueError):
        V.mesh_normals(ctx, SLOT, pos[..., :2])


# ------------------------------------------------------------------------------------------------------ refusals
def refused(fn_name, fn, *untouched):
    """fn() raises SRZ_E_INVALID naming fn_name; every tensor of `untouched` still holds the sentinel"""
    with pytest.raises(srz.SrzError) as e:
        fn()
    assert e.value.code == abi.SRZ_E_INVALID and fn_name in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for t in untouched:
        assert (words(t) == SENTINEL).all(), fn_name + ": an output was written"


def test_refusals(ctx):
    """every SRZ_E_INVALID of the two entry points: nothing launched, the outputs keep the sentinel"""
    p, faces = upload(ctx, "fan", 2)
    nv = p.shape[1]
    L = srz.lib()
    vp = srz.C.c_void_p
    pos, out, work, g = i32(p), filled((2 * nv * 8,)), filled((2 * nv * 3,)), i32(p)
    a, o, wk, gg, s = pos.data_ptr(), out.data_ptr(), work.data_ptr(), g.data_ptr(), stream()
    name = "srz_mesh_normals"
    fwd = ctx.mesh_normals
    assert L.srz_mesh_normals(None, SLOT, vp(a), 3, 1, vp(o), 3, None) == abi.SRZ_E_INVALID
    for slot in (-1, 256, 200):                                                       # a bad id, an empty slot
        refused(name, lambda slot=slot: fwd(slot, a, 3, 1, o, 3, s), out)
    for n_sets in (0, 65536):
        refused(name, lambda n_sets=n_sets: fwd(SLOT, a, 3, n_sets, o, 3, s), out)
    refused(name, lambda: fwd(SLOT, a, 2, 1, o, 3, s), out)                           # a stride below 3
    refused(name, lambda: fwd(SLOT, a, 3, 1, o, 2, s), out)
    refused(name, lambda: fwd(SLOT, None, 8, 2, o, 3, s), out)                        # the slot's own vertices are one set
    refused(name, lambda: fwd(SLOT, a, 3, 2, None, 8, s), out)                        # and so are its own normals
    refused(name, lambda: fwd(SLOT, None, 8, 2, None, 8, s), out)
    refused(name, lambda: fwd(SLOT, a + 2, 3, 1, o, 3, s), out)                       # a misaligned pointer
    refused(name, lambda: fwd(SLOT, a, 3, 1, o + 2, 3, s), out)
    refused(name, lambda: fwd(SLOT, o, 3, 2, o + 4 * (2 * nv * 3 - 1), 3, s), out)    # the normals' span reaches into the positions'
    refused(name, lambda: fwd(SLOT, o + 4 * 8, 3, 2, o, 8, s), out)
    refused(name, lambda: fwd(SLOT, o, 5, 2, o + 12, 5, s), out)                      # records too short for pos3 + nrm3
    refused(name, lambda: fwd(SLOT, o, 8, 2, o + 12, 7, s), out)                      # records of two strides
    refused(name, lambda: fwd(SLOT, o, 8, 2, o + 8, 8, s), out)                       # normals over the positions' z
    name = "srz_mesh_normals_grad"
    bwd = ctx.mesh_normals_grad
    gp = filled((2 * nv * 3,))
    q = gp.data_ptr()
    assert L.srz_mesh_normals_grad(None, SLOT, vp(a), 3, 1, vp(gg), 3, vp(wk), vp(q), None) == abi.SRZ_E_INVALID
    for slot in (-1, 256, 200):
        refused(name, lambda slot=slot: bwd(slot, a, 3, 1, gg, 3, wk, q, s), work, gp)
    for n_sets in (0, 65536):
        refused(name, lambda n_sets=n_sets: bwd(SLOT, a, 3, n_sets, gg, 3, wk, q, s), work, gp)
    refused(name, lambda: bwd(SLOT, a, 2, 1, gg, 3, wk, q, s), work, gp)
    refused(name, lambda: bwd(SLOT, a, 3, 1, gg, 2, wk, q, s), work, gp)
    refused(name, lambda: bwd(SLOT, None, 8, 2, gg, 3, wk, q, s), work, gp)
    for nulls in ((None, wk, q), (gg, None, q), (gg, wk, None)):                       # a null required buffer
        refused(name, lambda nulls=nulls: bwd(SLOT, a, 3, 1, *nulls[:1], 3, *nulls[1:], s), work, gp)
    for bad in ((a + 2, gg, wk, q), (a, gg + 2, wk, q), (a, gg, wk + 2, q), (a, gg, wk, q + 2)):
        refused(name, lambda bad=bad: bwd(SLOT, bad[0], 3, 1, bad[1], 3, bad[2], bad[3], s), work, gp)
    big = filled((4 * 2 * nv * 3,))
    b, span = big.data_ptr(), 4 * 2 * nv * 3
    refused(name, lambda: bwd(SLOT, b, 3, 2, gg, 3, wk, b + span - 4, s), big, work)              # gpos overlaps the positions
    refused(name, lambda: bwd(SLOT, b, 3, 2, gg, 3, b + span - 4, q, s), big, gp)                 # the workspace does
    refused(name, lambda: bwd(SLOT, a, 3, 2, b, 3, wk, b + span - 4, s), big, work)               # gpos overlaps the normals' gradient
    refused(name, lambda: bwd(SLOT, a, 3, 2, b, 3, b + span - 4, q, s), big, gp)
    refused(name, lambda: bwd(SLOT, a, 3, 2, gg, 3, b, b + span - 4, s), big)                     # the two outputs overlap
    ctx.sync()
