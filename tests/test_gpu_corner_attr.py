"""-m gpu: per-vertex attributes to a sceneset's triangle stream and back — srz_sceneset_corner_attr (k_corner_attr),
srz_sceneset_corner_attr_grad (k_corner_attr_grad) — and srz.visibility.corner_attr.  Expected values: tests/normalsref.py (pinned on
the CPU by tests/test_normals_ref.py), BIT FOR BIT: the forward is a copy, the backward a gather in a stated order.  The chain
corner_attr(mesh_normals(verts)) has no atomics anywhere: its gradient is held bit for bit to the references composed on the CPU."""
import types

import numpy as np
import pytest
import torch

import normalsref as nr
import srz
import vgkit
from srz import abi
from srz import visibility as V
from support import SENTINEL, ctx, filled, scene_pair, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

W = H = 64
IDENT = np.eye(4, dtype=np.float32).reshape(16)
SLOT, OTHER, GUARD = 3, 5, 5
M_A = vgkit.perspective(50.0, 46.0, 5.0, 6.0)
M_B = vgkit.perspective(38.0, 52.0, 14.0, 3.0, w=1.5, wx=-0.2, wy=0.3, wz=0.25, sz=2.0, oz=4.0)
M_O = vgkit.perspective(30.0, 30.0, 20.0, 18.0, w=2.5, oz=1.0)
ZMAP = ((1.75, 0.5), (1.25, 0.25), (0.75, 1.0))
MESHES = {"fan": lambda: vgkit.fan(70, 2), "grid257": lambda: vgkit.grid(16, 16, 3, extra=1)}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def scene(c, tmp_path, name):
    """three frames of 64 x 64 over mesh `name` in slot SLOT and a small grid in slot OTHER (the scene shape of the vertex stage's
    tests): frame 0 draws SLOT, OTHER, SLOT (two matrices), frame 1 OTHER alone — a frame WITHOUT the slot —, frame 2 OTHER then
    SLOT -> a namespace: the abi.SceneFrame's, per frame the draws as (slot, face count), the meshes' normalsref.Lists, T above the
    counts"""
    pos, faces = MESHES[name]()
    faces = vgkit.oriented(pos, faces, M_A)
    v8, (po, fo) = vgkit.verts8(pos), vgkit.grid(3, 3, 9)
    fo = vgkit.oriented(po, fo, M_O)
    vo8 = vgkit.verts8(po)
    mine = lambda m: (v8, faces, abi.SHADER_NORMAL, -1, m, IDENT)  # noqa: E731
    other = (vo8, fo, abi.SHADER_NORMAL, -1, M_O, IDENT)
    plan = [([mine(M_A), other, mine(M_B)], [SLOT, OTHER, SLOT]), ([other], [OTHER]), ([other, mine(M_B)], [OTHER, SLOT])]
    s = types.SimpleNamespace(pos=pos, faces=faces, other_pos=po, sframes=[], frames=[], draws=[],
                              lists={SLOT: nr.Lists(tmp_path, faces, len(pos)), OTHER: nr.Lists(tmp_path, fo, len(po))})
    for i, ((draws, slots), (zs, zo)) in enumerate(zip(plan, ZMAP)):
        sf, f = scene_pair(draws, W, H, (0.0, 0.0, 1.0), [], zs, zo, ctx=c if i == 0 else None, slots=slots)
        s.sframes.append(sf), s.frames.append(f)
        s.draws.append([(slot, len(d[1])) for d, slot in zip(draws, slots)])
    s.T = max(f.n_tris for f in s.frames) + 2
    return s


def guarded(n):
    """a buffer of n + 2 GUARD sentinel words -> (the tensor, the address of word GUARD)"""
    buf = filled((n + 2 * GUARD,))
    return buf, buf.data_ptr() + 4 * GUARD


def body(buf, shape):
    """(the words between the guards in `shape`, all guard words are the sentinel)"""
    w = words(buf)
    return w[GUARD:-GUARD].reshape(shape), bool((w[:GUARD] == SENTINEL).all() and (w[-GUARD:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------ forward and gradient
@pytest.mark.parametrize("n_ch", [1, 3, 64])
@pytest.mark.parametrize("name", list(MESHES))
def test_corner_attr_and_its_gradient_against_the_reference(ctx, tmp_path, name, n_ch):
    """forward with one attribute array for every frame and with one per frame: the slot's corners hold the reference's bits, the
    triangles of the other slot's draws, those behind a frame's count and the guard words keep the sentinel; then the other slot into
    the same buffer.  Gradient of both slots: bit for bit, exact +0 for the frame that does not draw the slot, every element written"""
    s = scene(ctx, tmp_path, name)
    fs = ctx.frameset(s.sframes)
    rng = np.random.default_rng([len(name), n_ch, 167])
    nv, no, T = len(s.pos), len(s.other_pos), s.T
    shape = (3, T, 3, n_ch)
    for attr_frames in (1, 3):
        a = rng.uniform(-1, 1, (nv, n_ch) if attr_frames == 1 else (3, nv, n_ch)).astype(np.float32)
        b = rng.uniform(-1, 1, (no, n_ch)).astype(np.float32)
        buf, at = guarded(int(np.prod(shape)))
        d_a, d_b = dev(a), dev(b)
        torch.cuda.synchronize()
        fs.corner_attr(SLOT, d_a.data_ptr(), n_ch, attr_frames, at, T, stream())
        torch.cuda.synchronize()
        want = np.full(shape, SENTINEL, np.uint32).view(np.float32)
        nr.corner_attr(tmp_path, s.draws, s.lists, {SLOT: a}, want)
        got, intact = body(buf, shape)
        assert intact and np.array_equal(got, want.view(np.uint32)), (name, n_ch, attr_frames, np.argwhere(got != want.view(np.uint32))[:4].tolist())
        assert (got == SENTINEL).any() and (got[1] == SENTINEL).all() and (got[:, T - 2:] == SENTINEL).all()
        fs.corner_attr(OTHER, d_b.data_ptr(), n_ch, 1, at, T, stream())
        torch.cuda.synchronize()
        nr.corner_attr(tmp_path, s.draws, s.lists, {OTHER: b}, want)
        got, intact = body(buf, shape)
        assert intact and np.array_equal(got, want.view(np.uint32)), (name, n_ch, attr_frames, "second slot")
    gout = rng.uniform(-1, 1, shape).astype(np.float32)
    d_gout = dev(gout)
    for slot, n in ((SLOT, nv), (OTHER, no)):
        buf, at = guarded(3 * n * n_ch)
        torch.cuda.synchronize()
        fs.corner_attr_grad(slot, d_gout.data_ptr(), n_ch, at, T, stream())
        torch.cuda.synchronize()
        want = nr.corner_attr_grad(tmp_path, s.draws, s.lists[slot], slot, gout)
        got, intact = body(buf, want.shape)
        assert intact and np.array_equal(got, want.view(np.uint32)), (name, n_ch, slot, np.argwhere(got != want.view(np.uint32))[:4].tolist())
        if slot == SLOT:
            assert not got[1].any() and got[0].any() and got[2].any()
    fs.close()


# ------------------------------------------------------------------------------------------------------ autograd
def test_the_chain_through_the_normals_is_deterministic(ctx, tmp_path):
    """torch.autograd.grad of corner_attr(fs, {slot: mesh_normals(ctx, slot, verts)}) against a fixed random cotangent, for the [V, 3]
    form shared by the frames (frame 1 does not draw the slot: its share is exact +0, so the sum over the frames has one order) and
    for the [n_frames, V, 3] form: bit-equal to normalsref's two backward rules composed on the CPU, and to a second run"""
    s = scene(ctx, tmp_path, "grid257")
    fs = ctx.frameset(s.sframes)
    L = s.lists[SLOT]
    cot = np.random.default_rng(173).uniform(-1, 1, (3, s.T, 3, 3)).astype(np.float32)
    gattr = nr.corner_attr_grad(tmp_path, s.draws, L, SLOT, cot)
    per_frame = np.stack([s.pos, s.pos + np.float32(0.01), s.pos * np.float32(1.01)]).astype(np.float32)
    for p, gn in ((s.pos, gattr[0] + gattr[1] + gattr[2]), (per_frame, gattr)):
        verts = dev(p).requires_grad_(True)
        runs = []
        for _ in range(2):
            out = V.corner_attr(fs, {SLOT: V.mesh_normals(ctx, SLOT, verts)}, pos_tris=s.T)
            (g,) = torch.autograd.grad(out, verts, dev(cot))
            torch.cuda.synchronize()
            runs.append(words(g))
        want_out = nr.corner_attr(tmp_path, s.draws, s.lists, {SLOT: nr.normals(tmp_path, L, p)}, np.zeros((3, s.T, 3, 3), np.float32))
        assert np.array_equal(words(out.detach()), want_out.view(np.uint32))
        want = nr.normals_grad(tmp_path, L, p, np.ascontiguousarray(gn, np.float32))
        assert want.any() and np.array_equal(runs[0].reshape(want.shape), want.view(np.uint32)), np.argwhere(runs[0].reshape(want.shape) != want.view(np.uint32))[:4].tolist()
        assert np.array_equal(runs[0], runs[1])
    fs.close()


def test_interpolate_takes_the_stream_as_laid_out(ctx, tmp_path):
    """interpolate over the set's own visibility buffer, fed corner_attr's stream of both slots, is bit-equal to interpolate fed the same
    values laid out by numpy fancy indexing; and its gradient reaches both vertex arrays (float atomics in interpolate's own
    backward: values not compared bit for bit)"""
    s = scene(ctx, tmp_path, "grid257")
    fs = ctx.frameset(s.sframes)
    rng = np.random.default_rng(179)
    a, b = rng.uniform(0, 1, (len(s.pos), 3)).astype(np.float32), rng.uniform(0, 1, (len(s.other_pos), 3)).astype(np.float32)
    laid = np.zeros((3, s.T, 3, 3), np.float32)
    faces = {SLOT: s.lists[SLOT].f, OTHER: s.lists[OTHER].f}
    for f, draws in enumerate(s.draws):
        first = 0
        for slot, nf in draws:
            laid[f, first:first + nf] = (a if slot == SLOT else b)[faces[slot]]
            first += nf
    vis = visibility(fs)
    assert (words(vis)[:, 1] != 0).sum() > 300
    ta, tb = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    stream_ = V.corner_attr(fs, {SLOT: ta, OTHER: tb}, pos_tris=s.T)
    assert np.array_equal(words(stream_.detach()), laid.view(np.uint32))
    out = V.interpolate(fs, vis, stream_)
    want = V.interpolate(fs, vis, dev(laid))
    torch.cuda.synchronize()
    assert np.array_equal(words(out.detach()), words(want)) and words(want).any()
    out.sum().backward()
    torch.cuda.synchronize()
    assert ta.grad.shape == ta.shape and tb.grad.shape == tb.shape and ta.grad.abs().sum() > 0 and tb.grad.abs().sum() > 0
    with pytest.raises(ValueError):
        V.corner_attr(fs, {SLOT: ta, OTHER: tb[:, :2]})
    fs.close()


# ------------------------------------------------------------------------------------------------------ refusals
def refused(fn_name, fn, *untouched):
    """fn() raises SRZ_E_INVALID naming fn_name; every tensor of `untouched` still holds the sentinel"""
    with pytest.raises(srz.SrzError) as e:
        fn()
    assert e.value.code == abi.SRZ_E_INVALID and fn_name in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for t in untouched:
        assert (words(t) == SENTINEL).all(), fn_name + ": an output was written"


def test_refusals(ctx, tmp_path):
    """every SRZ_E_INVALID of the two entry points: nothing launched, the outputs keep the sentinel"""
    s = scene(ctx, tmp_path, "fan")
    fs, plain = ctx.frameset(s.sframes), ctx.frameset(s.frames)
    nv, T, C_ = len(s.pos), s.T, 3
    L = srz.lib()
    vp = srz.C.c_void_p
    attr, out, gattr = filled((3, nv, C_)), filled((3, T, 3, C_)), filled((3, nv, C_))
    a, o, g, st = attr.data_ptr(), out.data_ptr(), gattr.data_ptr(), stream()
    fwd, bwd = "srz_sceneset_corner_attr", "srz_sceneset_corner_attr_grad"
    assert L.srz_sceneset_corner_attr(None, fs.h, SLOT, vp(a), C_, 1, vp(o), T, None) == abi.SRZ_E_INVALID
    assert L.srz_sceneset_corner_attr_grad(None, fs.h, SLOT, vp(o), C_, vp(g), T, None) == abi.SRZ_E_INVALID
    refused(fwd, lambda: ctx._check(L.srz_sceneset_corner_attr(ctx.h, None, SLOT, vp(a), C_, 1, vp(o), T, None)), out)  # no set
    refused(bwd, lambda: ctx._check(L.srz_sceneset_corner_attr_grad(ctx.h, None, SLOT, vp(o), C_, vp(g), T, None)), gattr)
    refused(fwd, lambda: plain.corner_attr(SLOT, a, C_, 1, o, T, st), out)                      # not a sceneset
    refused(bwd, lambda: plain.corner_attr_grad(SLOT, o, C_, g, T, st), gattr)
    ctx.mesh_upload(OTHER + 2, vgkit.verts8(s.pos), s.faces)
    for slot in (-1, 256, OTHER + 1, OTHER + 2):                                                # a bad id, an empty slot, one not drawn
        refused(fwd, lambda slot=slot: fs.corner_attr(slot, a, C_, 1, o, T, st), out)
        refused(bwd, lambda slot=slot: fs.corner_attr_grad(slot, o, C_, g, T, st), gattr)
    for n_ch in (0, abi.ATTR_MAX_CH + 1):
        refused(fwd, lambda n_ch=n_ch: fs.corner_attr(SLOT, a, n_ch, 1, o, T, st), out)
        refused(bwd, lambda n_ch=n_ch: fs.corner_attr_grad(SLOT, o, n_ch, g, T, st), gattr)
    refused(fwd, lambda: fs.corner_attr(SLOT, a, C_, 1, o, T - 3, st), out)                     # pos_tris below a frame's count
    refused(bwd, lambda: fs.corner_attr_grad(SLOT, o, C_, g, T - 3, st), gattr)
    for frames in (0, 2, 4):
        refused(fwd, lambda frames=frames: fs.corner_attr(SLOT, a, C_, frames, o, T, st), out)  # attr_frames not 1 or 3
    refused(fwd, lambda: fs.corner_attr(SLOT, 0, C_, 1, o, T, st), out)                         # a null buffer
    refused(fwd, lambda: fs.corner_attr(SLOT, a, C_, 1, 0, T, st), out)
    refused(bwd, lambda: fs.corner_attr_grad(SLOT, 0, C_, g, T, st), gattr)
    refused(bwd, lambda: fs.corner_attr_grad(SLOT, o, C_, 0, T, st), gattr)
    refused(fwd, lambda: fs.corner_attr(SLOT, a + 2, C_, 1, o, T, st), out)                     # a misaligned pointer
    refused(fwd, lambda: fs.corner_attr(SLOT, a, C_, 1, o + 2, T, st), out)
    refused(bwd, lambda: fs.corner_attr_grad(SLOT, o + 2, C_, g, T, st), gattr)
    refused(bwd, lambda: fs.corner_attr_grad(SLOT, o, C_, g + 2, T, st), gattr)
    big = filled((3 * T * 3 * C_ + 3 * nv * C_,))
    q, n_out = big.data_ptr(), 3 * T * 3 * C_
    refused(fwd, lambda: fs.corner_attr(SLOT, q + 4 * (n_out - 1), C_, 3, q, T, st), big)       # the output overlaps the attributes
    refused(bwd, lambda: fs.corner_attr_grad(SLOT, q, C_, q + 4 * (n_out - 1), T, st), big)     # the gradient overlaps gout
    # a slot uploaded anew since the set was created (the set is then destroyed, never rendered: its draws point at freed buffers)
    ctx.mesh_upload(SLOT, vgkit.verts8(s.pos), s.faces)
    refused(fwd, lambda: fs.corner_attr(SLOT, a, C_, 1, o, T, st), out)
    refused(bwd, lambda: fs.corner_attr_grad(SLOT, o, C_, g, T, st), gattr)
    fs.close(), plain.close()
    ctx.sync()
