"""-m gpu: the mesh Laplacian on the device — srz_mesh_laplacian and srz_mesh_laplacian_grad (k_mesh_laplacian).  Expected values:
tests/lapref.py's binary32 functions (the rules of include/srz.h, pinned on the CPU by tests/test_lap_ref.py), BIT FOR BIT — both
passes are gathers without atomics; a NaN on one side must be a NaN on the other (its sign and payload are the machine's).  The
shapes are the smallest at which the kernel can go wrong: one vertex past a block (grid257), more than two blocks (grid700), a corner
list longer than a wave (fan), a vertex no face names and a mesh without faces (n_v = 0), degenerate and non-finite weight positions
(edge), a closed mesh (octa); channel counts on both sides of the kernel's chunk of four, and the cap."""
import numpy as np
import pytest
import torch

import lapref as lr
import normalsref as nr
import vgkit
from srz import abi
from srz import visibility as V
from support import SENTINEL, ctx, filled, stream, words  # noqa: F401

pytestmark = pytest.mark.gpu

SLOT, GUARD = 9, 5
KINDS = (abi.LAP_UMBRELLA, abi.LAP_GRAPH, abi.LAP_COTAN)
CHANNELS = (1, 3, 4, 5, 64)
MESHES = {"single": vgkit.single, "fan": lambda: vgkit.fan(70, 2), "grid257": lambda: vgkit.grid(16, 16, 3, extra=1),
          "grid700": lambda: vgkit.grid(28, 25, 4), "edge": lambda: nr.edge_mesh()[:2],
          "no-faces": lambda: (vgkit.grid(3, 3, 5)[0], np.zeros((0, 3), np.uint32)), "octa": lr.octahedron4}


def i32(a):
    """a float32 / uint32 numpy array's words as an int32 tensor on the device"""
    return torch.as_tensor(np.ascontiguousarray(a).view(np.int32)).cuda()


def differing(got_words, want):
    return nr.same_or_nan(np.ascontiguousarray(got_words).view(np.float32), want)


def upload(c, name):
    pos, faces = MESHES[name]()
    c.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    return pos, faces


def packed(call, d_x, n_ch, n_sets, kind, d_wpos, n, st=None):
    """one plain call, packed, into the middle of a buffer of sentinel words -> the output's words [n]; the guards are checked"""
    buf = filled((n + 2 * GUARD,))
    torch.cuda.synchronize()
    call(SLOT, d_x, n_ch, n_ch, n_sets, kind, d_wpos, 3, buf.data_ptr() + 4 * GUARD, n_ch, stream() if st is None else st)
    torch.cuda.synchronize()
    w = words(buf)
    assert (w[:GUARD] == SENTINEL).all() and (w[GUARD + n:] == SENTINEL).all(), "a guard word was written"
    return w[GUARD:GUARD + n]


def strided(call, x, kind, d_wpos):
    """the same call with x in records of C + 2 floats (from float 1) and the output in records of C + 3 (from float 2), both filled
    with sentinel words -> the output's words in x's shape; the records' other floats and the guards are checked"""
    n_sets, nv, C_ = x.shape
    xin = filled((n_sets * nv, C_ + 2))
    xin[:, 1:1 + C_] = i32(x).view(-1, C_)
    rec = filled((GUARD + n_sets * nv * (C_ + 3) + GUARD,))
    torch.cuda.synchronize()
    call(SLOT, xin.data_ptr() + 4, C_ + 2, C_, n_sets, kind, d_wpos, 3, rec.data_ptr() + 4 * (GUARD + 2), C_ + 3, stream())
    torch.cuda.synchronize()
    w = words(rec)
    r = w[GUARD:-GUARD].reshape(n_sets, nv, C_ + 3)
    assert (w[:GUARD] == SENTINEL).all() and (w[-GUARD:] == SENTINEL).all(), "a guard word was written"
    assert (r[:, :, :2] == SENTINEL).all() and (r[:, :, 2 + C_:] == SENTINEL).all(), "a record's other floats were written"
    xi = words(xin)
    assert (xi[:, 0] == SENTINEL).all() and (xi[:, 1 + C_] == SENTINEL).all() and np.array_equal(xi[:, 1:1 + C_].reshape(x.shape), x.view(np.uint32))
    return r[:, :, 2:2 + C_]


@pytest.mark.parametrize("n_sets", [1, 3])
@pytest.mark.parametrize("name", list(MESHES))
def test_laplacian_against_the_reference(ctx, tmp_path, name, n_sets):
    """every kind and channel count, forward and backward: packed and strided, bit for bit; two launches bit-equal; the symmetric
    kinds' _grad call gives the forward call's bits"""
    pos, faces = upload(ctx, name)
    nv = len(pos)
    L = lr.Lists(tmp_path, faces, nv)
    d_wpos = i32(pos)
    for C_ in CHANNELS:
        x = np.random.default_rng([len(name), n_sets, C_, 173]).uniform(-1, 1, (n_sets, nv, C_)).astype(np.float32)
        d_x = i32(x)
        for kind in KINDS:
            what = (name, n_sets, C_, kind)
            want = lr.apply(tmp_path, L, x, kind, pos)
            want_t = lr.apply(tmp_path, L, x, kind, pos, transpose=True)
            if name == "no-faces":  # n_v = 0: +0 everywhere (GRAPH: 0 * x[v] - +0, a zero of x[v]'s sign)
                assert not want.any() and not want_t.any() and (kind == abi.LAP_GRAPH or not (want.view(np.uint32) | want_t.view(np.uint32)).any())
            if name == "grid700" and kind != abi.LAP_UMBRELLA:
                assert np.isfinite(want).all() and (want != 0).all()
            fwd = packed(ctx.mesh_laplacian, d_x.data_ptr(), C_, n_sets, kind, d_wpos.data_ptr(), x.size)
            bad = differing(fwd.reshape(x.shape), want)
            assert not bad.any(), (what, "forward", np.argwhere(bad)[:4].tolist())
            bwd = packed(ctx.mesh_laplacian_grad, d_x.data_ptr(), C_, n_sets, kind, d_wpos.data_ptr(), x.size)
            bad = differing(bwd.reshape(x.shape), want_t)
            assert not bad.any(), (what, "backward", np.argwhere(bad)[:4].tolist())
            if kind != abi.LAP_UMBRELLA:
                assert np.array_equal(bwd, fwd), (what, "the symmetric kinds' backward is the forward call")
            if C_ in (3, 4, 5, 64):  # (a part chunk, a full one, one channel past a full one, the cap: the store mask and ch0 under a stride)
                assert np.array_equal(packed(ctx.mesh_laplacian, d_x.data_ptr(), C_, n_sets, kind, d_wpos.data_ptr(), x.size), fwd), (what, "two runs")
                assert np.array_equal(packed(ctx.mesh_laplacian_grad, d_x.data_ptr(), C_, n_sets, kind, d_wpos.data_ptr(), x.size), bwd), (what, "two runs")
                assert np.array_equal(strided(ctx.mesh_laplacian, x, kind, d_wpos.data_ptr()), fwd.reshape(x.shape)), (what, "strided")
                assert np.array_equal(strided(ctx.mesh_laplacian_grad, x, kind, d_wpos.data_ptr()), bwd.reshape(x.shape)), (what, "strided")


def test_on_a_side_stream(ctx, tmp_path):
    pos, faces = upload(ctx, "grid257")
    L = lr.Lists(tmp_path, faces, len(pos))
    x = np.random.default_rng(179).uniform(-1, 1, (2, len(pos), 5)).astype(np.float32)
    d_x, d_wpos = i32(x), i32(pos)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for kind in KINDS:
        got = packed(ctx.mesh_laplacian, d_x.data_ptr(), 5, 2, kind, d_wpos.data_ptr(), x.size, side.cuda_stream)
        assert not differing(got.reshape(x.shape), lr.apply(tmp_path, L, x, kind, pos)).any(), kind
        got = packed(ctx.mesh_laplacian_grad, d_x.data_ptr(), 5, 2, kind, d_wpos.data_ptr(), x.size, side.cuda_stream)
        assert not differing(got.reshape(x.shape), lr.apply(tmp_path, L, x, kind, pos, transpose=True)).any(), kind


def test_the_null_forms_are_the_slots_own_positions(ctx, tmp_path):
    """after mesh_update: a null d_x is the moved positions (stride 8 inside the records), a null d_wpos gives the bits of an explicit
    copy of them — and not those of the positions the slot was uploaded with"""
    pos, faces = upload(ctx, "grid257")
    L = lr.Lists(tmp_path, faces, len(pos))
    moved = (pos + np.random.default_rng(181).uniform(-0.02, 0.02, pos.shape)).astype(np.float32)
    V.mesh_update(ctx, SLOT, torch.as_tensor(vgkit.verts8(moved)).cuda())
    d_moved = i32(moved)
    for kind in KINDS:
        own = packed(ctx.mesh_laplacian, None, 3, 1, kind, None, moved.size)
        assert not differing(own.reshape(moved.shape), lr.apply(tmp_path, L, moved, kind, moved)).any(), kind
        assert np.array_equal(packed(ctx.mesh_laplacian, d_moved.data_ptr(), 3, 1, kind, d_moved.data_ptr(), moved.size), own), kind
    x = np.random.default_rng(191).uniform(-1, 1, (3, len(pos), 4)).astype(np.float32)
    d_x = i32(x)
    for call, t in ((ctx.mesh_laplacian, False), (ctx.mesh_laplacian_grad, True)):
        null = packed(call, d_x.data_ptr(), 4, 3, abi.LAP_COTAN, None, x.size)
        assert np.array_equal(null, packed(call, d_x.data_ptr(), 4, 3, abi.LAP_COTAN, d_moved.data_ptr(), x.size))
        assert not differing(null.reshape(x.shape), lr.apply(tmp_path, L, x, "cotan", moved, transpose=t)).any()
        assert differing(null.reshape(x.shape), lr.apply(tmp_path, L, x, "cotan", pos, transpose=t)).any(), "the test shows nothing"


def test_hand_written_values(ctx, tmp_path):
    """zero, subnormal, huge, infinite and NaN fields on a 5 x 4 grid: the reference's bits, and every non-finite output is at a vertex
    that holds such a value or at one of its neighbours"""
    pos, faces = vgkit.grid(5, 4, 11)
    ctx.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    nv = len(pos)
    L = lr.Lists(tmp_path, faces, nv)
    x = np.random.default_rng(193).uniform(-1, 1, (nv, 6)).astype(np.float32)
    x[:, 0] = 0.0
    x[:, 1] = np.float32(1e-41) * np.arange(1, nv + 1, dtype=np.float32)  # subnormals
    x[:, 2] *= np.float32(3e38)                                           # sums that overflow
    x[6, 3], x[13, 3] = np.inf, -np.inf                                   # 6 and 13 are neighbours' neighbours at most
    x[7, 4] = np.nan
    x[0, 5], x[19, 5] = -0.0, np.float32(1e-45)
    assert (np.abs(x[:, 1]) < np.finfo(np.float32).tiny).all()
    hot = {3: [6, 13], 4: [7]}
    d_x, d_wpos = i32(x), i32(pos)
    for kind in KINDS:
        for call, t in ((ctx.mesh_laplacian, False), (ctx.mesh_laplacian_grad, True)):
            got = packed(call, d_x.data_ptr(), 6, 1, kind, d_wpos.data_ptr(), x.size).reshape(x.shape)
            bad = differing(got, lr.apply(tmp_path, L, x, kind, pos, transpose=t))
            assert not bad.any(), (kind, t, np.argwhere(bad)[:4].tolist())
            g = got.view(np.float32)
            assert not got[:, 0].any(), "a zero field does not give +0 everywhere"
            assert np.isfinite(g[:, [0, 1, 5]]).all() and g[:, 1].any()
            for ch, at in hot.items():
                near = np.zeros(nv, bool)
                near[np.unique(faces[np.isin(faces, at).any(1)])] = True
                assert not np.isfinite(g[at, ch]).any() and np.isfinite(g[~near, ch]).all(), (kind, t, ch)
