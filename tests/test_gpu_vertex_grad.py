"""-m gpu: the differentiable vertex stage — srz_frameset_positions (k_positions), srz_sceneset_vertex_grad (k_vertex_grad) and
srz_mesh_update — and srz.visibility.scene_positions, the autograd function that begins the chain.  Expected values: support's numpy
vertex stage for the positions, tests/vertexgradref.py (the rule of include/srz.h, pinned on the CPU by tests/test_vertex_grad_ref.py)
for the gradients: gverts bit for bit, untouched elements included; gdraw within gamma_n * sum |term| of the float64 sums, n the draw's
contributing vertices — derived, not measured —, and exactly untouched where no draw of the slot writes."""
import types

import numpy as np
import pytest
import torch

import chainref as cr
import srz
import vertexgradref as vgr
import vgkit
from srz import abi
from srz import visibility as V
from support import (SENTINEL, bits, ctx, filled, padded_positions, place, same, scene_pair, sceneset_update, stream, visibility,  # noqa: F401
                     words)

pytestmark = pytest.mark.gpu

W = H = 64
IDENT = np.eye(4, dtype=np.float32).reshape(16)
PATTERN = np.float32(-7.25)
SLOT, OTHER = 3, 5
MESHES = {"A": lambda: vgkit.single(), "B": lambda: vgkit.fan(70, 2), "C257": lambda: vgkit.grid(16, 16, 3, extra=1),
          "C700": lambda: vgkit.grid(28, 25, 4)}
M_A = vgkit.perspective(50.0, 46.0, 5.0, 6.0)
M_B = vgkit.perspective(38.0, 52.0, 14.0, 3.0, w=1.5, wx=-0.2, wy=0.3, wz=0.25, sz=2.0, oz=4.0)
M_C = vgkit.perspective(55.0, 40.0, 2.0, 11.0, w=3.0, wx=0.5, wy=0.4, wz=-0.3)
M_O = vgkit.perspective(30.0, 30.0, 20.0, 18.0, w=2.5, oz=1.0)
ZMAP = ((1.75, 0.5), (1.25, 0.25), (0.75, 1.0))  # (zscale, zoffset) per frame: zscale is not 1


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def scene(c, name, pos=None, upload=True, mats=None):
    """three frames of 64 x 64 over mesh `name` in slot SLOT and a small grid in slot OTHER: frame 0 draws SLOT, OTHER, SLOT (two
    matrices), frame 1 SLOT alone, frame 2 OTHER then SLOT; perspective matrices, a depth mapping per frame -> a namespace: the
    abi.SceneFrame's, the abi.Frame's of support.vertex_stage, `draws` as vertexgradref.grad takes them, T and D (both above the
    counts)"""
    p0, faces = MESHES[name]()
    pos = p0 if pos is None else pos
    m_a, m_b, m_c = (M_A, M_B, M_C) if mats is None else mats
    faces = vgkit.oriented(p0, faces, M_A)
    v8, (po, fo) = vgkit.verts8(pos), vgkit.grid(3, 3, 9)
    fo = vgkit.oriented(po, fo, M_O)
    vo8 = vgkit.verts8(po)
    mine = lambda m: (v8, faces, abi.SHADER_NORMAL, -1, m, IDENT)  # noqa: E731
    other = (vo8, fo, abi.SHADER_NORMAL, -1, M_O, IDENT)
    plan = [([mine(m_a), other, mine(m_b)], [SLOT, OTHER, SLOT]), ([mine(m_c)], [SLOT]), ([other, mine(m_b)], [OTHER, SLOT])]
    s = types.SimpleNamespace(name=name, pos=pos, faces=faces, v8=v8, other=(vo8, fo), sframes=[], frames=[], draws=[])
    for i, ((draws, slots), (zs, zo)) in enumerate(zip(plan, ZMAP)):
        sf, f = scene_pair(draws, W, H, (0.0, 0.0, 1.0), [], zs, zo, ctx=c if (upload and i == 0) else None, slots=slots)
        s.sframes.append(sf), s.frames.append(f)
        s.draws.append([(slot, len(d[1]), d[4], zs) for d, slot in zip(draws, slots)])
    s.T = max(f.n_tris for f in s.frames) + 2
    s.D = 3 + 1
    return s


# ------------------------------------------------------------------------------------------------------ positions
def raw_positions(fs, T, s=None, guard=5):
    """srz_frameset_positions into the middle of a buffer of SENTINEL words -> (positions [n, T, 9] as uint32 words, the guard words
    before, after)"""
    n = fs.n_frames * T * 9
    buf = filled((n + 2 * guard,))
    fs.positions(T, buf.data_ptr() + 4 * guard, 4 * n, stream() if s is None else s)
    torch.cuda.synchronize()
    w = words(buf)
    return w[guard:guard + n].reshape(fs.n_frames, T, 9), w[:guard], w[guard + n:]


@pytest.mark.parametrize("name", ["A", "C257"])
def test_positions_of_a_sceneset_and_a_frameset(ctx, name):
    """on a sceneset bit-equal to support.vertex_stage's positions, on the frameset of the same triangles to support.padded_positions;
    the triangles behind a frame's count are +0; the words before and after the buffer keep the sentinel; once on a non-default
    stream; srz.visibility.positions returns the same floats"""
    s = scene(ctx, name)
    want = bits(padded_positions(s.frames, s.T))
    side = torch.cuda.Stream()
    for what, frames in (("sceneset", s.sframes), ("frameset", s.frames)):
        fs = ctx.frameset(frames)
        for st in (None, side.cuda_stream):
            got, before, after = raw_positions(fs, s.T, st)
            assert np.array_equal(got, want), (what, st, np.argwhere(got != want)[:4].tolist())
            assert (before == SENTINEL).all() and (after == SENTINEL).all()
        for i, f in enumerate(s.frames):
            assert not got[i, f.n_tris:].any()
        assert np.array_equal(words(V.positions(fs, s.T)).reshape(want.shape), want)
        if what == "sceneset":
            assert V.positions(fs).shape[1] == s.T - 2  # (the default: the largest triangle count, from the slots' face counts)
        fs.close()


# ------------------------------------------------------------------------------------------------------ vertex_grad
def call(fs, s, gpos, want_gverts=True, want_gdraw=True, slot=SLOT):
    """one srz_sceneset_vertex_grad: gverts starts as PATTERN everywhere; gdraw as PATTERN in the rows no draw of `slot` writes and in
    the padding, zeros in the rows it adds into -> (gverts [n, V, 3], gdraw [n, D, 18]) float32, None where not asked for"""
    n, nv = fs.n_frames, len(s.v8 if slot == SLOT else s.other[0])
    gv = torch.full((n, nv, 3), float(PATTERN), dtype=torch.float32, device="cuda") if want_gverts else None
    gd = None
    if want_gdraw:
        gd = np.full((n, s.D, 18), PATTERN, np.float32)
        for f, draws in enumerate(s.draws):
            for j, d in enumerate(draws):
                if d[0] == slot:
                    gd[f, j] = 0
        gd = dev(gd)
    g = dev(gpos)
    fs.vertex_grad(slot, g.data_ptr(), s.T, gv.data_ptr() if want_gverts else None, gd.data_ptr() if want_gdraw else None, s.D, stream())
    torch.cuda.synchronize()
    return (gv.cpu().numpy() if want_gverts else None), (gd.cpu().numpy() if want_gdraw else None)


def expect(tmp_path, s, gpos, slot=SLOT):
    v8, faces = (s.v8, s.faces) if slot == SLOT else s.other
    dg = vgr.DrawGrad(len(s.draws), s.D)
    gv = vgr.grad(tmp_path, v8, faces, s.draws, slot, gpos, np.full((len(s.draws), len(v8), 3), PATTERN, np.float32), dg)
    return gv, dg


def check_gverts(got, want, what):
    """bit for bit, the untouched elements (still PATTERN) included; a NaN on one side must be a NaN on the other (its payload is the
    machine's)"""
    g, w = bits(got), bits(want)
    g_nan, w_nan = np.isnan(got), np.isnan(want)
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} gverts words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def check_gdraw(got, s, dg, what, slot=SLOT):
    """rows of the slot's draws: within the reference's bound of the float64 sums, bit for bit where one vertex contributes; every
    other row and the padding: still PATTERN, bit for bit"""
    written = np.zeros(got.shape[:2], bool)
    for f, draws in enumerate(s.draws):
        for j, d in enumerate(draws):
            written[f, j] = d[0] == slot
    assert (bits(got[~written]) == bits(PATTERN)).all(), what + ": a row no draw of the slot writes was touched"
    ref, bound = dg.gdraw[written], dg.bound()[written]
    fin = np.isfinite(dg.gabs[written])
    with np.errstate(invalid="ignore"):
        err = np.abs(got[written].astype(np.float64) - ref)
    ratio = err[fin & (bound > 0)] / bound[fin & (bound > 0)]
    print(f"{what}: gdraw max err {err[fin].max() if fin.any() else 0:.3e}, max err / bound {ratio.max() if ratio.size else 0:.3f}, "
          f"max n {int(dg.count.max())}")
    bad = fin & ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} gdraw elements beyond the bound: err {err[bad][:4]} bound {bound[bad][:4]}"
    assert np.array_equal(np.isnan(got[written][~fin]), np.isnan(ref[~fin])), what + ": NaN elements of gdraw"
    inf = ~fin & np.isinf(ref)
    assert np.array_equal(got[written][inf].astype(np.float64), ref[inf]), what + ": infinite elements of gdraw"
    one = np.broadcast_to((dg.count[written] == 1)[:, None], ref.shape) & fin
    assert np.array_equal(got[written][one] + np.float32(0), ref.astype(np.float32)[one] + np.float32(0)), what + ": n = 1 is not exact"


def chain_gpos(fs, s, seed):
    """gpos of a real chain over the set's own visibility render: interpolate_geo → antialias → a smooth loss, backward to the positions
    (one position_grad and one antialias_grad call) -> [n, T, 9] float32"""
    rng = np.random.default_rng([seed, 103])
    vis = visibility(fs)
    pos = V.positions(fs, s.T).requires_grad_(True)
    attr = dev(rng.uniform(0, 1, (s.T, 3, 3)))
    out = V.antialias(fs, vis, V.interpolate_geo(fs, vis, attr, pos), pos)
    gout = np.stack([cr.smooth_planes(seed + i, 3, W, H) for i in range(fs.n_frames)])
    (out * dev(gout)).sum().backward()
    torch.cuda.synchronize()
    return pos.grad.cpu().numpy().reshape(fs.n_frames, s.T, 9)


@pytest.mark.parametrize("source", ["chain", "dense"])
@pytest.mark.parametrize("name", list(MESHES))
def test_vertex_grad_against_the_reference(ctx, tmp_path, name, source):
    """gpos from a real chain (hidden, culled and off-screen triangles carry zeros: their vertices are skipped unless a visible face
    shares them) and as dense random values (every corner contributes); both outputs together, then each alone; then the other slot's
    mesh into the same kind of buffers"""
    s = scene(ctx, name)
    fs = ctx.frameset(s.sframes)
    if source == "chain":
        gpos = chain_gpos(fs, s, 11)
        tri_any = np.abs(gpos).sum(2) > 0
        assert tri_any.any(), "the chain's gpos is all zeros"
        print(f"{name}: {int(tri_any.sum())} triangles of {sum(f.n_tris for f in s.frames)} receive a gradient from the chain")
    else:
        gpos = np.random.default_rng([len(name), 107]).uniform(-1, 1, (3, s.T, 9)).astype(np.float32)
    for slot in (SLOT, OTHER):
        want_gv, dg = expect(tmp_path, s, gpos, slot)
        assert dg.count.any()
        if slot == SLOT and source == "dense":
            named = len(np.unique(s.faces))
            assert (dg.count[0, 0], dg.count[0, 2], dg.count[1, 0], dg.count[2, 1]) == (named,) * 4
            assert (bits(want_gv) == bits(PATTERN)).all(2).sum() == 3 * (len(s.v8) - named)  # (vertices no face names: untouched)
        for want_v, want_d in ((True, True), (True, False), (False, True)):
            what = f"{name} {source} slot {slot} gverts {want_v} gdraw {want_d}"
            gv, gd = call(fs, s, gpos, want_v, want_d, slot)
            if want_v:
                check_gverts(gv, want_gv, what)
            if want_d:
                check_gdraw(gd, s, dg, what, slot)
    fs.close()


def test_a_vertex_on_the_camera_plane(ctx, tmp_path):
    """vertex 2 of the single triangle lies where r3 == 0 under the slot's matrices.  Under zero gpos on its corner it is skipped: every
    output is finite and equals the reference.  Under a non-zero gpos the outputs are non-finite exactly where the reference's are —
    the isnan and isinf masks and the finite remainder are compared."""
    pos, _ = vgkit.single()
    pos[:, 2] = [0.4, 0.3, 0.5]
    keep = dict(wx=0.0, wy=0.0, wz=-4.0, w=2.0)  # r3 = 2 - 4 z: 0 at z = 0.5
    s = scene(ctx, "A", pos, mats=(vgkit.perspective(50.0, 46.0, 5.0, 6.0, **keep), vgkit.perspective(38.0, 52.0, 14.0, 3.0, **keep),
                                   vgkit.perspective(55.0, 40.0, 2.0, 11.0, **keep)))
    fs = ctx.frameset(s.sframes)
    k = 3 * list(s.faces[0]).index(2)  # (the floats of the corner that names vertex 2)
    first = [[sum(d[1] for d in draws[:j]) for j, d in enumerate(draws) if d[0] == SLOT] for draws in s.draws]
    gpos = np.random.default_rng(109).uniform(-1, 1, (3, s.T, 9)).astype(np.float32)
    for f, firsts in enumerate(first):
        for t in firsts:
            gpos[f, t, k:k + 3] = 0
    want_gv, dg = expect(tmp_path, s, gpos)
    gv, gd = call(fs, s, gpos)
    assert np.isfinite(gv).all() and np.isfinite(gd).all() and (bits(gv[:, 2]) == bits(PATTERN)).all()
    check_gverts(gv, want_gv, "r3 == 0, zero gpos")
    check_gdraw(gd, s, dg, "r3 == 0, zero gpos")
    for f, firsts in enumerate(first):
        for t in firsts:
            gpos[f, t, k:k + 3] = [1.0, 0.0, 0.5]
    want_gv, dg = expect(tmp_path, s, gpos)
    gv, gd = call(fs, s, gpos)
    assert not np.isfinite(want_gv[:, 2]).any() and np.isfinite(want_gv[:, :2]).all()
    assert np.array_equal(np.isnan(gv), np.isnan(want_gv)) and np.array_equal(np.isinf(gv), np.isinf(want_gv))
    check_gverts(gv, want_gv, "r3 == 0, non-zero gpos")
    check_gdraw(gd, s, dg, "r3 == 0, non-zero gpos")
    fs.close()


# ------------------------------------------------------------------------------------------------------ mesh_update
def test_mesh_update_under_a_live_set(ctx, orc):
    """new vertices from a device tensor: the live set's render equals the oracle's render of the new mesh bit for bit, with no set
    rebuilt; srz_sceneset_update still accepts the set; positions returns the new positions; and back again"""
    s = scene(ctx, "C257")
    fs = ctx.frameset(s.sframes)
    out = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(113)
    moved = (s.pos + rng.uniform(-0.02, 0.02, s.pos.shape)).astype(np.float32)
    for what, pos in (("as uploaded", s.pos), ("after mesh_update", moved), ("and back", s.pos)):
        now = scene(None, "C257", pos, upload=False)
        if what != "as uploaded":
            V.mesh_update(ctx, SLOT, dev(now.v8))
            torch.cuda.synchronize()
            sceneset_update(ctx, fs, s.sframes)
        out.fill_(-1.0)
        fs.render(out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
        torch.cuda.synchronize()
        for i, f in enumerate(now.frames):
            rc, ref, _ = orc.draw(f)
            assert rc == 0
            same(out[i].cpu().numpy(), ref, f"{what}, frame {i}")
        assert np.array_equal(words(V.positions(fs, s.T)).reshape(3, s.T, 9), bits(padded_positions(now.frames, s.T))), what
    assert not np.array_equal(bits(padded_positions(scene(None, "C257", moved, upload=False).frames, s.T)), bits(padded_positions(s.frames, s.T)))
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


def test_refusals(ctx):
    """every SRZ_E_INVALID of the three entry points, nothing launched and the outputs untouched"""
    s = scene(ctx, "B")
    fs, plain = ctx.frameset(s.sframes), ctx.frameset(s.frames)
    nv, T, D = len(s.v8), s.T, s.D
    L = srz.lib()
    vp = srz.C.c_void_p
    # ---- srz_frameset_positions
    buf = filled((3 * T * 9 + 4,))
    p, nbytes = buf.data_ptr(), 3 * T * 9 * 4
    name = "srz_frameset_positions"
    refused(name, lambda: ctx._check(L.srz_frameset_positions(ctx.h, None, T, vp(p), nbytes, None)), buf)
    refused(name, lambda: fs.positions(T, 0, nbytes, stream()), buf)
    refused(name, lambda: fs.positions(T, p, nbytes - 4, stream()), buf)
    refused(name, lambda: fs.positions(T, p + 2, nbytes, stream()), buf)
    refused(name, lambda: fs.positions(T - 3, p, nbytes, stream()), buf)
    refused(name, lambda: plain.positions(T - 3, p, nbytes, stream()), buf)
    assert L.srz_frameset_positions(None, fs.h, T, vp(p), nbytes, None) == abi.SRZ_E_INVALID
    # ---- srz_mesh_update
    v = filled((nv, 8))
    name = "srz_mesh_update"
    before = words(V.positions(fs, T))
    refused(name, lambda: ctx.mesh_update(200, v.data_ptr(), nv, stream()))          # an empty slot
    refused(name, lambda: ctx.mesh_update(-1, v.data_ptr(), nv, stream()))           # a bad id
    refused(name, lambda: ctx.mesh_update(256, v.data_ptr(), nv, stream()))
    refused(name, lambda: ctx.mesh_update(SLOT, 0, nv, stream()))                    # a null pointer
    refused(name, lambda: ctx.mesh_update(SLOT, v.data_ptr(), nv - 1, stream()))     # a wrong count
    refused(name, lambda: ctx.mesh_update(SLOT, v.data_ptr() + 2, nv, stream()))     # a misaligned pointer
    assert L.srz_mesh_update(None, SLOT, vp(v.data_ptr()), nv, None) == abi.SRZ_E_INVALID
    assert np.array_equal(words(V.positions(fs, T)), before), "a refused srz_mesh_update changed the slot"
    # ---- srz_sceneset_vertex_grad
    name = "srz_sceneset_vertex_grad"
    gpos = torch.zeros((3, T, 9), dtype=torch.float32, device="cuda")
    gv, gd = filled((3, nv, 3)), filled((3, D, 18))
    g, a, b = gpos.data_ptr(), gv.data_ptr(), gd.data_ptr()
    refused(name, lambda: plain.vertex_grad(SLOT, g, T, a, b, D, stream()), gv, gd)        # not a sceneset
    refused(name, lambda: fs.vertex_grad(OTHER + 1, g, T, a, b, D, stream()), gv, gd)      # an empty slot
    refused(name, lambda: fs.vertex_grad(-1, g, T, a, b, D, stream()), gv, gd)
    refused(name, lambda: fs.vertex_grad(256, g, T, a, b, D, stream()), gv, gd)
    ctx.mesh_upload(OTHER + 2, s.v8, s.faces)
    refused(name, lambda: fs.vertex_grad(OTHER + 2, g, T, a, b, D, stream()), gv, gd)      # a slot the set does not draw
    refused(name, lambda: fs.vertex_grad(SLOT, 0, T, a, b, D, stream()), gv, gd)           # no gpos
    refused(name, lambda: fs.vertex_grad(SLOT, g, T, None, None, D, stream()), gv, gd)     # both outputs null
    refused(name, lambda: fs.vertex_grad(SLOT, g, T - 3, a, b, D, stream()), gv, gd)       # pos_tris too small
    refused(name, lambda: fs.vertex_grad(SLOT, g, T, a, b, 2, stream()), gv, gd)           # draw_stride too small
    for bad in ((g + 2, a, b), (g, a + 2, b), (g, a, b + 2)):                              # a misaligned pointer
        refused(name, lambda bad=bad: fs.vertex_grad(SLOT, bad[0], T, bad[1], bad[2], D, stream()), gv, gd)
    big = filled((3 * T * 9 + 3 * nv * 3 + 3 * D * 18,))
    q = big.data_ptr()
    refused(name, lambda: fs.vertex_grad(SLOT, q, T, q + 4 * (3 * T * 9 - 1), None, D, stream()), big)  # gverts overlaps gpos
    refused(name, lambda: fs.vertex_grad(SLOT, q, T, None, q + 4 * (3 * T * 9 - 1), D, stream()), big)  # gdraw overlaps gpos
    refused(name, lambda: fs.vertex_grad(SLOT, q, T, q + 4 * 3 * T * 9, q + 4 * (3 * T * 9 + 3 * nv * 3 - 1), D, stream()), big)  # each other
    assert L.srz_sceneset_vertex_grad(None, fs.h, SLOT, vp(g), T, vp(a), vp(b), D, None) == abi.SRZ_E_INVALID
    fs.vertex_grad(SLOT, g, T, a, None, 2, stream())  # (without gdraw its stride is not looked at; zero gpos: nothing is written)
    torch.cuda.synchronize()
    assert (words(gv) == SENTINEL).all()
    # ---- a slot uploaded anew since the set was created (the set is then destroyed, never rendered: its draws point at freed buffers)
    ctx.mesh_upload(SLOT, s.v8, s.faces)
    refused(name, lambda: fs.vertex_grad(SLOT, g, T, a, b, D, stream()), gv, gd)
    fs.close(), plain.close()
    ctx.sync()


# ------------------------------------------------------------------------------------------------------ autograd
def test_scene_positions_begins_the_chain(ctx, tmp_path, orc):
    """pos = scene_positions(fs, {slot: verts}, mvp, zmap); antialias(fs, vis, [interpolate_geo(fs, vis, attr, pos), depth(fs, vis, pos)],
    pos); backward.  Two frames of vgkit.chain_scene under two matrices, the backdrop a mesh of its own.  The expected values are the
    CPU chain's: chainref.loss_and_grad per frame, its gpos through tests/vertexgradref.py.  verts.grad (the shared [V, 3] form: the
    sum over the frames), mvp.grad and zmap.grad lie within the summed bounds: chainref's bound on every gpos element carried through
    |d position / d parameter| (a float64 restatement's Jacobian), plus the reference's own bound on gdraw, plus 32 * 2^-24 * sum
    |J| |gpos| for the float32 roundings of the rule on both sides (fewer than 16 on any path from a gpos element to an output)."""
    c = vgkit.chain_scene(1)
    m2 = c.m.copy()
    m2[12] += np.float32(1.5)
    m2[13] -= np.float32(1.0)
    mats = [c.m, m2]
    bpos, bfaces = vgkit.backdrop_mesh()
    unit = place(1.0, 1.0, 0.0, 0.0)
    ctx.mesh_upload(0, vgkit.verts8(c.pos), c.faces)
    ctx.mesh_upload(1, vgkit.verts8(bpos), bfaces)
    sframes = [abi.SceneFrame(cr.W, cr.H, (0.0, 0.0, 1.0), np.zeros((0, 2, 3), np.float32),
                              [(0, abi.SHADER_NORMAL, -1, m, IDENT), (1, abi.SHADER_NORMAL, -1, unit, IDENT)], 1.0, 0.0, abi.FUSED_CLEAR) for m in mats]
    fs = ctx.frameset(sframes)
    P = [vgkit.chain_positions(c, c.pos, m) for m in mats]
    T, nv = len(P[0]), len(c.pos)
    assert np.array_equal(words(V.positions(fs)).reshape(2, T, 9), bits(np.stack(P)).reshape(2, T, 9)), "the set's positions are not the CPU chain's"
    attr = cr.attributes(1, P[0], 3)
    gout = np.stack([cr.smooth_planes(1 + f, 4) for f in range(2)])
    # ---- the CPU chain
    base = [cr.loss_and_grad(tmp_path, orc, P[f], attr, gout[f], depth=True) for f in range(2)]
    draws = [[(0, T - 1, m, 1.0), (1, 1, unit, 1.0)] for m in mats]
    gpos = np.stack([b.total for b in base]).astype(np.float32).reshape(2, T, 9)
    gbound = np.stack([b.interior.bound() + b.silhouette.bound() for b in base])  # [2, T, 3, 3]
    gmag = np.abs(np.stack([b.total for b in base])) * 32 * 2.0 ** -24 + gbound
    want_v = vgr.grad(tmp_path, vgkit.verts8(c.pos), c.faces, draws, 0, gpos, np.zeros((2, nv, 3), np.float32), dg := vgr.DrawGrad(2, 2))
    vgr.grad(tmp_path, vgkit.verts8(bpos), bfaces, draws, 1, gpos, None, dg)
    bound_v, bound_d = np.zeros((nv, 3)), dg.bound()
    for f in range(2):
        jv, jm, jz = vgkit.abs_jacobians(c.pos, c.faces, mats[f], 1.0, 0.0)
        bound_v += np.einsum("tkc,tkcvd->vd", gmag[f, :T - 1], jv)
        bound_d[f, 0, :16] += np.einsum("tkc,tkce->e", gmag[f, :T - 1], jm)
        bound_d[f, 0, 16:] += np.einsum("tkc,tkce->e", gmag[f, :T - 1], jz)
        _, jm, jz = vgkit.abs_jacobians(bpos, bfaces, unit, 1.0, 0.0)
        bound_d[f, 1, :16] += np.einsum("tkc,tkce->e", gmag[f, T - 1:], jm)
        bound_d[f, 1, 16:] += np.einsum("tkc,tkce->e", gmag[f, T - 1:], jz)
    # ---- the device
    verts = dev(c.pos).requires_grad_(True)
    mvp = dev(np.stack([np.stack([m, unit]) for m in mats])).requires_grad_(True)
    zmap = dev(np.tile(np.float32([1.0, 0.0]), (2, 2, 1))).requires_grad_(True)
    vis = visibility(fs)
    pos = V.scene_positions(fs, {0: verts}, mvp, zmap)
    assert np.array_equal(words(pos.detach()).reshape(2, T, 9), bits(np.stack(P)).reshape(2, T, 9))
    planes = torch.cat([V.interpolate_geo(fs, vis, dev(attr), pos), V.depth(fs, vis, pos)], 1)
    out = V.antialias(fs, vis, planes, pos)
    (out * dev(gout)).sum().backward()
    torch.cuda.synchronize()
    for f in range(2):
        assert np.array_equal(bits(out[f].detach().cpu().numpy()), bits(base[f].out)), f"frame {f}: the planes are not the CPU chain's"
    for what, got, want, bound in (("verts.grad", verts.grad.cpu().numpy(), want_v.astype(np.float64).sum(0), bound_v),
                                   ("mvp.grad", mvp.grad.cpu().numpy(), dg.gdraw[:, :, :16], bound_d[:, :, :16]),
                                   ("zmap.grad", zmap.grad.cpu().numpy(), dg.gdraw[:, :, 16:], bound_d[:, :, 16:])):
        err = np.abs(got.astype(np.float64) - want)
        print(f"{what}: max |value| {np.abs(want).max():.3e}, max err {err.max():.3e}, max err / bound {(err[bound > 0] / bound[bound > 0]).max():.3f}")
        assert got.shape == want.shape and np.abs(want).max() > 0 and (err <= bound).all(), (what, np.argwhere(err > bound)[:4].tolist())
    assert np.abs(bound_v).max() < 1e-2 * np.abs(want_v).max(), "the bound says nothing"
    fs.close()
