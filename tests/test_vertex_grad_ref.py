"""not-gpu: the reference of the vertex stage's backward (tests/vertex_grad_ref.c, the rule of include/srz.h verbatim) held to what it
is the derivative of — central differences of a float64 restatement of the vertex stage, and, end to end, frames RENDERED AGAIN with
the mesh and the matrix moved (tests/chainref.py's method) — and the rule's own cases: the skip, list order, a vertex no face names,
a face that names a vertex twice."""
import types

import numpy as np
import pytest

import chainref as cr
import vertexgradref as vgr
import vgkit
from support import vertex_stage

SEEDS = range(8)
# measured on the CPU over SEEDS (test_reference_against_central_differences prints them again; DESIGN.md has the table): the worst gap
# per group of probes.  Asserted: four times the overall worst — the factor covers the seed dependence of float32 rounding in the gradient
FD_GAP = {"vertex": 5.57e-6, "matrix": 1.34e-6, "depth": 9.90e-7}
FD_TOL = 4 * max(FD_GAP.values())


def fd_case(seed):
    """a fan (a long corner list, an unreferenced vertex, a (v, v, w) face) under a perspective matrix whose w varies by a third over
    the mesh, dense random gpos: every corner contributes"""
    rng = np.random.default_rng([seed, 97])
    pos, faces = vgkit.fan(12, seed)
    m = vgkit.perspective(40.0 + seed, 33.0, 3.0, 4.0, w=2.0 + 0.1 * seed)
    zs, zo = np.float32(1.75), np.float32(0.5)
    gpos = rng.uniform(-1, 1, (len(faces) + 2, 9)).astype(np.float32)
    return pos, faces, m, zs, zo, gpos


def loss64(pos, faces, m, zs, zo, gpos):
    P = vgkit.stage64(pos, m, zs, zo)[np.asarray(faces, np.int64)]  # [F, 3, 3]
    return float((gpos[:len(faces)].astype(np.float64).reshape(-1, 3, 3) * P).sum())


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_against_central_differences(tmp_path, seed):
    """L = sum gpos * pos(verts, m, zscale, zoffset) in float64; every vertex axis, all 16 matrix entries and both depth constants are
    moved by +-h (h = 2^-20 of the parameter's scale) and the central difference is compared with the reference's gradient: the gap
    is |dL - <g, step>| / sum |g_i step_i|.  Tolerance: four times the worst gap measured over the seeds."""
    pos, faces, m, zs, zo, gpos = fd_case(seed)
    V = len(pos)
    frames = [[(0, len(faces), m, zs)]]
    gverts = vgr.grad(tmp_path, vgkit.verts8(pos), faces, frames, 0, gpos[None], np.zeros((1, V, 3), np.float32), into=(dg := vgr.DrawGrad(1, 1)))[0]
    named = np.zeros(V, bool)
    named[np.unique(faces)] = True
    assert not gverts[~named].any() and dg.count[0, 0] == named.sum()

    def gap(g, d_l, step):
        return abs(d_l - g * step) / abs(g * step)
    worst = {"vertex": 0.0, "matrix": 0.0, "depth": 0.0}
    p64, m64 = pos.astype(np.float64), m.astype(np.float64)
    for v in np.flatnonzero(named):
        for c in range(3):
            h = 2.0 ** -20
            hi, lo = p64.copy(), p64.copy()
            hi[v, c] += h
            lo[v, c] -= h
            d_l = loss64(hi, faces, m64, zs, zo, gpos) - loss64(lo, faces, m64, zs, zo, gpos)
            worst["vertex"] = max(worst["vertex"], gap(float(gverts[v, c]), d_l, hi[v, c] - lo[v, c]))
    for e in range(16):
        h = 2.0 ** -20 * max(1.0, abs(m64[e]))
        hi, lo = m64.copy(), m64.copy()
        hi[e] += h
        lo[e] -= h
        d_l = loss64(p64, faces, hi, zs, zo, gpos) - loss64(p64, faces, lo, zs, zo, gpos)
        worst["matrix"] = max(worst["matrix"], gap(dg.gdraw[0, 0, e], d_l, hi[e] - lo[e]))
    h = 2.0 ** -20
    for e, (a, b) in enumerate((((zs + h, zo), (zs - h, zo)), ((zs, zo + h), (zs, zo - h)))):
        d_l = loss64(p64, faces, m64, *a, gpos) - loss64(p64, faces, m64, *b, gpos)
        worst["depth"] = max(worst["depth"], gap(dg.gdraw[0, 0, 16 + e], d_l, 2 * h))
    print(f"seed {seed}: worst gap vertex {worst['vertex']:.3e} matrix {worst['matrix']:.3e} depth {worst['depth']:.3e}; recorded {FD_GAP}, "
          f"tolerance {FD_TOL:.3e}")
    assert max(worst.values()) <= FD_TOL, worst


PATTERN = np.float32(-7.25)


def test_skip_keeps_a_vertex_on_the_camera_plane_out(tmp_path):
    """vertex 2 lies on the camera plane (r3 == 0 exactly) and every corner that names it carries zero gpos: its element of gverts keeps
    the pattern it was prefilled with, the draw counts two contributing vertices, and every output is finite.  With a non-zero gpos
    on one of its corners the same vertex is not skipped and its outputs are not finite."""
    pos, faces = vgkit.single()
    m = vgkit.perspective(40.0, 30.0, 2.0, 3.0, w=2.0, wx=0.0, wy=0.0, wz=-4.0)  # r3 = 2 - 4 z
    pos[:, 2] = [0.4, 0.3, 0.5]
    gpos = np.float32([[0.5, -0.25, 0.75, 1.0, 2.0, -0.5, 0.0, 0.0, 0.0]])
    frames = [[(0, 1, m, 1.5)]]
    gv = vgr.grad(tmp_path, vgkit.verts8(pos), faces, frames, 0, gpos[None], np.full((1, 3, 3), PATTERN), into=(dg := vgr.DrawGrad(1, 1)))[0]
    assert np.array_equal(gv[2], np.full(3, PATTERN)) and (gv[:2] != PATTERN).all() and dg.count[0, 0] == 2
    assert np.isfinite(gv).all() and np.isfinite(dg.gdraw).all() and dg.gdraw[0, 0].any()
    gpos[0, 6] = 1.0
    gv = vgr.grad(tmp_path, vgkit.verts8(pos), faces, frames, 0, gpos[None], np.full((1, 3, 3), PATTERN), into=(dg := vgr.DrawGrad(1, 1)))[0]
    assert not np.isfinite(gv[2]).any() and np.isfinite(gv[:2]).all() and not np.isfinite(dg.gdraw[0, 0]).all() and dg.count[0, 0] == 3


def test_list_order_unnamed_vertex_and_twice_named_vertex(tmp_path):
    """the corner lists: every vertex's corners 3 * face + k in increasing order, an empty list for the vertex no face names, both
    corners of the face (1, 1, 3) in vertex 1's.  The sums run in LIST ORDER: with gpos non-zero only in the z slots of the hub's
    corners the hub alone contributes, so the zoffset gradient IS its GZ, a float32 sum whose value depends on the order — it equals
    the sequential float32 sum in increasing corner order and not the one in decreasing order.  Likewise vertex 1's GZ is the sum
    over all its corners, the face's two included."""
    pos, faces = vgkit.fan(70, 5)
    V = len(pos)
    off, corners = vgr.corner_lists(tmp_path, faces, V)
    flat = faces.reshape(-1)
    assert off[0] == 0 and off[V] == len(flat) and sorted(corners.tolist()) == list(range(len(flat)))
    for v in range(V):
        mine = corners[off[v]:off[v + 1]]
        assert (np.diff(mine.astype(np.int64)) > 0).all() and (flat[mine] == v).all()
    assert off[V - 1] == off[V] and off[1] - off[0] == 70 and {3 * 70, 3 * 70 + 1} <= set(corners[off[1]:off[2]].tolist())
    m = vgkit.perspective(40.0, 30.0, 2.0, 3.0)
    frames = [[(0, len(faces), m, 1.0)]]
    rng = np.random.default_rng(101)
    for vertex in (0, 1):
        mine = corners[off[vertex]:off[vertex + 1]]
        vals = (rng.uniform(1, 2, len(mine)) * 10.0 ** rng.integers(-4, 5, len(mine)) * rng.choice([-1, 1], len(mine))).astype(np.float32)
        if vertex == 1:
            vals = np.float32([1.0, 1e8, -9e7])  # (corners 1, 210, 211)
        gpos = np.zeros((len(faces), 9), np.float32)
        gpos.reshape(-1, 3)[mine, 2] = vals
        gv = vgr.grad(tmp_path, vgkit.verts8(pos), faces, frames, 0, gpos[None], np.full((1, V, 3), PATTERN), into=(dg := vgr.DrawGrad(1, 1)))[0]
        fwd = bwd = np.float32(0)
        for x in vals:
            fwd = np.float32(fwd + x)
        for x in vals[::-1]:
            bwd = np.float32(bwd + x)
        assert fwd != bwd, "the values do not tell the orders apart"
        assert dg.count[0, 0] == 1 and dg.gdraw[0, 0, 17] == float(fwd)
        touched = (gv != PATTERN).any(1)
        assert touched[vertex] and touched.sum() == 1


# ------------------------------------------------------------------------------------------------------ end to end, re-rendered
# of the seeds 1 .. 8 the three that meet the cap below on the CPU (chosen by the cap alone: 30 of 33, 27 of 30 and 28 of 31 probes quiet)
E2E_SEEDS = (1, 3, 7)
# the half steps: object-space x and y (a unit is some 35 pixels), object-space z (it moves x and y through w only, an eighth as far),
# the matrix's translation entries (divided by w, about 2.3): each moves a screen position by about chainref.STEP = 2^-9 pixel
H_VERT, H_MAT = (2.0 ** -14, 2.0 ** -14, 2.0 ** -11), 2.0 ** -8
# measured on the CPU (test_end_to_end_against_re_rendered_frames prints them again; DESIGN.md has the table beside chainref's): the
# worst gap of a quiet probe per seed.  Asserted: four times the overall worst
E2E_GAP = {1: 6.79e-4, 3: 1.67e-3, 7: 9.30e-4}
E2E_TOL = 4 * max(E2E_GAP.values())
_e2e = {}


def e2e_evaluate(tmp, orc, seed):
    """the scene, its chain gradient through the reference, and every probe rendered at both ends; computed once per session"""
    if seed in _e2e:
        return _e2e[seed]
    s = vgkit.chain_scene(seed)
    P = vgkit.chain_positions(s, s.pos, s.m)
    T, V = len(P), len(s.pos)
    attr, gout = cr.attributes(seed, P, 3), cr.smooth_planes(seed, 3)
    s.base = cr.loss_and_grad(tmp, orc, P, attr, gout)
    frames = [[(0, T - 1, s.m, s.zs)]]
    gpos = s.base.total.astype(np.float32).reshape(1, T, 9)
    s.dg = vgr.DrawGrad(1, 1)
    s.gverts = vgr.grad(tmp, vgkit.verts8(s.pos), s.faces, frames, 0, gpos, np.zeros((1, V, 3), np.float32), into=s.dg)[0]
    probes = [("vertex", v, c) for v in range(V) for c in range(3)] + [("matrix", e, 0) for e in (12, 13, 14)]
    s.names, quiet, gap, gap0, scales = [], [], [], [], []
    for kind, i, c in probes:
        ends = []
        for sign in (1, -1):
            pos, m = s.pos.copy(), s.m.copy()
            if kind == "vertex":
                pos[i, c] = np.float32(pos[i, c] + np.float32(sign * H_VERT[c]))
            else:
                m[i] = np.float32(m[i] + np.float32(sign * H_MAT))
            ends.append((pos, m, vgkit.chain_positions(s, pos, m)))
        (ph, mh, Ph), (pl, ml, Pl) = ends
        step = float(ph[i, c]) - float(pl[i, c]) if kind == "vertex" else float(mh[i]) - float(ml[i])
        g = float(s.gverts[i, c]) if kind == "vertex" else float(s.dg.gdraw[0, 0, i])
        scale = float((s.base.gabs * np.abs(Ph.astype(np.float64) - Pl.astype(np.float64))).sum())
        if scale == 0.0:  # (a vertex no visible pixel depends on)
            continue
        scales.append(scale)
        a, b = (cr.loss_and_grad(tmp, orc, Q, attr, gout, want_grad=False) for Q in (Ph, Pl))
        quiet.append(all(np.array_equal(e.words[1], s.base.words[1]) and np.array_equal(e.dec, s.base.dec) for e in (a, b)))
        gap.append(abs((a.L - b.L) - g * step) / scale)
        gap0.append(abs(a.L - b.L) / scale)  # (the gradient zeroed)
        s.names.append(f"{kind} {i} {'xyz'[c] if kind == 'vertex' else ''}")
    # (chainref.probes' floor: a probe whose scale is below PROBE_FLOOR of the scene's largest measures the float32 rounding of L, an
    # absolute error whatever the probe, not the rule: left out)
    keep = np.array(scales) >= cr.PROBE_FLOOR * max(scales)
    s.names = [n for n, k in zip(s.names, keep) if k]
    s.quiet, s.gap, s.gap0 = np.array(quiet)[keep], np.array(gap)[keep], np.array(gap0)[keep]
    _e2e[seed] = s
    return s


@pytest.mark.parametrize("seed", E2E_SEEDS)
def test_end_to_end_against_re_rendered_frames(tmp_path, orc, seed):
    """L through chainref.loss_and_grad, its gpos through the reference to gverts and gdraw; every mesh vertex along x, y (+-2^-14
    of the unit square), z (+-2^-11) and the matrix's three translation entries (+-2^-8) are moved and the frame is RENDERED AGAIN; the central
    difference of L against gradient * step, relative to the sum of |gpos_i| * |moved screen position_i| (chainref.gaps' scale).
    Only quiet probes — the id planes and the antialiasing decisions of the three renders equal — are asserted; at most 25 % of the
    probes are not quiet, at least 24 are.  Tolerance: four times the worst quiet gap measured on the CPU over the seeds.  Zeroing
    the gradient makes the worst quiet gap exceed ten tolerances."""
    s = e2e_evaluate(tmp_path, orc, seed)
    q = s.quiet
    worst = float(s.gap[q].max())
    print(f"seed {seed}: {len(q)} probes, {int(q.sum())} quiet; quiet gap worst {worst:.3e} median {np.median(s.gap[q]):.3e}, recorded "
          f"{E2E_GAP[seed]:.3e}, tolerance {E2E_TOL:.3e}; gradient zeroed: worst quiet gap {s.gap0[q].max():.3f}; not quiet: worst "
          f"{s.gap[~q].max() if (~q).any() else 0:.3e}")
    assert (~q).mean() <= 0.25 and q.sum() >= 24, (len(q), int(q.sum()))
    bad = np.flatnonzero(q & (s.gap > E2E_TOL))
    assert not len(bad), [(s.names[i], float(s.gap[i])) for i in bad[:6]]
    assert s.gap0[q].max() > 10 * E2E_TOL


# ------------------------------------------------------------------------------------------------------ fitting, through the references
IDENT = np.eye(4, dtype=np.float32).reshape(16)


@pytest.mark.parametrize("kind", ["matrix", "verts"])
@pytest.mark.parametrize("seed", cr.POSE_SEEDS)
def test_fit_through_the_cpu_chain(tmp_path, orc, seed, kind):
    """vgkit's two descents (its comment states them) with every step through the CPU references: support.vertex_stage → the oracle's
    visibility → chainref.loss_and_grad → tests/vertexgradref.py.  The final errors are the recorded ones, which
    tests/test_gpu_scene_fit.py holds the device to; the matrix descent is chainref's pose recovery, and ends where that does up to the
    rounding of the translation through the matrix."""
    pos0, faces, attr = vgkit.fit_model(seed)
    zero = np.zeros((3, cr.H, cr.W), np.float32)

    def positions(pos, p):
        t = vertex_stage(vgkit.verts8(pos), faces, vgkit.fit_matrix(p), IDENT, 1.0, 0.0)
        return np.concatenate([t["pos"], cr.BACKDROP[None]]).astype(np.float32)
    target = cr.loss_and_grad(tmp_path, orc, positions(pos0, vgkit.FIT_W * np.float32(cr.POSE_OFFSET)), attr, zero, want_grad=False).out

    def grad_of(pos, p):
        P = positions(pos, p)
        out = cr.loss_and_grad(tmp_path, orc, P, attr, zero, want_grad=False).out
        r = cr.loss_and_grad(tmp_path, orc, P, attr, cr.pose_gout(out, target))
        dg = vgr.DrawGrad(1, 1)
        gv = vgr.grad(tmp_path, vgkit.verts8(pos), faces, [[(0, len(faces), vgkit.fit_matrix(p), 1.0)]], 0,
                      r.total.astype(np.float32).reshape(1, -1, 9), np.zeros((1, len(pos), 3), np.float32), dg)[0]
        return gv, dg.gdraw[0, 0]
    err = vgkit.fit_descend(kind, grad_of, pos0)
    recorded = (vgkit.FIT_MATRIX_FINAL if kind == "matrix" else vgkit.FIT_VERTS_FINAL)[seed]
    print(f"seed {seed} {kind}: error 1.0000 -> {err[-1]:.4f} (recorded {recorded:.4f}; chainref's pose recovery {cr.POSE_FINAL[seed]:.4f})")
    assert abs(err[-1] - recorded) < 5e-4
    assert kind == "verts" or abs(err[-1] - cr.POSE_FINAL[seed]) < 0.01
