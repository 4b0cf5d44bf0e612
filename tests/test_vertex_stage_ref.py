"""The numpy restatement of the vertex stage the GPU tests build their frames with (support.xform_div_w / vertex_stage / scene_pair)
against the oracle's orc_vertex_stage, word for word, NaN positions in the same places: no GPU.  The oracle takes model / view /
projection / ndc; with view = proj = ndc = identity its NDC_MVP is the model matrix exactly (products with 1 and sums with 0), and its
Normal_M is the inverse transpose of the model, known in closed form where that inverse is exact in binary32."""
import numpy as np

from srz import abi
from support import bits, scene_pair, vertex_stage, xform_div_w

F32 = np.float32
IDENT = np.eye(4, dtype=F32).reshape(16)


def same_tris(got, want, what):
    """every word identical except where both hold a NaN (a NaN's payload and sign are not the reference's to fix)"""
    for key in ("pos", "nrm", "uv"):
        g, w = got[key], want[key]
        assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: {key}: NaN in other places"
        ok = np.isnan(w) | (bits(g) == bits(w))
        assert ok.all(), f"{what}: {key}: {int((~ok).sum())} words differ, first {np.argwhere(~ok)[:4].tolist()}"


def projective_case(seed=0, n_verts=400, n_faces=1000):
    rng = np.random.default_rng(seed)
    M = rng.uniform(-2, 2, 16).astype(F32)
    M[[0 * 4 + 3, 1 * 4 + 3, 2 * 4 + 3, 3 * 4 + 3]] = (0.0, 0.0, 1.0, -0.5)  # the last ROW: w = z - 0.5
    v = np.zeros((n_verts, 8), F32)
    v[:, 0:3] = rng.uniform(-1, 1, (n_verts, 3))
    v[::7, 2] = 0.5  # w == 0 exactly
    v[:, 3:6] = rng.normal(size=(n_verts, 3))
    v[:, 6:8] = rng.uniform(0, 1, (n_verts, 2))
    faces = rng.integers(0, n_verts, (n_faces, 3)).astype(np.uint32)
    return M, v, faces


def test_positions_under_a_projective_matrix(orc):
    """model = M, last row (0, 0, 1, -0.5), every seventh vertex at z = 0.5: w == 0 there (inf / NaN positions), w < 0 behind it.
    z * zscale + zoffset with 49.95 / 50.05 (znear 0.1, zfar 100)"""
    M, v, faces = projective_case()
    want = orc.vertex_stage(v, faces, M, IDENT, IDENT, IDENT, 0.1, 100.0)
    zs, zo = F32((F32(100.0) - F32(0.1)) / F32(2.0)), F32((F32(100.0) + F32(0.1)) / F32(2.0))
    assert (zs, zo) == (F32(49.95), F32(50.05))
    nm = orc.m4_transpose(orc.m4_inverse(M))  # (the oracle's own Normal_M of this model: a general matrix, no closed form)
    got = vertex_stage(v, faces, M, nm, zs, zo)
    w = v[:, 2] - F32(0.5)
    assert int((w == 0).sum()) == len(v[::7]) and int((w < 0).sum()) > 100
    assert int((~np.isfinite(want["pos"]).all(axis=(1, 2))).sum()) > 100  # (triangles setup_triangle must drop)
    same_tris(got, want, "projective")


def test_normals_under_models_with_an_exact_inverse(orc):
    """power-of-two scales, dyadic translations: inverse(model) is exact, Normal_M = diag(1 / s) with the last ROW (-t / s, 1) — w of a
    normal is 1 - sum(t n / s), a non-trivial fourth row, zero for some normals of the first model"""
    rng = np.random.default_rng(1)
    v = np.zeros((90, 8), F32)
    v[:, 0:3], v[:, 3:6], v[:, 6:8] = rng.uniform(-1, 1, (90, 3)), rng.normal(size=(90, 3)), rng.uniform(0, 1, (90, 2))
    v[::9, 3:6] = (4.0, 0.0, 0.0)  # w == 0 under the first model: 1 - 0.25 * 4
    faces = rng.integers(0, 90, (200, 3)).astype(np.uint32)
    for s, t in (((2.0, 0.5, 4.0), (0.5, -1.25, 2.0)), ((0.25, 0.25, 0.25), (1.0, 0.0, -3.5)), ((1.0, 8.0, 0.125), (0.0, 0.0, 0.0))):
        model = np.zeros(16, F32)
        model[[0, 5, 10]], model[12:15], model[15] = s, t, 1.0
        nm = np.zeros(16, F32)
        nm[[0, 5, 10]] = 1.0 / np.asarray(s, F32)
        nm[[3, 7, 11]] = -np.asarray(t, F32) / np.asarray(s, F32)
        nm[15] = 1.0
        assert np.array_equal(orc.m4_transpose(orc.m4_inverse(model)), nm)  # (values: a -0 where the closed form has +0 is equal)
        want = orc.vertex_stage(v, faces, model, IDENT, IDENT, IDENT, 0.1, 100.0)
        got = vertex_stage(v, faces, model, nm, F32(49.95), F32(50.05))
        same_tris(got, want, f"scale {s} translation {t}")
        hit_zero_w = bool(np.isnan(want["nrm"]).any())
        assert hit_zero_w == (t == (0.5, -1.25, 2.0)), (s, t)


def test_one_vertex_by_hand():
    """x' = (2 * 1 + 0 * 2) + (0 * 3 + 1) = 3, y' = (0 + 0.5 * 2) + (0 - 2) = -1, z' = (0 + 0) + (4 * 3 + 0) = 12,
    w = (0 + 0) + (1 * 3 - 1) = 2 -> (1.5, -0.5, 6); depth 6 * 0.5 + 10 = 13.  Normal (1, 2, 3) through diag(2, 2, 2) with the last
    row (0, 1, 0, 2): (2, 4, 6) / (2 + 2) = (0.5, 1, 1.5)"""
    m = np.zeros(16, F32)
    m[0 * 4 + 0], m[1 * 4 + 1], m[2 * 4 + 2] = 2.0, 0.5, 4.0
    m[3 * 4 + 0], m[3 * 4 + 1] = 1.0, -2.0
    m[2 * 4 + 3], m[3 * 4 + 3] = 1.0, -1.0
    nm = np.zeros(16, F32)
    nm[[0, 5, 10]] = 2.0
    nm[1 * 4 + 3], nm[3 * 4 + 3] = 1.0, 2.0
    v = np.array([[1.0, 2.0, 3.0, 1.0, 2.0, 3.0, 0.25, 0.75]], F32)
    assert xform_div_w(m, v[:, 0:3]).tolist() == [[1.5, -0.5, 6.0]]
    t = vertex_stage(v, [[0, 0, 0]], m, nm, 0.5, 10.0)
    assert t["pos"].tolist() == [[[1.5, -0.5, 13.0]] * 3]
    assert t["nrm"].tolist() == [[[0.5, 1.0, 1.5]] * 3]
    assert t["uv"].tolist() == [[[0.25, 0.75]] * 3]


def test_scene_pair_builds_both_frames():
    """no context: nothing is uploaded; the Frame's batches are vertex_stage()'s triangles, the SceneFrame names the slots"""
    M, v, faces = projective_case(3, 30, 40)
    empty = np.zeros((0, 3), np.uint32)
    draws = [(v, faces, abi.SHADER_NORMAL, -1, M, IDENT), (v, empty, abi.SHADER_PHONG, -1, IDENT, M), (v, faces, abi.SHADER_PHONG, -1, IDENT, M)]
    sf, f = scene_pair(draws, 64, 48, (0, 0, 1), [((1, 2, 3), (4, 5, 6))], 49.95, 50.05, slots=[4, 9, 4], p=7.5)
    assert (sf.c.n_draws, f.c.n_batches, sf.c.n_lights, f.c.n_lights) == (3, 3, 1, 1) and sf.c.p == f.c.p == 7.5
    assert [sf._draws[i].mesh_id for i in range(3)] == [4, 9, 4] and [len(t) for t in f.tris] == [40, 0, 40]
    assert list(sf._draws[0].ndc_mvp) == M.tolist() and list(sf._draws[2].normal_m) == M.tolist()
    same_tris(f.tris[2], vertex_stage(v, faces, IDENT, M, 49.95, 50.05), "scene_pair batch 2")
