"""The test reference of the mesh Laplacian (tests/lap_ref.c holds the rules of srz_mesh_laplacian and srz_mesh_laplacian_grad once, in
a `real` type compiled as binary32 and as binary64): the binary32 functions give the bits the device must give, the binary64 ones
what the DERIVED rounding bounds below are held against (tests/test_lap_ref.py).  Corner lists: normalsref.Lists.  Built and loaded
like tests/normalsref.py's library; nothing of the product is involved."""
import ctypes as C

import numpy as np

from normalsref import U, Lists, gamma  # noqa: F401
from support import ref_lib

vp, u32, ci = C.c_void_p, C.c_uint32, C.c_int
_SIG = (None, [vp, u32, u32, u32, vp, vp, vp, ci, vp, u32, vp, u32])
SIGNATURES = {"lr_apply_f32": _SIG, "lr_apply_t_f32": _SIG, "lr_apply_f64": _SIG, "lr_apply_t_f64": _SIG}
UMBRELLA, GRAPH, COTAN = 0, 1, 2
KINDS = {"umbrella": UMBRELLA, "graph": GRAPH, "cotan": COTAN}


def lib(tmpdir):
    return ref_lib("lap_ref", tmpdir, SIGNATURES)


def apply(tmpdir, L, x, kind, wpos=None, transpose=False, dtype=np.float32):
    """x [V, C] or [B, V, C] (any C) -> the operator of `kind` (a name or its number) over Lists L applied to it, in `dtype`
    (np.float32: the device's bits; np.float64: the same rule in binary64); transpose: the backward's rule over x = gout.  wpos [V, 3]:
    COTAN's weight positions, one set"""
    kind = KINDS.get(kind, kind)
    x = np.ascontiguousarray(x, dtype)
    sets = x.reshape((1,) + x.shape) if x.ndim == 2 else x
    assert sets.shape[1] == L.n_verts
    w = np.zeros((max(1, L.n_verts), 3), dtype) if wpos is None else np.ascontiguousarray(wpos, dtype)
    assert kind != COTAN or (wpos is not None and w.shape == (L.n_verts, 3))
    fn = getattr(lib(tmpdir), ("lr_apply_t_" if transpose else "lr_apply_") + ("f32" if dtype == np.float32 else "f64"))
    out = np.zeros_like(sets)
    n_ch = sets.shape[2]
    for s in range(len(sets)):
        fn(sets[s].ctypes.data, n_ch, n_ch, L.n_verts, L.faces.ctypes.data, L.off.ctypes.data, L.corners.ctypes.data, kind, w.ctypes.data, 3,
           out[s].ctypes.data, n_ch)
    return out.reshape(x.shape)


def dense(tmpdir, L, kind, wpos=None, dtype=np.float64):
    """the operator's matrix [V, V] (out = M @ x) assembled from the reference applied to the identity"""
    return apply(tmpdir, L, np.eye(L.n_verts, dtype=dtype), kind, wpos, dtype=dtype)


# ------------------------------------------------------------------------------------------------ the derived bounds
# binary32 against binary64 over the same binary32 inputs.  An element that is a sum of terms, each of which passes through at most n
# roundings on its way into the result, is off by at most gamma_n * sum |term| (Higham, Accuracy and Stability, 3.1) — n counted
# from the rule, the sums of absolute terms evaluated in float64.  The binary64 evaluation's own rounding (2^-29 of these) is not
# counted, as in normalsref.
def _neigh(L):
    """per corner of the lists, in list order: (v, a, b, k, face) as int64 arrays"""
    corners = L.corners[:3 * L.n_faces].astype(np.int64)
    v = np.repeat(np.arange(L.n_verts), np.diff(L.off.astype(np.int64)))
    face, k = corners // 3, corners % 3
    f = L.f
    return v, f[face, (k + 1) % 3], f[face, (k + 2) % 3], k, face


def plain_bound(L, x, kind, transpose=False):
    """UMBRELLA, GRAPH and UMBRELLA's transpose, x [V, C] -> the bound [V, C].  With m = |list(v)|:
      UMBRELLA:   a neighbour's value passes the pair's add, at most m adds of S, the division and the subtraction: m + 3 roundings; x[v]
                  one.  |err| <= gamma_(m+3) (|x[v]| + sum (|x[a]| + |x[b]|) / n_v)
      GRAPH:      no division; n_v * x[v] is one rounding and the subtraction one more: |err| <= gamma_(m+2) (n_v |x[v]| + sum (|x[a]| + |x[b]|))
      TRANSPOSE:  each quotient is a rounding, then as UMBRELLA's without its division: |err| <= gamma_(m+3) (|g[v]| + sum (|g[a]| / n_a +
                  |g[b]| / n_b))"""
    kind = KINDS.get(kind, kind)
    ax = np.abs(np.asarray(x, np.float64))
    v, a, b, _, _ = _neigh(L)
    m = np.diff(L.off.astype(np.int64)).astype(np.float64)
    n = 2.0 * m
    SA = np.zeros_like(ax)
    if kind == UMBRELLA and transpose:
        np.add.at(SA, v, ax[a] / n[a][:, None] + ax[b] / n[b][:, None])
        return gamma(m + 3)[:, None] * (np.where(m[:, None] > 0, ax, 0.0) + SA)
    np.add.at(SA, v, ax[a] + ax[b])
    if kind == GRAPH:
        return gamma(m + 2)[:, None] * (n[:, None] * ax + SA)
    assert kind == UMBRELLA
    with np.errstate(all="ignore"):
        return np.where(m[:, None] > 0, gamma(m + 3)[:, None] * (ax + SA / n[:, None]), 0.0)


def cotan_weights64(L, wpos):
    """per face, in float64 from the float32 positions -> a namespace: ok [F] (the face is not skipped), cot [F, 3] (zeros where
    skipped), dcot [F, 3] a bound on |binary32 cot - cot| (inf where the two evaluations may disagree on `ok` or the weight is not
    resolved).  The derivation, with e the edges (one rounded difference each):
      N's component = e1.y e2.z - e1.z e2.y: each product carries two rounded edges, its own rounding and the subtraction's: off by
        dN = gamma_4 A, A = |e1.y e2.z| + |e1.z e2.y|
      d2 = dot3(N, N): each square carries its rounding and at most two adds: |d2 - D2| <= sum (2 |N| dN + dN^2)(1 + gamma_3) + gamma_3 D2;
        rho = that / D2 must stay below 1/2 (else inf)
      ia = 1 / sqrt(d2): (1 - rho)^(-1/2) <= 1 / (1 - rho), then the root's and the division's rounding: relative e_ia =
        (1 + rho / (1 - rho))(1 + gamma_2) - 1
      dot_m: two rounded edges, the product, at most two adds: off by gamma_5 DA, DA = sum |e_a,i e_b,i|;  cot = dot * ia, one more
        rounding:  dcot = IA (gamma_5 DA (1 + e_ia)(1 + u) + |dot| ((1 + e_ia)(1 + u) - 1))"""
    import types
    p = np.asarray(wpos, np.float32).astype(np.float64)
    f = L.f
    q = p[f]  # [F, 3, 3]
    e1, e2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
    N = np.cross(e1, e2)
    A = np.abs(e1[:, [1, 2, 0]] * e2[:, [2, 0, 1]]) + np.abs(e1[:, [2, 0, 1]] * e2[:, [1, 2, 0]])
    dN = gamma(4) * A
    D2 = (N * N).sum(1)
    with np.errstate(all="ignore"):
        rho = ((2 * np.abs(N) * dN + dN * dN).sum(1) * (1 + gamma(3)) + gamma(3) * D2) / D2
        exact_zero = (D2 == 0) & (A.sum(1) == 0)  # (every product is zero in both evaluations: skipped by both)
        ok = (D2 > 0) & (D2 <= np.finfo(np.float32).max)
        good = ok & (rho < 0.5)
        e_ia = (1 + rho / (1 - rho)) * (1 + gamma(2)) - 1
        IA = 1.0 / np.sqrt(D2)
        cot, dcot = np.zeros((len(f), 3)), np.zeros((len(f), 3))
        for m in range(3):
            ea, eb = q[:, (m + 1) % 3] - q[:, m], q[:, (m + 2) % 3] - q[:, m]
            dot, DA = (ea * eb).sum(1), np.abs(ea * eb).sum(1)
            grow = (1 + e_ia) * (1 + U)
            cot[:, m] = np.where(ok, dot * IA, 0.0)
            dcot[:, m] = np.where(good, IA * (gamma(5) * DA * grow + np.abs(dot) * (grow - 1)), np.where(exact_zero, 0.0, np.inf))
    return types.SimpleNamespace(ok=ok, cot=cot, dcot=dcot)


def cotan_bound(L, x, wpos):
    """COTAN, x [V, C] -> the bound [V, C] (inf at a vertex of a face whose weights are not resolved).  A corner's two products carry
    the difference's rounding, their own, the pair's add and at most m adds of acc (0.5 * acc is exact): m + 3 roundings on top of
    the weight's own error:
      |err| <= 0.5 sum_c [ (dcot_b |x[v] - x[a]| + dcot_a |x[v] - x[b]|)(1 + gamma_(m+3)) + gamma_(m+3) (|cot_b| |x[v] - x[a]| + |cot_a| |x[v] - x[b]|) ]"""
    w = cotan_weights64(L, wpos)
    x = np.asarray(x, np.float64)
    v, a, b, k, face = _neigh(L)
    m = np.diff(L.off.astype(np.int64)).astype(np.float64)
    g = gamma(m + 3)[v][:, None]
    da, db = np.abs(x[v] - x[a]), np.abs(x[v] - x[b])
    cot_a, cot_b = np.abs(w.cot[face, (k + 1) % 3])[:, None], np.abs(w.cot[face, (k + 2) % 3])[:, None]
    dcot_a, dcot_b = w.dcot[face, (k + 1) % 3][:, None], w.dcot[face, (k + 2) % 3][:, None]
    with np.errstate(invalid="ignore"):
        term = (np.where(da > 0, dcot_b * da, 0.0) + np.where(db > 0, dcot_a * db, 0.0)) * (1 + g) + g * (cot_b * da + cot_a * db)
        term = np.where(np.isinf(dcot_a) | np.isinf(dcot_b), np.inf, term)
    out = np.zeros_like(x)
    np.add.at(out, v, term)
    return 0.5 * out


def bound(L, x, kind, wpos=None, transpose=False):
    """the derived bound of apply(..., np.float32) against apply(..., np.float64), x [V, C]"""
    kind = KINDS.get(kind, kind)
    return cotan_bound(L, x, wpos) if kind == COTAN else plain_bound(L, x, kind, transpose)


# ------------------------------------------------------------------------------------------------ meshes of the tests' own
def octahedron4():
    """a closed manifold mesh: the octahedron with each face split in four -> (pos [18, 3] float32 on the unit sphere, faces [32, 3])"""
    base = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    tris = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    pos, mid, faces = [tuple(p) for p in base], {}, []

    def midpoint(i, j):
        key = (min(i, j), max(i, j))
        if key not in mid:
            mid[key] = len(pos)
            pos.append(tuple((base[i] + base[j]) / 2))
        return mid[key]
    for a, b, c in tris:
        ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
        faces += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    p = np.array(pos)
    p = p / np.linalg.norm(p, axis=1, keepdims=True)
    assert p.shape == (18, 3) and len(faces) == 32
    return p.astype(np.float32), np.array(faces, np.uint32)
