"""The test reference of the mesh edge terms (tests/edge_ref.c holds the rules of srz_mesh_edges and srz_mesh_edges_grad once, in a
`real` type compiled as binary32 and as binary64): the binary32 functions give the bits the device must give, the binary64 ones what
the DERIVED rounding bounds below are held against (tests/test_edge_ref.py).  Corner lists: normalsref.Lists.  Built and loaded like
tests/normalsref.py's library; nothing of the product is involved."""
import ctypes as C
import types

import numpy as np

from normalsref import U, Lists, gamma  # noqa: F401
from support import ref_lib

vp, u32, ci = C.c_void_p, C.c_uint32, C.c_int
_FWD = (None, [vp, u32, u32, vp, vp, vp, ci, vp, u32])
_BWD = (None, [vp, u32, u32, u32, vp, vp, vp, ci, vp, u32, vp, vp])
SIGNATURES = {"er_entries": (u32, [vp, vp, vp, u32, u32, vp, vp, u32]), "er_forward_f32": _FWD, "er_forward_f64": _FWD,
              "er_backward_f32": _BWD, "er_backward_f64": _BWD}
COUNT, LENGTH, DIHEDRAL = 0, 1, 2
KINDS = {"count": COUNT, "length": LENGTH, "dihedral": DIHEDRAL}


def lib(tmpdir):
    return ref_lib("edge_ref", tmpdir, SIGNATURES)


def _sets(x, dtype):
    x = np.ascontiguousarray(x, dtype)
    return x.reshape((1,) + x.shape) if x.ndim == 2 else x


def forward(tmpdir, L, pos, kind, dtype=np.float32):
    """pos [V, 3] or [B, V, 3] -> the per-(face, edge) field [F, 3] or [B, F, 3] of `kind` (a name or its number) over Lists L, in
    `dtype` (np.float32: the device's bits; np.float64: the same rule in binary64).  COUNT reads no positions: pos may be None"""
    kind = KINDS.get(kind, kind)
    pos = np.zeros((max(1, L.n_verts), 3), dtype) if pos is None else pos
    p = _sets(pos, dtype)
    fn = getattr(lib(tmpdir), "er_forward_" + ("f32" if dtype == np.float32 else "f64"))
    out = np.zeros((len(p), L.n_faces, 3), dtype)
    for s in range(len(p)):
        fn(p[s].ctypes.data, 3, L.n_faces, L.faces.ctypes.data, L.off.ctypes.data, L.corners.ctypes.data, kind, out[s].ctypes.data, 3)
    return out[0] if np.ndim(pos) == 2 else out


def backward(tmpdir, L, pos, kind, gout, dtype=np.float32):
    """pos [V, 3] or [B, V, 3], gout [F, 3] or [B, F, 3] -> gpos in pos' shape (LENGTH or DIHEDRAL)"""
    kind = KINDS.get(kind, kind)
    assert kind in (LENGTH, DIHEDRAL)
    p, g = _sets(pos, dtype), _sets(gout, dtype)
    assert len(p) == len(g) and g.shape[1:] == (L.n_faces, 3)
    fn = getattr(lib(tmpdir), "er_backward_" + ("f32" if dtype == np.float32 else "f64"))
    out, work = np.zeros_like(p), np.zeros((max(1, L.n_faces), 3), dtype)
    for s in range(len(p)):
        fn(p[s].ctypes.data, 3, L.n_verts, L.n_faces, L.faces.ctypes.data, L.off.ctypes.data, L.corners.ctypes.data, kind,
           np.ascontiguousarray(g[s]).ctypes.data if L.n_faces else work.ctypes.data, 3, work.ctypes.data, out[s].ctypes.data)
    return out[0] if np.ndim(pos) == 2 else out


def entries(tmpdir, L):
    """the neighbour relation as the reference walks it -> a namespace of int64 arrays, one element per entry, ordered by (f, j) and
    then in entry order: f, j (the edge that asks), g, jp (the entry), and n [F, 3] the number of entries of every (f, j)"""
    if not hasattr(L, "_entries"):
        fn = lib(tmpdir).er_entries
        cap = 3 * L.n_faces + 1
        g, jp = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        rows, n = [], np.zeros((L.n_faces, 3), np.int64)
        for f in range(L.n_faces):
            for j in range(3):
                n[f, j] = fn(L.faces.ctypes.data, L.off.ctypes.data, L.corners.ctypes.data, f, j, g.ctypes.data, jp.ctypes.data, cap)
                rows += [(f, j, int(g[e]), int(jp[e])) for e in range(n[f, j])]
        t = np.array(rows, np.int64).reshape(-1, 4)
        L._entries = types.SimpleNamespace(f=t[:, 0], j=t[:, 1], g=t[:, 2], jp=t[:, 3], n=n)
    return L._entries


# ------------------------------------------------------------------------------------------------ the derived bounds
# binary32 against binary64 over the same binary32 inputs.  An element that is a sum of terms, each of which passes through at most n
# roundings on its way into the result, is off by at most gamma_n * sum |term| (Higham, Accuracy and Stability, 3.1) — n counted
# from the rule, the sums of absolute terms evaluated in float64.  The binary64 evaluation's own rounding (2^-29 of these) and
# underflow (the tests' magnitudes are far from it) are not counted, as in normalsref and lapref.
def _edge_vectors(L, pos):
    """-> d [F, 3 (edge), 3] = p[b_j] - p[a_j] and its length [F, 3], in float64 from the float32 positions"""
    p = np.asarray(pos, np.float32).astype(np.float64)
    q = p[L.f]
    d = np.stack([q[:, (j + 2) % 3] - q[:, (j + 1) % 3] for j in range(3)], 1)
    return d, np.sqrt((d * d).sum(2))


def length_bound(L, pos):
    """LENGTH, pos [V, 3] -> the bound [F, 3].  A square d_c^2 carries its difference's rounding twice, the product's and at most two
    adds: dot3 is off by gamma_5 relative; the root does not grow a relative error (sqrt(1 + e) is within |e| of 1) and rounds once:
    |err| <= gamma_6 len"""
    return gamma(6) * _edge_vectors(L, pos)[1]


def length_grad_bound(L, pos, gout, e_gout=None):
    """LENGTH's backward, gout [F, 3] (binary32 values) -> the bound [V, 3] on gpos; e_gout [F, 3]: how far gout itself may be from
    the binary64 evaluation's (carried through: the backward is linear in gout).  len is off by gamma_6 relative (above), 1 / len by
    e_inv = (1 + u) / (1 - gamma_6) - 1, a component of u = d * inv by e_u = (1 + u)^2 (1 + e_inv) - 1 (the difference's and the
    product's rounding); a term g * u_c rounds once more and passes at most 2 m adds of acc, m = |list(v)|:
      |err| <= sum over the corner's two edges of |u_c| (|g| ((1 + e_u)(1 + gamma_(2m+1)) - 1) + e_g (1 + e_u)(1 + gamma_(2m+1)))"""
    d, ln = _edge_vectors(L, pos)
    g = np.abs(np.asarray(gout, np.float64))
    eg = np.zeros_like(g) if e_gout is None else np.asarray(e_gout, np.float64)
    e_inv = (1 + U) / (1 - gamma(6)) - 1
    e_u = (1 + U) ** 2 * (1 + e_inv) - 1
    with np.errstate(all="ignore"):
        u = np.where(ln[:, :, None] > 0, np.abs(d) / ln[:, :, None], 0.0)
    m = np.diff(L.off.astype(np.int64)).astype(np.float64)
    f = L.f
    out = np.zeros((L.n_verts, 3))
    for k in range(3):
        v = f[:, k]
        grow = ((1 + e_u) * (1 + gamma(2 * m[v] + 1)))[:, None]
        for j in ((k + 1) % 3, (k + 2) % 3):
            np.add.at(out, v, u[:, j] * (g[:, j, None] * (grow - 1) + eg[:, j, None] * grow))
    return out


def normals64(L, pos):
    """per face, in float64 from the float32 positions -> a namespace: ok [F] (the face is not skipped), zero [F] (every product of
    the cross product is zero: skipped by both evaluations), n [F, 3] the unit normal (zeros where skipped), dn [F, 3] a bound on
    |binary32 n - n| per component (inf where the two evaluations may disagree on `ok`), R [F] = 1 / |N|, e_r [F] the relative error
    of the binary32 r.  The derivation is lapref.cotan_weights64's, with e the edges (one rounded difference each):
      N's component = e1.y e2.z - e1.z e2.y: each product carries two rounded edges, its own rounding and the subtraction's: off by
        dN = gamma_4 A, A = |e1.y e2.z| + |e1.z e2.y|
      d2 = dot3(N, N): |d2 - D2| <= sum (2 |N| dN + dN^2)(1 + gamma_3) + gamma_3 D2;  rho = that / D2 must stay below 1/2 (else inf)
      r = 1 / sqrt(d2): (1 - rho)^(-1/2) <= 1 / (1 - rho), then the root's and the division's rounding: e_r = (1 + rho / (1 - rho))
        (1 + gamma_2) - 1
      n = N * r, one more rounding:  dn = R (dN (1 + e_r)(1 + u) + |N| ((1 + e_r)(1 + u) - 1))"""
    p = np.asarray(pos, np.float32).astype(np.float64)
    q = p[L.f]
    e1, e2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
    with np.errstate(all="ignore"):
        N = np.cross(e1, e2)
        A = np.abs(e1[:, [1, 2, 0]] * e2[:, [2, 0, 1]]) + np.abs(e1[:, [2, 0, 1]] * e2[:, [1, 2, 0]])
        dN = gamma(4) * A
        D2 = (N * N).sum(1)
        rho = ((2 * np.abs(N) * dN + dN * dN).sum(1) * (1 + gamma(3)) + gamma(3) * D2) / D2
        zero = A.sum(1) == 0
        ok = (D2 > 0) & (D2 <= np.finfo(np.float32).max)
        good = ok & (rho < 0.5)
        e_r = np.where(good, (1 + rho / (1 - rho)) * (1 + gamma(2)) - 1, 0.0)
        R = np.where(ok, 1.0 / np.sqrt(np.where(ok, D2, 1.0)), 0.0)
        grow = ((1 + e_r) * (1 + U))[:, None]
        n = np.where(ok[:, None], N * R[:, None], 0.0)
        dn = np.where(good[:, None], R[:, None] * (dN * grow + np.abs(N) * (grow - 1)), np.where(zero[:, None], 0.0, np.inf))
    return types.SimpleNamespace(ok=ok, zero=zero, good=good, n=n, dn=dn, R=R, e_r=e_r, p=p)


def _pairs(tmpdir, L, pos):
    """the entries with what the bounds need of each: E (entries), w (normals64), live [n] (both faces ok), sure [n] (both resolved
    or one exactly zero: the two evaluations agree on whether the term exists)"""
    E, w = entries(tmpdir, L), normals64(L, pos)
    live = w.ok[E.f] & w.ok[E.g]
    sure = (w.good[E.f] | w.zero[E.f]) & (w.good[E.g] | w.zero[E.g])
    return E, w, live, sure


def dihedral_bound(tmpdir, L, pos):
    """DIHEDRAL, pos [V, 3] -> the bound [F, 3] (inf where a face of the sum is not resolved).  A product n_f,c n_g,c is off by
    |n_f| dn_g + |n_g| dn_f + dn_f dn_g, rounds once and passes dot3's two adds (gamma_3); 1 - dot rounds once; a term passes at
    most m adds of acc, m the number of entries of (f, j):
      e_dot = sum_c (|n_f| dn_g + |n_g| dn_f + dn_f dn_g)(1 + gamma_3) + gamma_3 sum_c |n_f n_g|;  e_t = e_dot + u (|t| + e_dot)
      |err| <= sum over the entries of e_t (1 + gamma_m) + gamma_m |t|"""
    E, w, live, sure = _pairs(tmpdir, L, pos)
    nf, ng, dnf, dng = np.abs(w.n[E.f]), np.abs(w.n[E.g]), w.dn[E.f], w.dn[E.g]
    with np.errstate(invalid="ignore"):
        e_dot = (nf * dng + ng * dnf + dnf * dng).sum(1) * (1 + gamma(3)) + gamma(3) * (nf * ng).sum(1)
        t = np.abs(1.0 - (w.n[E.f] * w.n[E.g]).sum(1))
        gm = gamma(E.n[E.f, E.j])
        term = np.where(live & sure, (e_dot + U * (t + e_dot)) * (1 + gm) + gm * t, np.where(sure, 0.0, np.inf))
    out = np.zeros((L.n_faces, 3))
    np.add.at(out, (E.f, E.j), term)
    return out


def dihedral_grad_bound(tmpdir, L, pos, gout, e_gout=None):
    """DIHEDRAL's backward, gout [F, 3] (binary32 values), e_gout as in length_grad_bound -> the bound [V, 3] on gpos (inf at the
    vertices of a face whose sum meets a face that is not resolved).  Per face, M the number of its entries over the three edges,
    per component c:
      s = w[f][j] + w[g][j'] rounds once and carries e_s = e_gout[f][j] + e_gout[g][j'];  a term n_g,c s is off by dn_g and s' error,
      rounds once and passes at most M adds of H:
        eH_c = sum (|n_g,c| + dn_g,c)(|s| (1 + u) + e_s)(1 + gamma_(M+1)) - |n_g,c| |s|;   mH_c = sum |n_g,c| |s|  (>= |H_c|)
      t = dot3(n_f, H):  e_t = sum_c (dn_f,c (mH_c + eH_c) + |n_f,c| eH_c)(1 + gamma_3) + gamma_3 m_t,  m_t = sum_c |n_f,c| mH_c
      q_c = H_c - n_f,c t, two roundings:  e_q = (eH_c + dn_f,c (m_t + e_t) + |n_f,c| e_t)(1 + gamma_2) + gamma_2 m_q,
        m_q = mH_c + |n_f,c| m_t
      gN_c = q_c r, one rounding and r's e_r:  e_gN = R (e_q (1 + e_r)(1 + u) + m_q ((1 + e_r)(1 + u) - 1));  m_gN = R m_q
    Phase 2 is normalsref.grad_bound's last step with G = gN of one face: a corner's term component is e_i G_j - e_j G_i, e an edge
    (one rounded difference): each product is off by |e| eG + gamma_2 |e| (mG + eG), the subtraction and the list's adds bring
    gamma_(m+1) of the products' magnitudes |e| (mG + eG); eG, mG: the sums of e_gN, m_gN over the components"""
    E, w, live, sure = _pairs(tmpdir, L, pos)
    g = np.asarray(gout, np.float64)
    eg = np.zeros_like(g) if e_gout is None else np.asarray(e_gout, np.float64)
    F = L.n_faces
    M = E.n.sum(1).astype(np.float64)
    s, e_s = np.abs(g[E.f, E.j] + g[E.g, E.jp]), eg[E.f, E.j] + eg[E.g, E.jp]
    ng, dng = np.abs(w.n[E.g]), w.dn[E.g]
    with np.errstate(invalid="ignore"):
        eh = (ng + dng) * ((s * (1 + U) + e_s) * (1 + gamma(M[E.f] + 1)))[:, None] - ng * s[:, None]
        eh = np.where((live & sure)[:, None], eh, np.where(sure[:, None], 0.0, np.inf))
    eH, mH = np.zeros((F, 3)), np.zeros((F, 3))
    np.add.at(eH, E.f, eh)
    np.add.at(mH, E.f, np.where(live[:, None], ng * s[:, None], 0.0))
    nf, dnf = np.abs(w.n), np.where(w.ok[:, None], w.dn, 0.0)
    with np.errstate(invalid="ignore"):
        m_t = (nf * mH).sum(1)
        e_t = (dnf * (mH + eH) + nf * eH).sum(1) * (1 + gamma(3)) + gamma(3) * m_t
        m_q = mH + nf * m_t[:, None]
        e_q = (eH + dnf * (m_t + e_t)[:, None] + nf * e_t[:, None]) * (1 + gamma(2)) + gamma(2) * m_q
        grow = ((1 + w.e_r) * (1 + U))[:, None]
        e_gN = w.R[:, None] * (e_q * grow + m_q * (grow - 1))
        e_gN = np.where(w.ok[:, None], np.where(w.good[:, None], e_gN, np.inf), np.where(w.zero[:, None], 0.0, np.inf))
        eG, mG = e_gN.sum(1), np.where(w.ok, w.R * m_q.sum(1), 0.0)
    f, p = L.f, w.p
    m = np.diff(L.off.astype(np.int64)).astype(np.float64)
    out = np.zeros((L.n_verts, 3))
    for k, (i, j) in enumerate([(1, 2), (2, 0), (0, 1)]):  # the edge a corner's term crosses G with
        edge = np.abs(p[f[:, i]] - p[f[:, j]])
        two = edge[:, [1, 2, 0]] + edge[:, [2, 0, 1]]  # the two edge components that enter component c of a cross product
        with np.errstate(invalid="ignore"):
            term = two * (eG + gamma(2) * (mG + eG))[:, None] + gamma(m[f[:, k]] + 1)[:, None] * two * (mG + eG)[:, None]
            term = np.where(np.isinf(eG)[:, None], np.inf, np.where(two > 0, term, 0.0))
        np.add.at(out, f[:, k], term)
    return out


def bound(tmpdir, L, pos, kind):
    """the derived bound of forward(..., np.float32) against forward(..., np.float64), pos [V, 3]"""
    kind = KINDS.get(kind, kind)
    return length_bound(L, pos) if kind == LENGTH else dihedral_bound(tmpdir, L, pos)


def grad_bound(tmpdir, L, pos, kind, gout, e_gout=None):
    """the derived bound of backward(..., np.float32) against backward(..., np.float64), pos [V, 3], gout [F, 3]"""
    kind = KINDS.get(kind, kind)
    return length_grad_bound(L, pos, gout, e_gout) if kind == LENGTH else dihedral_grad_bound(tmpdir, L, pos, gout, e_gout)


# ------------------------------------------------------------------------------------------------ meshes of the tests' own
def two_faces(flipped=False):
    """two faces on the edge (0, 1), folded a little; flipped: the second face wound the other way -> (pos [4, 3], faces [2, 3])"""
    pos = np.float32([[0.1, 0.2, 0.3], [0.9, 0.25, 0.35], [0.45, 0.85, 0.4], [0.55, -0.4, 0.55]])
    return pos, np.array([[0, 1, 2], [0, 1, 3] if flipped else [1, 0, 3]], np.uint32)


def book():
    """three faces on the edge (0, 1): non-manifold, two entries per side -> (pos [5, 3], faces [3, 3])"""
    pos = np.float32([[0.1, 0.2, 0.3], [0.9, 0.25, 0.35], [0.45, 0.85, 0.4], [0.55, -0.4, 0.55], [0.5, 0.3, 1.1]])
    return pos, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.uint32)


def flat_collapsed():
    """vgkit.grid(8, 7, 4, jitter=0) in the plane z = 0.5 with ONE face collapsed to zero area: the top right corner vertex, which
    one face alone names, moved onto that face's first vertex -> (pos, faces, the collapsed face)"""
    import vgkit
    pos, faces = vgkit.grid(8, 7, 4, jitter=0)
    pos[:, 2] = 0.5
    corner = len(pos) - 1
    (face,) = np.flatnonzero((faces == corner).any(1))
    pos[corner] = pos[[v for v in faces[face] if v != corner][0]]
    return pos, faces, int(face)


def edge_dictionary(faces):
    """the adjacency built the usual way, independent of the corner lists: {frozenset(a, b): [(face, edge), ...] in face order} over
    the edges whose two ends differ"""
    table = {}
    for f, i in enumerate(np.asarray(faces, np.int64)):
        for j in range(3):
            a, b = int(i[(j + 1) % 3]), int(i[(j + 2) % 3])
            if a != b:
                table.setdefault(frozenset((a, b)), []).append((f, j))
    return table


def meshes():
    """the smallest meshes on which each branch can go wrong: name -> a function -> (pos, faces)"""
    import lapref
    import vgkit
    return {"single": vgkit.single, "pair": two_faces, "pair-flipped": lambda: two_faces(True), "book": book, "octa": lapref.octahedron4,
            "fan": lambda: vgkit.fan(70, 2), "grid257": lambda: vgkit.grid(16, 16, 3, extra=1), "flat": lambda: flat_collapsed()[:2]}


# ------------------------------------------------------------------------------------------------ an independent restatement
def pair_table(faces):
    """edge_dictionary as rows (f, j, g, j'): every ordered pair of DIFFERENT faces on one edge, by (f, j) and then in face order ->
    int64 [n, 4]"""
    table = edge_dictionary(faces)
    rows = []
    for f, i in enumerate(np.asarray(faces, np.int64)):
        for j in range(3):
            a, b = int(i[(j + 1) % 3]), int(i[(j + 2) % 3])
            rows += [(f, j, g, jp) for g, jp in table.get(frozenset((a, b)), []) if g != f] if a != b else []
    return np.array(rows, np.int64).reshape(-1, 4)


def torch_terms(pos, faces, pairs, kind):
    """the rules restated in torch ops over a host-built edge table, in pos' dtype and on its device, differentiable by torch: pos
    [V, 3], faces [F, 3] int64 and pairs [n, 4] int64 tensors (pair_table) -> [F, 3].  The sums are index_add's, in no stated order"""
    import torch
    q = pos[faces]  # [F, 3 (corner), 3]
    if kind in ("length", LENGTH):
        d = torch.stack([q[:, (j + 2) % 3] - q[:, (j + 1) % 3] for j in range(3)], 1)
        d2 = (d * d).sum(2)  # (an edge of zero length passes no gradient on: the rule skips it)
        return torch.where(d2 > 0, torch.sqrt(torch.where(d2 > 0, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    N = torch.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0], dim=1)
    d2 = (N * N).sum(1)
    ok = (d2 > 0) & (d2 <= torch.finfo(torch.float32).max)
    n = N / torch.sqrt(torch.where(ok, d2, torch.ones_like(d2)))[:, None]
    f, j, g = pairs[:, 0], pairs[:, 1], pairs[:, 2]
    live = ok[f] & ok[g]
    f, j, g = f[live], j[live], g[live]
    term = 1.0 - (n[f] * n[g]).sum(1)
    return torch.zeros(faces.shape[0] * 3, dtype=pos.dtype, device=pos.device).index_add(0, f * 3 + j, term).view(-1, 3)
