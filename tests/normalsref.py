"""The test reference of the vertex normals and the per-vertex attributes (tests/normals_ref.c holds the four rules): normals of
position sets and their backward in float32, bit for bit; a sceneset's corner attributes and their backward, bit for bit.  It makes its
own corner lists.  Built and loaded like tests/posgradref.py's library; nothing of the product is involved.  Also here: the float64
restatements and the DERIVED rounding bounds tests/test_normals_ref.py holds the reference itself to."""
import ctypes as C

import numpy as np

from support import ref_lib

vp, u32 = C.c_void_p, C.c_uint32
SIGNATURES = {"nr_corner_lists": (None, [vp, u32, u32, vp, vp, vp]),
              "nr_normals": (None, [vp, u32, u32, vp, vp, vp, vp, u32, vp]),
              "nr_normals_grad": (None, [vp, u32, u32, vp, vp, vp, vp, u32, vp, vp]),
              "nr_corner_attr": (None, [vp, vp, u32, u32, u32, vp]),
              "nr_corner_attr_grad": (None, [vp, vp, vp, u32, u32, u32, vp])}
U = 2.0 ** -24


def lib(tmpdir):
    return ref_lib("normals_ref", tmpdir, SIGNATURES)


def gamma(n):
    """gamma_n = n u / (1 - n u): the relative error of n float32 roundings in a row"""
    n = np.asarray(n, np.float64) * U
    return n / (1.0 - n)


class Lists:
    """a face list [F, 3] over n_verts vertices with its corner lists: .faces (never an empty array: a pointer to pass), .n_faces, .off
    [n_verts + 1], .corners [3 F] — vertex v is named by corners[off[v]:off[v + 1]], each 3 * face + k, increasing"""

    def __init__(self, tmpdir, faces, n_verts):
        f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
        assert f.size == 0 or int(f.max()) < n_verts
        self.n_verts, self.n_faces = n_verts, len(f)
        self.faces = np.ascontiguousarray(np.concatenate([f.reshape(-1), np.zeros(3, np.uint32)]))
        self.off, self.corners = np.zeros(n_verts + 1, np.uint32), np.zeros(f.size + 1, np.uint32)
        scratch = np.zeros(max(1, n_verts), np.uint32)
        lib(tmpdir).nr_corner_lists(self.faces.ctypes.data, len(f), n_verts, self.off.ctypes.data, self.corners.ctypes.data, scratch.ctypes.data)

    @property
    def f(self):
        return self.faces[:3 * self.n_faces].reshape(-1, 3).astype(np.int64)


def _sets(pos):
    p = np.ascontiguousarray(pos, np.float32)
    return p.reshape((1,) + p.shape) if p.ndim == 2 else p


def normals(tmpdir, L, pos, want_mask=False):
    """pos [V, 3] or [B, V, 3] float32 -> the normals in the same shape (and, wanted, the bool mask of the normalised vertices)"""
    p = _sets(pos)
    out, mask = np.zeros_like(p), np.zeros(p.shape[:2], np.uint8)
    for s in range(len(p)):
        lib(tmpdir).nr_normals(p[s].ctypes.data, 3, L.n_verts, L.faces.ctypes.data, L.off.ctypes.data, L.corners.ctypes.data,
                               out[s].ctypes.data, 3, mask[s].ctypes.data)
    out, mask = out.reshape(np.shape(pos)), mask.reshape(np.shape(pos)[:-1]).astype(bool)
    return (out, mask) if want_mask else out


def normals_grad(tmpdir, L, pos, gnrm):
    """pos, gnrm [V, 3] or [B, V, 3] float32 -> gpos in the same shape"""
    p, g = _sets(pos), _sets(gnrm)
    assert p.shape == g.shape
    out, work = np.zeros_like(p), np.zeros_like(p)
    for s in range(len(p)):
        lib(tmpdir).nr_normals_grad(p[s].ctypes.data, 3, L.n_verts, L.faces.ctypes.data, L.off.ctypes.data, L.corners.ctypes.data,
                                    g[s].ctypes.data, 3, work[s].ctypes.data, out[s].ctypes.data)
    return out.reshape(np.shape(pos))


def corner_attr(tmpdir, frames, meshes, attrs, out):
    """frames: per frame its draws in draw order, each (mesh slot, face count); meshes: slot -> Lists; attrs: slot -> [V, C] or
    [n_frames, V, C] float32 (the slots that are laid out); out: [n_frames, T, 3, C] float32, written in place where a draw of a slot of
    `attrs` has a corner -> out"""
    assert out.dtype == np.float32 and out.flags.c_contiguous
    n_ch = out.shape[-1]
    for f, draws in enumerate(frames):
        first = 0
        for slot, nf in draws:
            if slot in attrs:
                a = np.ascontiguousarray(attrs[slot], np.float32)
                a = np.ascontiguousarray(a[f] if a.ndim == 3 else a)
                assert nf == meshes[slot].n_faces and first + nf <= out.shape[1] and a.shape == (meshes[slot].n_verts, n_ch)
                lib(tmpdir).nr_corner_attr(a.ctypes.data, meshes[slot].faces.ctypes.data, nf, n_ch, first, out[f].ctypes.data)
            first += nf
    return out


def corner_attr_grad(tmpdir, frames, L, slot, gout):
    """gout [n_frames, T, 3, C] float32 -> gattr [n_frames, V, C] float32 of mesh `slot` (its Lists L): zeros for a frame without it"""
    gout = np.ascontiguousarray(gout, np.float32)
    n_ch = gout.shape[-1]
    g = np.zeros((len(frames), L.n_verts, n_ch), np.float32)
    for f, draws in enumerate(frames):
        first = 0
        for s, nf in draws:
            if s == slot:
                assert nf == L.n_faces and first + nf <= gout.shape[1]
                lib(tmpdir).nr_corner_attr_grad(gout[f].ctypes.data, L.off.ctypes.data, L.corners.ctypes.data, L.n_verts, n_ch, first, g[f].ctypes.data)
            first += nf
    return g


# ------------------------------------------------------------------------------------------------ float64 and the derived bounds
def normals64(L, pos):
    """one set, pos [V, 3]: the rule evaluated in float64 from the float32 positions -> a namespace of what the bounds need: S [V, 3],
    len [V], n [V, 3] (zeros where len is 0), dS [V] a bound on the euclidean error of the float32 S, valence [V]"""
    import types
    p = np.asarray(pos, np.float32).astype(np.float64)
    f = L.f
    u, w = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
    N = np.cross(u, w)
    # |products| of every face component: the float32 value of a component is (u.y w.z (1 + d)^3 - u.z w.y (1 + d)^3)(1 + d): two
    # rounded differences and one rounded product each, one rounded subtraction; then it passes through at most m adds of the sum
    A = np.abs(u[:, [1, 2, 0]] * w[:, [2, 0, 1]]) + np.abs(u[:, [2, 0, 1]] * w[:, [1, 2, 0]])
    V = L.n_verts
    S, SA, val = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V)
    for k in range(3):
        np.add.at(S, f[:, k], N), np.add.at(SA, f[:, k], A), np.add.at(val, f[:, k], 1.0)
    dS = np.linalg.norm(gamma(val + 4)[:, None] * SA, axis=1)
    ln = np.linalg.norm(S, axis=1)
    with np.errstate(all="ignore"):
        n = np.where(ln[:, None] > 0, S / ln[:, None], 0.0)
    return types.SimpleNamespace(S=S, len=ln, n=n, dS=dS, valence=val, p=p, f=f)


def normals_bound(e):
    """per vertex, on every component of the float32 normal against e.n: || x/|x| - y/|y| || <= 2 |x - y| / |y| carries dS through the
    normalisation; the scale r = 1 / sqrt(dot3) adds gamma_3 / 2 (three rounded products and two adds of positive terms, halved by
    the root) + the root + the division, the product S * r one more: below gamma_6 of a unit vector.  inf where len is 0"""
    with np.errstate(all="ignore"):
        return np.where(e.len > 0, 2.0 * e.dS / e.len + gamma(6), np.inf)


def grad_bound(e, g):
    """per vertex and component, on the float32 gpos against the exact gradient at the float32 inputs; e = normals64(...), g [V, 3] the
    gradient of the normals.  Valid where every vertex that shares a face with v has dS < len / 2 (else inf).  With en = normals_bound
    (the error of n), er = dS / (len - dS) + gamma_6 (the relative error of r), G = |g|:
      d = dot3(n, g):  ed = en G + gamma_3 (1 + en) G
      t = g - n d, two roundings per component:  et = en G + ed + en ed + gamma_2 (G + (1 + en)(G + ed))
      gS = t r, one rounding:  egs = [et (1 + er)(1 + u) + G (er + u (1 + er))] / len,  |gS| <= G / len (1 + ...) =: mgs
      G3 = (gS0 + gS1) + gS2 of a face:  eG = sum egs + gamma_2 sum mgs,  |G3| <= sum mgs =: mG
      a corner's term component = e_i G3_j - e_j G3_i, e an edge (one rounded difference, |e| exact in float64): each product is off by
      |e| eG + gamma_2 |e| (mG + eG) (the edge's and the product's rounding), the subtraction and the valence's adds of the sum bring
      gamma_(valence + 1) of the products' magnitudes |e| (mG + eG)"""
    G = np.linalg.norm(np.asarray(g, np.float64), axis=1)
    with np.errstate(all="ignore"):
        ok = (e.len > 0) & (e.dS < 0.5 * e.len)
        en = np.where(ok, normals_bound(e), 0.0)
        er = np.where(ok, (1 + e.dS / (e.len - e.dS)) * (1 + gamma(6)) - 1, 0.0)
        ed = en * G + gamma(3) * (1 + en) * G
        et = en * G + ed + en * ed + gamma(2) * (G + (1 + en) * (G + ed))
        egs = np.where(ok, (et * (1 + er) * (1 + U) + G * (er + U * (1 + er))) / e.len, 0.0)
        mgs = np.where(ok, G / e.len, 0.0) + egs
    # (a vertex that is exactly degenerate passes nothing on in either evaluation; one that is nearly so makes the bound infinite)
    bad = (e.len > 0) & ~ok
    f, p = e.f, e.p
    eG, mG = egs[f].sum(1) + gamma(2) * mgs[f].sum(1), mgs[f].sum(1)
    eG = np.where(bad[f].any(1), np.inf, eG)
    out = np.zeros((len(p), 3))
    opposite = [(1, 2), (2, 0), (0, 1)]  # the edge a corner's term crosses G with
    for k, (i, j) in enumerate(opposite):
        edge = np.abs(p[f[:, i]] - p[f[:, j]])  # [F, 3]
        two = edge[:, [1, 2, 0]] + edge[:, [2, 0, 1]]  # the two edge components that enter component c of a cross product
        with np.errstate(invalid="ignore"):
            term = two * (eG + gamma(2) * (mG + eG))[:, None] + gamma(e.valence[f[:, k]] + 1)[:, None] * two * (mG + eG)[:, None]
        np.add.at(out, f[:, k], np.where(two > 0, term, 0.0))
    return out


# ------------------------------------------------------------------------------------------------ meshes of the tests' own
def soup(seed, n_verts=40, n_faces=90):
    """a random triangle soup over n_verts vertices in the unit cube (no face names a vertex twice) -> (pos [V, 3] float32, faces [F, 3])"""
    rng = np.random.default_rng([seed, 127])
    faces = np.array([rng.choice(n_verts, 3, replace=False) for _ in range(n_faces)], np.uint32)
    return rng.uniform(0, 1, (n_verts, 3)).astype(np.float32), faces


def edge_mesh():
    """19 vertices, 8 faces -> (pos, faces, normalised [19] bool): an ordinary face (0, 1, 2); a face that names a vertex twice
    (3, 3, 4); a collinear face (5, 6, 7) whose cross product is exactly zero; a face with a NaN position (8, 9, 10) whose vertex 9 a
    good face (9, 11, 12) shares; a face of 1e20 coordinates (13, 14, 15: the products overflow); a face of 1e-25 coordinates
    (16, 17, 18: the products underflow to zero).  Only 0, 1, 2, 11 and 12 are normalised"""
    pos = np.zeros((19, 3), np.float32)
    pos[0:3] = [[0.1, 0.2, 0.3], [0.9, 0.1, 0.4], [0.3, 0.8, 0.2]]
    pos[3:5] = [[0.5, 0.5, 0.5], [0.7, 0.2, 0.9]]
    pos[5:8] = [[0, 0, 0], [1, 1, 1], [2, 2, 2]]
    pos[8:11] = [[np.nan, 0.3, 0.1], [0.4, 0.6, 0.2], [0.8, 0.7, 0.5]]
    pos[11:13] = [[0.2, 0.9, 0.7], [0.6, 0.1, 0.8]]
    pos[13:16] = np.float32([[1, 2, 3], [4, 1, 2], [2, 5, 1]]) * np.float32(1e20)
    pos[16:19] = np.float32([[1, 2, 3], [4, 1, 2], [2, 5, 1]]) * np.float32(1e-25)
    faces = np.array([[0, 1, 2], [3, 3, 4], [5, 6, 7], [8, 9, 10], [9, 11, 12], [13, 14, 15], [16, 17, 18], [2, 0, 1]], np.uint32)
    ok = np.zeros(19, bool)
    ok[[0, 1, 2, 11, 12]] = True
    return pos, faces, ok


def same_or_nan(got, want):
    """bit for bit, except that a NaN must be a NaN on the other side (its sign and payload are the machine's) -> the mask of the
    elements that differ"""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    g_nan, w_nan = np.isnan(g), np.isnan(w)
    return (g_nan != w_nan) | (~g_nan & (g.view(np.uint32) != w.view(np.uint32)))
