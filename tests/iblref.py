"""The image-based-lighting passes' test reference (tests/ibl_ref.c holds the arithmetic, stated once in a `real` type and built as
binary32 — the rules themselves — and as binary64): reflect and its backward, the split-sum table, ibl and its backward with the
table's gradient accumulated in double with sum |term| and counts, and the branch every pixel took.  Built and loaded like
tests/microfacetref.py's library; nothing of the product is involved.  Also here: the same rules in torch float64 ops (autograd
differentiates them), an independent trigonometric quadrature of the table in numpy float64, and what the CPU and GPU tests share."""
import ctypes as C

import numpy as np

from support import ref_lib

OWNED, LIT, VIEW, NV_POS = 1, 2, 4, 8  # reflect_classify()'s bits
R_LOW, R_HIGH, M_LOW, M_HIGH, NV_LOW, NV_HIGH, LAST_CELL = 2, 4, 8, 16, 32, 64, 128  # ibl_classify()'s (with OWNED)
INV_PI, RMIN, RSPAN = float(np.float32(float.fromhex("0x1.45f306p-2"))), 0.0625, 0.9375
F004 = float(np.float32(0.04))
TABLE_MAX = 64
# binary32 against binary64 on well-conditioned pixels, MEASURED on the CPU (tests/test_ibl_ref.py prints them): every plane relative
# to the plane's largest magnitude.  The tests assert 8 x these, because seeds differ; the GPU chain test uses the same margin.
MEASURED_REFLECT, MEASURED_IBL = 5.7e-7, 1.18e-6
vp, u32, sz, ci = C.c_void_p, C.c_uint32, C.c_size_t, C.c_int
SIGNATURES = {}
for _b in ("ib32_", "ib64_"):
    SIGNATURES[_b + "reflect"] = (None, [sz, u32, vp, vp, vp, vp, ci, vp])
    SIGNATURES[_b + "reflect_grad"] = (None, [sz, u32, vp, vp, vp, vp, vp, ci, vp, vp])
    SIGNATURES[_b + "reflect_classify"] = (None, [sz, u32, vp, vp, vp, vp, vp])
    SIGNATURES[_b + "table"] = (None, [ci, ci, vp, vp])
    SIGNATURES[_b + "ibl"] = (None, [sz, u32, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp])
    SIGNATURES[_b + "ibl_grad"] = (None, [sz, u32, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp])
    SIGNATURES[_b + "ibl_classify"] = (None, [sz, u32, vp, vp, vp, ci, vp])


def lib(tmpdir):
    return ref_lib("ibl_ref", tmpdir, SIGNATURES)


def _fn(tmpdir, name, dtype):
    return getattr(lib(tmpdir), ("ib32_" if dtype == np.float32 else "ib64_") + name)


def _p(a):
    return a.ctypes.data if a is not None else None


def _planes(ids, dtype, **planes):
    """name=(array or None, plane count) → contiguous arrays of dtype, shapes checked against ids [rows, W]"""
    out = []
    for name, (t, k) in planes.items():
        if t is not None:
            t = np.ascontiguousarray(t, dtype)
            assert t.shape == (k,) + ids.shape, (name, t.shape, ids.shape)
        out.append(t)
    return out


def _fresh(k, ids, prefill, dtype):
    if prefill is None:
        return np.zeros((k,) + ids.shape, dtype)
    assert dtype == np.float32
    return np.array(prefill[:k], np.uint32, copy=True, order="C").view(np.float32)


# ------------------------------------------------------------------------------------------------ reflect
def reflect(tmpdir, n_tris, ids, nrm, pos, eye, fused=True, prefill=None, dtype=np.float32):
    """ids [rows, W] uint32, nrm / pos [3, rows, W], eye [3] → [4, rows, W] of dtype.  prefill: [4, rows, W] uint32 words the float32
    planes start from (not fused: nobody's words stay)."""
    ids = np.ascontiguousarray(ids, np.uint32)
    nrm, pos = _planes(ids, dtype, nrm=(nrm, 3), pos=(pos, 3))
    eye = np.ascontiguousarray(eye, dtype).reshape(3)
    out = _fresh(4, ids, prefill, dtype)
    _fn(tmpdir, "reflect", dtype)(ids.size, n_tris, _p(ids), _p(nrm), _p(pos), _p(eye), int(fused), _p(out))
    return out


def reflect_grad(tmpdir, n_tris, ids, nrm, pos, eye, gout, fused=True, prefill=None, dtype=np.float32):
    """→ (gnrm, gpos) [3, rows, W] each"""
    ids = np.ascontiguousarray(ids, np.uint32)
    nrm, pos, gout = _planes(ids, dtype, nrm=(nrm, 3), pos=(pos, 3), gout=(gout, 4))
    eye = np.ascontiguousarray(eye, dtype).reshape(3)
    gnrm, gpos = _fresh(3, ids, prefill, dtype), _fresh(3, ids, prefill, dtype)
    _fn(tmpdir, "reflect_grad", dtype)(ids.size, n_tris, _p(ids), _p(nrm), _p(pos), _p(eye), _p(gout), int(fused), _p(gnrm), _p(gpos))
    return gnrm, gpos


def reflect_classify(tmpdir, n_tris, ids, nrm, pos, eye):
    ids = np.ascontiguousarray(ids, np.uint32)
    nrm, pos = _planes(ids, np.float32, nrm=(nrm, 3), pos=(pos, 3))
    eye = np.ascontiguousarray(eye, np.float32).reshape(3)
    cls = np.zeros(ids.shape, np.uint8)
    lib(tmpdir).ib32_reflect_classify(ids.size, n_tris, _p(ids), _p(nrm), _p(pos), _p(eye), _p(cls))
    return cls


# ------------------------------------------------------------------------------------------------ the table
def table(tmpdir, n, m, dtype=np.float32, want_signs=False):
    """[n, n, 2] of dtype by the rule; want_signs: also the A sums of the two signs of hx apart [n, n, 2]"""
    tab = np.zeros((n, n, 2), dtype)
    signs = np.zeros((n, n, 2), dtype) if want_signs else None
    _fn(tmpdir, "table", dtype)(n, m, _p(tab), _p(signs))
    return (tab, signs) if want_signs else tab


def table_polar(n, n_theta=1536, n_phi=768):
    """the same integrals by an INDEPENDENT quadrature in numpy float64: over the LIGHT direction in spherical coordinates with cos,
    sin and arccos-free trigonometry — f_spec(l, v) (n.l) dl with D, Vs, F as microfacet states them, midpoint in cos(theta) and phi —,
    no half-vector substitution, no importance sampling → [n, n, 2].  Converges slowly at low roughness (the lobe is narrow): the
    callers compare where it has converged."""
    out = np.zeros((n, n, 2))
    mu = (np.arange(n_theta) + 0.5) / n_theta  # n.l, uniform in the cosine: dl = dmu dphi
    phi = (np.arange(n_phi) + 0.5) / n_phi * np.pi  # half the circle, mirrored
    st = np.sqrt(1 - mu * mu)
    lx, lz = st[:, None] * np.cos(phi)[None, :], mu[:, None] + 0 * phi[None, :]
    ly = st[:, None] * np.sin(phi)[None, :]
    for i in range(n):
        nv = i / (n - 1)
        vx = np.sqrt(max(0.0, 1 - nv * nv))
        for j in range(n):
            rc = RMIN + RSPAN * j / (n - 1)
            al = rc * rc
            a2, k = al * al, 0.5 * al
            hx, hy, hz = lx + vx, ly, lz + nv
            hn = np.sqrt(hx * hx + hy * hy + hz * hz)
            ok = hn > 1e-12
            hn = np.where(ok, hn, 1.0)
            nh, vh = hz / hn, (vx * hx + nv * hz) / hn
            t = nh * nh * (a2 - 1) + 1
            D = a2 / np.pi / (t * t)
            Vs = 0.25 / ((lz * (1 - k) + k) * (nv * (1 - k) + k))
            x5 = (1 - np.clip(vh, 0, 1)) ** 5
            f = np.where(ok & (nv > 0), D * Vs * lz, 0.0) * (2 * np.pi / (n_theta * n_phi))
            out[i, j] = (f * (1 - x5)).sum(), (f * x5).sum()
    return out


# ------------------------------------------------------------------------------------------------ ibl
def ibl(tmpdir, n_tris, ids, base, mat, nv, irr, spec, tab, fused=True, prefill=None, dtype=np.float32):
    """ids [rows, W] uint32, base [3, rows, W] or None, mat [2, ..], nv [1, ..], irr / spec [3, ..], tab [n, n, 2] → [3, rows, W]"""
    ids = np.ascontiguousarray(ids, np.uint32)
    base, mat, nv, irr, spec = _planes(ids, dtype, base=(base, 3), mat=(mat, 2), nv=(nv, 1), irr=(irr, 3), spec=(spec, 3))
    tab = np.ascontiguousarray(tab, dtype)
    assert tab.ndim == 3 and tab.shape[0] == tab.shape[1] and tab.shape[2] == 2 and 2 <= tab.shape[0] <= TABLE_MAX
    out = _fresh(3, ids, prefill, dtype)
    _fn(tmpdir, "ibl", dtype)(ids.size, n_tris, _p(ids), _p(base), _p(mat), _p(nv), _p(irr), _p(spec), _p(tab), tab.shape[0], int(fused), _p(out))
    return out


class TabGrad:
    """the table's gradient of any number of frames, accumulated in double: .gsum [n, n, 2] float64, .gabs the sums of |term|, .count
    the contributing pixels per word"""

    def __init__(self, n):
        self.gsum, self.gabs, self.count = np.zeros((n, n, 2)), np.zeros((n, n, 2)), np.zeros((n, n, 2), np.uint32)

    def bound(self, extra=1):
        """per word: gamma_n * sum |term|, gamma_n = n u / (1 - n u), u = 2^-24, n the word's contributing pixels + extra (the add
        into the caller's word): the bound of any summation tree, srz_frameset_texture_grad's own"""
        n = (self.count.astype(np.float64) + extra) * 2.0 ** -24
        return n / (1.0 - n) * self.gabs


def ibl_grad(tmpdir, n_tris, ids, base, mat, nv, irr, spec, tab, gout, into=None, fused=True, prefill=None, want_terms=False,
             dtype=np.float32):
    """one frame's share: adds into `into` (a TabGrad, or None) and returns (gbase, gmat, gnv, girr, gspec): [3 | 2 | 1 | 3 | 3, rows,
    W] (gbase None without base); with want_terms also the per-pixel terms [8, rows, W] and the cells [2, rows, W] int32"""
    ids = np.ascontiguousarray(ids, np.uint32)
    base, mat, nv, irr, spec, gout = _planes(ids, dtype, base=(base, 3), mat=(mat, 2), nv=(nv, 1), irr=(irr, 3), spec=(spec, 3), gout=(gout, 3))
    tab = np.ascontiguousarray(tab, dtype)
    gbase = _fresh(3, ids, prefill, dtype) if base is not None else None
    gmat, gnv, girr, gspec = (_fresh(k, ids, prefill, dtype) for k in (2, 1, 3, 3))
    terms = np.zeros((8,) + ids.shape, dtype) if want_terms else None
    cell = np.zeros((2,) + ids.shape, np.int32) if want_terms else None
    _fn(tmpdir, "ibl_grad", dtype)(ids.size, n_tris, _p(ids), _p(base), _p(mat), _p(nv), _p(irr), _p(spec), _p(tab), tab.shape[0], _p(gout),
                                   int(fused), _p(gbase), _p(gmat), _p(gnv), _p(girr), _p(gspec), _p(into.gsum) if into else None,
                                   _p(into.gabs) if into else None, _p(into.count) if into else None, _p(terms), _p(cell))
    return (gbase, gmat, gnv, girr, gspec) + ((terms, cell) if want_terms else ())


def ibl_classify(tmpdir, n_tris, ids, mat, nv, n):
    ids = np.ascontiguousarray(ids, np.uint32)
    mat, nv = _planes(ids, np.float32, mat=(mat, 2), nv=(nv, 1))
    cls = np.zeros(ids.shape, np.uint8)
    lib(tmpdir).ib32_ibl_classify(ids.size, n_tris, _p(ids), _p(mat), _p(nv), n, _p(cls))
    return cls


# ------------------------------------------------------------------------------------------------ the rules in torch ops
def _clamp(x, lo, hi):
    """lo where !(x > lo) (a NaN too), hi where !(x < hi), x inside: the gradient passes strictly inside only"""
    import torch
    xd, one = x.detach(), torch.ones((), dtype=x.dtype, device=x.device)
    return torch.where(xd > lo, torch.where(xd < hi, x, hi * one), lo * one)


def torch_reflect(nrm, pos, eye):
    """srz_frameset_reflect's rule on planes [n, 3, rows, W] with torch ops in the tensors' dtype (no fmaf, torch's own order of
    operations), every pixel taken as owned; eye [3] or [n, 3] → [n, 4, rows, W].  Differentiable by autograd."""
    import torch
    dot = lambda a, b: (a * b).sum(-3, keepdim=True)  # noqa: E731
    ok = lambda x: (x > 0) & (x < float("inf"))  # noqa: E731
    safe = lambda x, m: torch.where(m, x, torch.ones_like(x))  # noqa: E731
    zero = torch.zeros((), dtype=nrm.dtype, device=nrm.device)
    nn = dot(nrm, nrm)
    lit = ok(nn.detach())
    N = nrm / safe(nn, lit).sqrt()
    V = eye.reshape(-1, 3, 1, 1) - pos
    vv = dot(V, V)
    view = ok(vv.detach())
    Vd = V / safe(vv, view).sqrt()
    nv = dot(N, Vd)
    return torch.where(lit & view, torch.cat([2 * nv * N - Vd, nv], -3), zero)


def torch_ibl(base, mat, nv, irr, spec, tab):
    """srz_frameset_ibl's rule on planes [n, 3 | 2 | 1, rows, W] and tab [t, t, 2] with torch ops in the tensors' dtype, every pixel
    taken as owned; base may be None → [n, 3, rows, W].  Differentiable by autograd, with respect to tab too."""
    import torch
    t = tab.shape[0]
    base = torch.ones_like(irr) if base is None else base
    r, m = mat[..., 0:1, :, :], mat[..., 1:2, :, :]
    rc, mc, nvc = _clamp(r, RMIN, 1.0), _clamp(m, 0.0, 1.0), _clamp(nv, 0.0, 1.0)
    x, y = nvc * (t - 1), (rc - RMIN) * ((t - 1) / RSPAN)
    x0, y0 = x.detach().floor().clamp(max=t - 2).long(), y.detach().floor().clamp(max=t - 2).long()
    tx, ty = x - x0, y - y0
    val = []
    for e in range(2):
        te = tab[:, :, e]
        t00, t01, t10, t11 = te[x0, y0], te[x0, y0 + 1], te[x0 + 1, y0], te[x0 + 1, y0 + 1]
        top, bot = t00 + ty * (t01 - t00), t10 + ty * (t11 - t10)
        val.append(top + tx * (bot - top))
    F0 = mc * (base - F004) + F004
    return base * (1 - mc) * irr + spec * (F0 * val[0] + val[1])


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
def rand_ids(rng, n, h, w, tris, holes=True):
    """owner id words [n, h, w] uint32: a triangle index + 1, four in ten with the S class bit, one in ten nobody's (0)"""
    ids = rng.integers(1, tris + 1, (n, h, w)).astype(np.uint32)
    ids |= (rng.random((n, h, w)) < 0.4).astype(np.uint32) << 31
    if holes:
        ids[rng.random((n, h, w)) < 0.1] = 0
    return ids


def make_eye(seed, frames=None):
    """an eye in front of the scene (z in 3 .. 6, x / y within +-1) [3] (or [frames, 3]) float32, deterministic"""
    rng = np.random.default_rng([seed, 17])
    n = 1 if frames is None else frames
    eye = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(3, 6, n)], 1).astype(np.float32)
    return eye[0] if frames is None else eye


def reflect_planes(seed, shape):
    """(nrm, pos, gout): nrm / pos [3, rows, W], gout [4, rows, W] float32: normals of lengths 0.9 .. 3, tilted, facing +z (one in twenty
    away), positions on a rough sheet around z = 0 within +-1 in x / y, gout normal"""
    rng = np.random.default_rng([seed, *shape, 5])
    rows, W = shape
    nrm = rng.normal(0, 0.25, (3, rows, W))
    nrm[2] = np.abs(nrm[2]) + 0.6
    nrm *= rng.uniform(1.5, 4.0, (1, rows, W)) * np.where(rng.random((1, rows, W)) < 0.05, -1.0, 1.0)
    pos = rng.uniform(-1.0, 1.0, (3, rows, W))
    pos[2] *= 0.3
    gout = rng.normal(0, 1, (4, rows, W))
    return tuple(np.ascontiguousarray(t, np.float32) for t in (nrm, pos, gout))


def reflect_well_conditioned(nrm, pos, eye, floor=0.25):
    """[rows, W] bool by the rule in float64: nn and vv >= floor"""
    n, V = np.float64(nrm), np.float64(eye).reshape(3, 1, 1) - np.float64(pos)
    return ((n * n).sum(0) >= floor) & ((V * V).sum(0) >= floor)


def ibl_planes(seed, shape, t):
    """(base, mat, nv, irr, spec, gout) float32 for a table of side t: base in (0.1, 1), irr and spec in (0, 2), gout normal; nv,
    roughness and metallic one draw in eight beyond a clamp, in [-0.2, -0.03] or [1.03, 1.2] (both clamps of each are met), the others
    inside: metallic in (0.05, 0.95), nv and roughness a cell of the table drawn uniformly and a place in (0.05, 0.95) of it —
    coordinates drawn uniformly over [0, 1] would leave 4 % of a CELL, two thirds of a 17-table's pixels, within well_conditioned's
    0.02 of a cell boundary; the edges and boundaries themselves are the KATs' and the hostile case's"""
    rng = np.random.default_rng([seed, *shape, t, 9])
    rows, W = shape
    base, irr, spec = rng.uniform(0.1, 1.0, (3, rows, W)), rng.uniform(0.0, 2.0, (3, rows, W)), rng.uniform(0.0, 2.0, (3, rows, W))
    cell = lambda: (rng.integers(0, t - 1, (rows, W)) + rng.uniform(0.05, 0.95, (rows, W))) / (t - 1)  # noqa: E731
    beyond = lambda: np.where(rng.random((rows, W)) < 0.5, rng.uniform(-0.2, -0.03, (rows, W)), rng.uniform(1.03, 1.2, (rows, W)))  # noqa: E731
    wide = lambda inside: np.where(rng.random((rows, W)) < 0.125, beyond(), inside)  # noqa: E731
    nv = wide(cell())[None]
    mat = np.stack([wide(RMIN + RSPAN * cell()), wide(rng.uniform(0.05, 0.95, (rows, W)))])
    gout = rng.normal(0, 1, (3, rows, W))
    return tuple(np.ascontiguousarray(a, np.float32) for a in (base, mat, nv, irr, spec, gout))


def ibl_well_conditioned(mat, nv, t, edge=0.02):
    """[rows, W] bool in float64: nv, roughness and metallic at least `edge` away from their clamp edges, and the table coordinates of
    an unclamped nv / roughness at least `edge` away from a cell boundary"""
    mat, nv = np.float64(mat), np.float64(nv)[0]
    ok = np.ones(nv.shape, bool)
    for x, lo, scale in ((nv, 0.0, t - 1.0), (mat[0], RMIN, (t - 1) / RSPAN), (mat[1], 0.0, None)):
        ok &= (np.abs(x - lo) >= edge) & (np.abs(x - 1.0) >= edge)
        if scale is not None:
            c = (np.clip(x, lo, 1.0) - lo) * scale
            inside = (x > lo) & (x < 1.0)
            ok &= ~inside | (np.abs(c - np.round(c)) >= edge)
    return ok


def smooth_table(t, seed=3):
    """a table [t, t, 2] float32 that is NOT the BRDF's: smooth and positive, with another slope in every cell, so that a wrong cell,
    weight or axis shows"""
    rng = np.random.default_rng([seed, t])
    i, j = np.meshgrid(np.arange(t) / (t - 1), np.arange(t) / (t - 1), indexing="ij")
    a = 0.2 + 0.7 * i - 0.3 * j * j + 0.05 * rng.random((t, t))
    b = 0.1 + 0.25 * (1 - i) ** 2 + 0.1 * j + 0.05 * rng.random((t, t))
    return np.ascontiguousarray(np.stack([a, b], -1), np.float32)


SPECIALS = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0, 1e-40, -3e-42])
UNIT_EDGES = np.float32([0.0, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)), 1e-45, -1e-45,
                         -0.5, 7.0, np.nan, np.nan, np.inf, -np.inf, 1e-40, -3e-42, 3e38, -3e38])
R_EDGES = np.float32([RMIN, np.nextafter(np.float32(RMIN), np.float32(1)), np.nextafter(np.float32(RMIN), np.float32(0)), 0.03])
HOSTILE = dict(seed=43, n=2, h=64, w=96, tris=20, t=5)  # the hostile test's case: its branch counts are checked on the CPU, then it runs on the GPU
REFLECT_KINDS, IBL_KINDS = 7, 7


def hostile_reflect(seed, n, h, w, tris, **_):
    """(ids [n, h, w], eye [3], nrm, pos [n, 3, h, w], gout [n, 4, h, w], kind [n, h, w]): 0 benign (one in five facing away), 1 a zero
    normal (+-0), 2 a NaN, inf, 3e38 or all-subnormal normal, 3 the eye exactly at P, 4 vv overflowing to inf, 5 N = Vd exactly (P on
    the vertical line under the eye, the normal (0, 0, s), s a power of two), 6 non-finite or subnormal position words and gout"""
    rng = np.random.default_rng([seed, 1])
    ids = rand_ids(rng, n, h, w, tris)
    eye = np.float32([0.5, 0.25, 4.0])
    nrm, pos, gout = (np.stack(t) for t in zip(*(reflect_planes(int(rng.integers(1 << 30)), (h, w)) for _ in range(n))))
    kind = rng.integers(0, REFLECT_KINDS, (n, h, w))

    def put(plane, mask, values):
        for c in range(plane.shape[1]):
            plane[:, c][mask] = values[c] if np.ndim(values) else values
    flip = (kind == 0) & (rng.random(kind.shape) < 0.2)
    for c in range(3):
        nrm[:, c][flip] = -np.abs(nrm[:, c][flip])
    z = kind == 1
    for c in range(3):
        nrm[:, c][z] = rng.choice(np.float32([0.0, -0.0]), int(z.sum()))
    s, what = kind == 2, rng.integers(0, 4, kind.shape)
    nrm[:, 0][s & (what == 0)] = np.nan
    nrm[:, 1][s & (what == 1)] = rng.choice(np.float32([np.inf, -np.inf, 3e38]), int((s & (what == 1)).sum()))
    sub = s & (what == 2)
    for c in range(3):
        nrm[:, c][sub] = (rng.integers(-2000, 2001, int(sub.sum())) * np.float64(2.0 ** -149)).astype(np.float32)
    nrm[:, 0][s & (what == 3)] = np.float32(1e-40)  # one subnormal component among ordinary ones: lit
    put(pos, kind == 3, eye)
    k4 = kind == 4
    for c in range(3):
        pos[:, c][k4] = rng.choice(np.float32([1.5e19, -2e19, 3e25]), int(k4.sum()))
    k5 = kind == 5
    put(pos, k5, np.float32([eye[0], eye[1], 0.0]))
    pos[:, 2][k5] = rng.choice(np.float32([0.0, 2.0, -4.0]), int(k5.sum()))
    put(nrm, k5, np.float32([0.0, 0.0, 1.0]))
    nrm[:, 2][k5] = rng.choice(np.float32([0.5, 1.0, 2.0, 4.0]), int(k5.sum()))
    k6 = kind == 6
    for t in (pos, gout):
        hit = k6[:, None] & (rng.random(t.shape) < 0.4)
        t[hit] = SPECIALS[rng.integers(0, len(SPECIALS), int(hit.sum()))]
    return ids, eye, nrm, pos, gout, kind


def reflect_branches(tmpdir, tris, ids, eye, nrm, pos, gout, kind):
    """name -> bool mask over [n, h, w] of every branch of reflect_classify, and of the hostile values that take no branch of their own"""
    own = ((ids & 0x7fffffff) - np.uint32(1)) < tris
    cls = np.stack([reflect_classify(tmpdir, tris, ids[i], nrm[i], pos[i], eye) for i in range(len(ids))])
    lit, view = (cls & LIT) != 0, (cls & VIEW) != 0
    return {"nobody": ~own, "not lit": own & ~lit, "lit": lit, "no view": lit & ~view, "view": view, "nv > 0": (cls & NV_POS) != 0,
            "nv <= 0": view & ((cls & NV_POS) == 0), "eye at P": own & lit & (kind == 3), "vv overflows": own & lit & (kind == 4),
            "N = Vd": view & (kind == 5), "non-finite position": own & lit & ~np.isfinite(pos).all(1),
            "non-finite gout": own & view & ~np.isfinite(gout).all(1),
            "subnormal words": own & (((np.abs(pos) < 1e-38) & (pos != 0)).any(1) | ((np.abs(nrm) < 1e-38) & (nrm != 0)).any(1))}


def hostile_table(t, rng):
    """smooth_table with NaN, +-inf, 3e38 and subnormal words put into one word in six"""
    tab = smooth_table(t).copy()
    hit = rng.random(tab.shape) < 1 / 6
    tab[hit] = SPECIALS[rng.integers(0, len(SPECIALS), int(hit.sum()))]
    return tab


def hostile_ibl(seed, n, h, w, tris, t, **_):
    """(ids [n, h, w], tab [t, t, 2] with special words, base, mat, nv, irr, spec, gout stacked over the n frames, kind [n, h, w]): 0
    benign, 1 nv at or beyond a clamp edge or special (UNIT_EDGES), 2 roughness the same (UNIT_EDGES and R_EDGES), 3 metallic the
    same, 4 nv exactly on a cell boundary i / (t - 1), 5 roughness exactly on a node RMIN + RSPAN j / (t - 1) as float32 has it, 6
    special words in base, irr, spec and gout"""
    rng = np.random.default_rng([seed, 2])
    ids = rand_ids(rng, n, h, w, tris)
    tab = hostile_table(t, rng)
    base, mat, nv, irr, spec, gout = (np.stack(a) for a in zip(*(ibl_planes(int(rng.integers(1 << 30)), (h, w), t) for _ in range(n))))
    kind = rng.integers(0, IBL_KINDS, (n, h, w))
    r_edges = np.concatenate([UNIT_EDGES, R_EDGES])
    for k, plane, values in ((1, nv[:, 0], UNIT_EDGES), (2, mat[:, 0], r_edges), (3, mat[:, 1], UNIT_EDGES)):
        hit = kind == k
        plane[hit] = values[rng.integers(0, len(values), int(hit.sum()))]
    k4 = kind == 4
    nv[:, 0][k4] = (rng.integers(0, t, int(k4.sum())) / np.float32(t - 1)).astype(np.float32)
    k5 = kind == 5
    mat[:, 0][k5] = (np.float32(RMIN) + np.float32(RSPAN) * (rng.integers(0, t, int(k5.sum())) / np.float32(t - 1)).astype(np.float32)).astype(np.float32)
    k6 = kind == 6
    for a in (base, irr, spec, gout):
        hit = k6[:, None] & (rng.random(a.shape) < 0.4)
        a[hit] = SPECIALS[rng.integers(0, len(SPECIALS), int(hit.sum()))]
    return ids, tab, base, mat, nv, irr, spec, gout, kind


def ibl_branches(tmpdir, tris, ids, tab, base, mat, nv, irr, spec, gout, kind):
    """name -> bool mask over [n, h, w] of every branch of ibl_classify, and of the hostile values that take no branch of their own"""
    t = tab.shape[0]
    own = ((ids & 0x7fffffff) - np.uint32(1)) < tris
    cls = np.stack([ibl_classify(tmpdir, tris, ids[i], mat[i], nv[i], t) for i in range(len(ids))])
    bit = lambda b: own & ((cls & b) != 0)  # noqa: E731
    special = lambda a: own & ~np.isfinite(a).all(1)  # noqa: E731
    r, m, v = mat[:, 0], mat[:, 1], nv[:, 0]
    x = np.float32(np.clip(v, 0, 1)) * np.float32(t - 1)
    return {"nobody": ~own, "owned": own, "roughness at or below RMIN": bit(R_LOW), "roughness at or above 1": bit(R_HIGH),
            "roughness inside": own & ((cls & (R_LOW | R_HIGH)) == 0), "metallic at or below 0": bit(M_LOW), "metallic at or above 1": bit(M_HIGH),
            "metallic inside": own & ((cls & (M_LOW | M_HIGH)) == 0), "nv at or below 0": bit(NV_LOW), "nv at or above 1": bit(NV_HIGH),
            "nv inside": own & ((cls & (NV_LOW | NV_HIGH)) == 0), "the last cell by the min": bit(LAST_CELL),
            "roughness NaN": own & np.isnan(r), "metallic NaN": own & np.isnan(m), "nv NaN": own & np.isnan(v),
            "roughness +-inf": own & np.isinf(r), "metallic +-inf": own & np.isinf(m), "nv +-inf": own & np.isinf(v),
            "a subnormal coordinate": own & (((np.abs(mat) < 1e-38) & (mat != 0)).any(1) | ((np.abs(v) < 1e-38) & (v != 0))),
            "nv on a cell boundary": own & (kind == 4) & (x == np.floor(x)), "roughness on a node": own & (kind == 5),
            "non-finite base": special(base), "non-finite irr": special(irr), "non-finite spec": special(spec), "non-finite gout": special(gout),
            "a special table word in the cell": own & (kind == 0) & ~np.isfinite(ibl_cell_words(tab, mat, nv)).all(-1)}


def ibl_cell_words(tab, mat, nv):
    """[n, h, w, 8]: the eight table words of every pixel's cell, by the binary32 rule restated in numpy"""
    t = tab.shape[0]
    r, v = np.float32(mat[:, 0]), np.float32(nv[:, 0])
    with np.errstate(invalid="ignore"):
        rc = np.where(r > np.float32(RMIN), np.where(r < 1, r, np.float32(1)), np.float32(RMIN)).astype(np.float32)
        vc = np.where(v > 0, np.where(v < 1, v, np.float32(1)), np.float32(0)).astype(np.float32)
    x, y = vc * np.float32(t - 1), (rc - np.float32(RMIN)) * (np.float32(t - 1) / np.float32(RSPAN))
    x0, y0 = np.minimum(np.floor(x).astype(int), t - 2), np.minimum(np.floor(y).astype(int), t - 2)
    return np.concatenate([tab[x0, y0], tab[x0, y0 + 1], tab[x0 + 1, y0], tab[x0 + 1, y0 + 1]], -1)
