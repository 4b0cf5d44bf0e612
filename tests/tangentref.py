"""The test reference of the mesh tangents (srz_mesh_tangents / _grad) and of the normal-mapping pass (srz_frameset_normal_map /
_grad): tests/tangent_ref.c holds the arithmetic, stated once in a `real` type and built as binary32 — the rules themselves — and as
binary64.  Corner lists come from tests/normalsref.py's Lists.  Built and loaded like tests/lightref.py's library; nothing of the
product is involved.  Also here: the same rules in torch float64 ops (autograd differentiates them), and what the CPU and GPU tests
share."""
import ctypes as C

import numpy as np

from normalsref import Lists, same_or_nan  # noqa: F401  (re-exported: the tests take them from here)
from support import ref_lib

NAMED, NORMALISED, W_NEG = 1, 2, 4  # tangents_classify()'s vertex bits
OWNED, LIT, FRAME, MAPPED = 1, 2, 4, 8  # nm_classify()'s pixel bits
U = 2.0 ** -24
vp, u32 = C.c_void_p, C.c_uint32
SIGNATURES = {}
for _b in ("tr32_", "tr64_"):
    SIGNATURES[_b + "tangents"] = (None, [u32, vp, vp, vp, vp, vp, vp])
    SIGNATURES[_b + "tangents_classify"] = (None, [u32, vp, vp, vp, vp, vp, vp])
    SIGNATURES[_b + "tangents_grad"] = (None, [u32, vp, vp, vp, vp, vp, vp, vp, vp])
    SIGNATURES[_b + "nm_forward"] = (None, [C.c_size_t, u32, vp, vp, vp, vp, C.c_int, vp])
    SIGNATURES[_b + "nm_classify"] = (None, [C.c_size_t, u32, vp, vp, vp, vp, vp])
    SIGNATURES[_b + "nm_grad"] = (None, [C.c_size_t, u32, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp])


def lib(tmpdir):
    return ref_lib("tangent_ref", tmpdir, SIGNATURES)


def _fn(tmpdir, name, dtype):
    return getattr(lib(tmpdir), ("tr32_" if dtype == np.float32 else "tr64_") + name)


def _p(a):
    return a.ctypes.data if a is not None else None


# ------------------------------------------------------------------------------------------------ the mesh tangents
def _sets(pos, dtype):
    p = np.ascontiguousarray(pos, dtype)
    return p.reshape((1,) + p.shape) if p.ndim == 2 else p


def tangents(tmpdir, L, pos, uv, dtype=np.float32):
    """pos [V, 3] or [B, V, 3], uv [V, 2] (one set) -> the tangents and handedness [V, 4] or [B, V, 4] of dtype"""
    p, q = _sets(pos, dtype), np.ascontiguousarray(uv, dtype)
    assert q.shape == (L.n_verts, 2) and p.shape[1:] == (L.n_verts, 3)
    out = np.zeros(p.shape[:2] + (4,), dtype)
    for s in range(len(p)):
        _fn(tmpdir, "tangents", dtype)(L.n_verts, _p(L.faces), _p(L.off), _p(L.corners), _p(p[s]), _p(q), _p(out[s]))
    return out.reshape(np.shape(pos)[:-1] + (4,))


def tangents_classify(tmpdir, L, pos, uv):
    """one set, by the binary32 rule -> [V] uint8: NAMED | NORMALISED | W_NEG"""
    p, q = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(uv, np.float32)
    cls = np.zeros(L.n_verts, np.uint8)
    lib(tmpdir).tr32_tangents_classify(L.n_verts, _p(L.faces), _p(L.off), _p(L.corners), _p(p), _p(q), _p(cls))
    return cls


def tangents_grad(tmpdir, L, pos, uv, gtan, dtype=np.float32):
    """pos [V, 3] or [B, V, 3], gtan the same with 4 floats a vertex (w is never read) -> gpos in pos's shape"""
    p, g, q = _sets(pos, dtype), _sets(gtan, dtype), np.ascontiguousarray(uv, dtype)
    assert g.shape == p.shape[:2] + (4,)
    out, work = np.zeros_like(p), np.zeros_like(p)
    for s in range(len(p)):
        _fn(tmpdir, "tangents_grad", dtype)(L.n_verts, _p(L.faces), _p(L.off), _p(L.corners), _p(p[s]), _p(q), _p(g[s]), _p(work[s]), _p(out[s]))
    return out.reshape(np.shape(pos))


def torch_tangents(pos, uv, faces):
    """the tangent rule with torch ops in pos's dtype (torch's own order of operations): pos [V, 3], uv [V, 2], faces [F, 3] int64 ->
    [V, 3]; s is held (uv carries no gradient), a vertex whose sum has no positive finite length gives zeros.  Differentiable."""
    import torch
    p0, p1, p2 = pos[faces[:, 0]], pos[faces[:, 1]], pos[faces[:, 2]]
    q0, q1, q2 = uv[faces[:, 0]], uv[faces[:, 1]], uv[faces[:, 2]]
    d1, d2 = q1 - q0, q2 - q0
    det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
    s = torch.where(det < 0, -torch.ones_like(det), torch.ones_like(det))
    Tf = ((p1 - p0) * d2[:, 1:2] - (p2 - p0) * d1[:, 1:2]) * s[:, None]
    S = torch.zeros_like(pos)
    for k in range(3):
        S = S.index_add(0, faces[:, k], Tf)
    len2 = (S * S).sum(1, keepdim=True)
    ok = (len2.detach() > 0) & torch.isfinite(len2.detach())
    return torch.where(ok, S / torch.where(ok, len2, torch.ones_like(len2)).sqrt(), torch.zeros_like(S))


# ------------------------------------------------------------------------------------------------ the normal-mapping pass
def _planes(ids, nrm, tan, m, dtype):
    ids = np.ascontiguousarray(ids, np.uint32)
    nrm, tan, m = (np.ascontiguousarray(t, dtype) for t in (nrm, tan, m))
    assert nrm.shape == (3,) + ids.shape and tan.shape == (4,) + ids.shape and m.shape == (3,) + ids.shape
    return ids, nrm, tan, m


def _fresh(n_planes, shape, prefill, dtype):
    if prefill is None:
        return np.zeros((n_planes,) + shape, dtype)
    assert dtype == np.float32
    pre = np.broadcast_to(np.asarray(prefill, np.uint32), (n_planes,) + shape)
    return np.array(pre, np.uint32, copy=True, order="C").view(np.float32)


def nm_forward(tmpdir, n_tris, ids, nrm, tan, m, fused=True, prefill=None, dtype=np.float32):
    """ids [rows, W] uint32 (plane 1 of one frame's visibility buffer), nrm / m [3, rows, W], tan [4, rows, W] -> [3, rows, W] of dtype.
    prefill: the uint32 word(s) the float32 planes start from (not fused: nobody's words stay)"""
    ids, nrm, tan, m = _planes(ids, nrm, tan, m, dtype)
    out = _fresh(3, ids.shape, prefill, dtype)
    _fn(tmpdir, "nm_forward", dtype)(ids.size, n_tris, _p(ids), _p(nrm), _p(tan), _p(m), int(fused), _p(out))
    return out


def nm_classify(tmpdir, n_tris, ids, nrm, tan, m):
    """[rows, W] uint8 by the binary32 rule: OWNED | LIT | FRAME | MAPPED (each implies the ones before it)"""
    ids, nrm, tan, m = _planes(ids, nrm, tan, m, np.float32)
    cls = np.zeros(ids.shape, np.uint8)
    lib(tmpdir).tr32_nm_classify(ids.size, n_tris, _p(ids), _p(nrm), _p(tan), _p(m), _p(cls))
    return cls


def nm_grad(tmpdir, n_tris, ids, nrm, tan, m, gout, fused=True, prefill=None, want=(True, True, True), dtype=np.float32):
    """-> (gnrm [3, rows, W], gtan [4, rows, W], gm [3, rows, W]), None where `want` says so"""
    ids, nrm, tan, m = _planes(ids, nrm, tan, m, dtype)
    gout = np.ascontiguousarray(gout, dtype)
    assert gout.shape == nrm.shape
    outs = [(_fresh(n, ids.shape, prefill, dtype) if w else None) for n, w in zip((3, 4, 3), want)]
    _fn(tmpdir, "nm_grad", dtype)(ids.size, n_tris, _p(ids), _p(nrm), _p(tan), _p(m), _p(gout), int(fused), *[_p(o) for o in outs])
    return tuple(outs)


def torch_normal_map(nrm, tan, m):
    """the pass's rule on planes [..., 3 / 4 / 3, rows, W] with torch ops in the tensors' dtype (no fmaf, torch's own order), every
    pixel taken as owned.  Differentiable by autograd: the branches are held by torch.where on detached conditions."""
    import torch
    dot = lambda a, b: (a * b).sum(-3, keepdim=True)  # noqa: E731
    ok = lambda x: (x > 0) & (x < float("inf"))  # noqa: E731
    safe = lambda x, c: torch.where(c, x, torch.ones_like(x))  # noqa: E731
    t3, tw = tan[..., 0:3, :, :], tan[..., 3:4, :, :]
    nn = dot(nrm, nrm)
    lit = ok(nn.detach())
    N = nrm / safe(nn, lit).sqrt()
    Tp = t3 - N * dot(N, t3)
    tt = dot(Tp, Tp)
    frame = lit & ok(tt.detach())
    T = Tp / safe(tt, frame).sqrt()
    hw = torch.where(tw.detach() < 0, -torch.ones_like(tw), torch.ones_like(tw))
    B = torch.cross(N, T, dim=-3) * hw
    R = m[..., 0:1, :, :] * T + m[..., 1:2, :, :] * B + m[..., 2:3, :, :] * N
    rr = dot(R, R)
    mapped = frame & ok(rr.detach())
    out = torch.where(mapped, R / safe(rr, mapped).sqrt(), N)
    return torch.where(lit, out, torch.zeros_like(out))


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
def make_uv(pos, kind, seed=0):
    """a uv set [V, 2] float32 for positions pos [V, 3] in the unit cube: "affine" (a rotation, scale and offset of x, y), "sheared",
    "mirrored" (u runs against x), "random" (independent of the positions: faces of either sign, mirrored on about half of them),
    "equal" (every vertex the same uv: every det is 0)"""
    p = np.asarray(pos, np.float64)
    rng = np.random.default_rng([seed, len(p), 173])
    x, y = p[:, 0], p[:, 1]
    if kind == "affine":
        uv = np.stack([0.8 * x - 0.3 * y + 0.1, 0.3 * x + 0.8 * y + 0.05], 1)
    elif kind == "sheared":
        uv = np.stack([x + 0.7 * y, 0.9 * y + 0.02 * p[:, 2]], 1)
    elif kind == "mirrored":
        uv = np.stack([1.0 - x, y], 1)
    elif kind == "folded":  # (u folds back at x = 0.5: the faces of the right half are mirrored)
        uv = np.stack([0.5 - np.abs(x - 0.5) + 0.1 * y, 0.9 * y + 0.05], 1)
    elif kind == "random":
        uv = rng.uniform(0, 1, (len(p), 2))
    elif kind == "equal":
        uv = np.full((len(p), 2), 0.25)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(uv, np.float32)


def degenerate_face(uv, faces, face=0):
    """uv with the three corners of `face` given one and the same uv: that face's det and Tf are exactly 0"""
    uv = np.array(uv, np.float32, copy=True)
    f = np.asarray(faces).reshape(-1, 3)
    if len(f):
        uv[f[face]] = uv[f[face][0]]
    return uv


def make_planes(seed, shape):
    """(nrm, tan, m, gout): nrm, m, gout [3, rows, W], tan [4, rows, W] float32 — normals of any length facing +z, tangents of any
    length roughly along x (not orthogonal to the normal, w = +-1 half and half), m a decoded tangent-space normal around (0, 0, 1)
    with slopes up to about one, gout normal"""
    rng = np.random.default_rng([seed, *shape, 179])
    rows, W = shape
    nrm = rng.normal(0, 0.3, (3, rows, W))
    nrm[2] = np.abs(nrm[2]) + 0.6
    nrm *= rng.uniform(0.5, 3.0, (1, rows, W))
    tan = np.zeros((4, rows, W))
    tan[0:3] = rng.normal(0, 0.3, (3, rows, W))
    tan[0] = np.abs(tan[0]) + 0.6
    tan[0:3] *= rng.uniform(0.3, 2.0, (1, rows, W))
    tan[3] = np.where(rng.random((rows, W)) < 0.5, -1.0, 1.0)
    m = rng.normal(0, 0.5, (3, rows, W))
    m[2] = np.abs(m[2]) + 0.4
    gout = rng.normal(0, 1, (3, rows, W))
    return tuple(np.ascontiguousarray(t, np.float32) for t in (nrm, tan, m, gout))


BRANCH_KINDS = 8


def branch_planes(seed, shape):
    """make_planes with every branch of the rule driven by hand -> (nrm, tan, m, gout, kind); kind [rows, W] per pixel: 0 benign,
    1 a zero normal (+-0), 2 a NaN or inf normal, 3 the tangent exactly parallel to the normal (axis-aligned: Tp = 0 exactly), 4 a zero
    tangent, 5 m = (+-0, +-0, +-0) (R = 0), 6 a NaN in m or a NaN / inf tangent, 7 non-finite gout, w = -0.0 or NaN"""
    rng = np.random.default_rng([seed, *shape, 181])
    nrm, tan, m, gout = (np.array(t, np.float32) for t in make_planes(seed, shape))
    kind = rng.integers(0, BRANCH_KINDS, shape)
    pick = lambda vals, n: rng.choice(np.float32(vals), n)  # noqa: E731
    k = kind == 1
    nrm[:, k] = pick([0.0, -0.0], (3, int(k.sum())))
    k = kind == 2
    nrm[0, k] = pick([np.nan, np.inf, -np.inf, 3e38], int(k.sum()))
    k = kind == 3
    axis = rng.integers(0, 3, shape)
    for a in range(3):
        ka = k & (axis == a)
        nrm[:, ka], tan[0:3, ka] = 0.0, 0.0
        nrm[a, ka], tan[a, ka] = pick([2.0, -0.5, 1.0], int(ka.sum())), pick([3.0, -1.0, 0.25], int(ka.sum()))
    k = kind == 4
    tan[0:3, k] = pick([0.0, -0.0], (3, int(k.sum())))
    k = kind == 5
    m[:, k] = pick([0.0, -0.0], (3, int(k.sum())))
    k = kind == 6
    which = rng.integers(0, 3, shape)
    m[1, k & (which == 0)] = np.nan
    tan[1, k & (which == 1)] = np.nan
    tan[2, k & (which == 2)] = np.inf
    k = kind == 7
    hit = k[None] & (rng.random((3,) + shape) < 0.5)
    gout[hit] = pick([np.nan, np.inf, -np.inf, 3e38, -3e38], int(hit.sum()))
    tan[3, k] = pick([-0.0, np.nan, -2.0, 1e-40], int(k.sum()))
    return nrm, tan, m, gout, kind


def well_conditioned(nrm, tan, m, floor=0.05):
    """[rows, W] bool by the rule in float64: nn, tt (of the unit-length-normal projection, relative to |t|²) and rr at least `floor`:
    the pixel is away from every branch boundary and its normalisations are tame"""
    n, t, mm = np.float64(nrm), np.float64(tan)[0:3], np.float64(m)
    dot = lambda a, b: (a * b).sum(0)  # noqa: E731
    nn = dot(n, n)
    N = n / np.sqrt(np.maximum(nn, 1e-300))
    Tp = t - N * dot(N, t)
    tt = dot(Tp, Tp)
    rr = dot(mm, mm)  # (T, B, N orthonormal: |R|² = |m|²)
    return (nn >= floor) & (tt >= floor) & (rr >= floor) & np.isfinite(nn + tt + rr)
