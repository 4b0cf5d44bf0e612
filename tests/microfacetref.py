"""The Cook-Torrance pass's test reference (tests/microfacet_ref.c holds the arithmetic, stated once in a `real` type and built as
binary32 — the rule itself — and as binary64): per pixel (owner id word, normal, position, base colour, roughness and metallic) and a
parameter frame (eye amb, then per light pos intensity) → the colour planes; backward, the gradient planes and the parameter gradient
accumulated in double with sum |term| and counts; and the branch every pixel took.  Built and loaded like tests/lightref.py's library;
nothing of the product is involved.  Also here: the same rule in torch float64 ops (autograd differentiates it), and what the CPU and
GPU tests share."""
import ctypes as C

import numpy as np

from support import ref_lib

OWNED, LIT, VIEW, NV_POS = 1, 2, 4, 8  # classify()'s pixel bits
R_LOW, R_HIGH, M_LOW, M_HIGH, R_NAN, M_NAN = 1, 2, 4, 8, 16, 32  # its material bits (of lit pixels)
SKIPPED, FACING, SPEC, NH_IN, VH_IN, REACHED = 1, 2, 4, 8, 16, 32  # and its per-light bits
LIGHT_MAX = 8
INV_PI, RMIN = float(np.float32(float.fromhex("0x1.45f306p-2"))), 0.0625
vp = C.c_void_p
_head = [C.c_size_t, C.c_uint32, vp, vp, vp, vp, vp, vp, C.c_int]
SIGNATURES = {}
for _b in ("mr32_", "mr64_"):
    SIGNATURES[_b + "forward"] = (None, _head + [C.c_int, vp])
    SIGNATURES[_b + "grad"] = (None, _head + [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp])
    SIGNATURES[_b + "classify"] = (None, [C.c_size_t, C.c_uint32, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp])


def par_len(n_lights):
    return 6 + 6 * n_lights


def lib(tmpdir):
    return ref_lib("microfacet_ref", tmpdir, SIGNATURES)


def _args(ids, nrm, pos, base, mat, par, dtype):
    ids = np.ascontiguousarray(ids, np.uint32)
    planes = [None if t is None else np.ascontiguousarray(t, dtype) for t in (nrm, pos, base)]
    for t in planes:
        assert t is None or t.shape == (3,) + ids.shape, (t.shape, ids.shape)
    mat = np.ascontiguousarray(mat, dtype)
    assert mat.shape == (2,) + ids.shape, (mat.shape, ids.shape)
    par = np.ascontiguousarray(par, dtype).reshape(-1)
    n_lights = (len(par) - 6) // 6
    assert 1 <= n_lights <= LIGHT_MAX and len(par) == par_len(n_lights)
    return ids, planes, mat, par, n_lights


def _p(a):
    return a.ctypes.data if a is not None else None


def forward(tmpdir, n_tris, ids, nrm, pos, base, mat, par, fused=True, prefill=None, dtype=np.float32):
    """ids [rows, W] uint32 (plane 1 of one frame's visibility buffer), nrm / pos / base [3, rows, W] (base may be None), mat
    [2, rows, W], par [6 + 6 L] → [3, rows, W] of dtype.  prefill: [3, rows, W] uint32 words the float32 planes start from (not fused:
    nobody's words stay)."""
    ids, (nrm, pos, base), mat, par, L = _args(ids, nrm, pos, base, mat, par, dtype)
    if prefill is None:
        out = np.zeros((3,) + ids.shape, dtype)
    else:
        assert dtype == np.float32
        out = np.array(prefill, np.uint32, copy=True, order="C").view(np.float32)
    fn = lib(tmpdir).mr32_forward if dtype == np.float32 else lib(tmpdir).mr64_forward
    fn(ids.size, n_tris, _p(ids), _p(nrm), _p(pos), _p(base), _p(mat), _p(par), L, int(fused), _p(out))
    return out


class Grad:
    """the parameter gradient of any number of frames, accumulated in double: .gsum [K] float64, .gabs the sums of |term|, .count [K]
    the contributing pixels per entry"""

    def __init__(self, n_lights):
        K = par_len(n_lights)
        self.gsum, self.gabs, self.count = np.zeros(K, np.float64), np.zeros(K, np.float64), np.zeros(K, np.uint32)

    def bound(self, extra=0):
        """per entry: gamma_n * sum |term|, gamma_n = n u / (1 - n u), u = 2^-24, n the entry's contributing pixels (+ extra: further
        roundings of the same sum, such as adding the ranks' or frames' partial results): the bound of any summation tree"""
        n = (self.count.astype(np.float64) + extra) * 2.0 ** -24
        return n / (1.0 - n) * self.gabs


def grad(tmpdir, n_tris, ids, nrm, pos, base, mat, par, gout, into=None, fused=True, prefill=None, want_terms=False, dtype=np.float32):
    """one frame's share: adds into `into` (a Grad, or None) and returns (gnrm, gpos, gbase, gmat): [3, rows, W] each (gbase None
    without base), gmat [2, rows, W]; and with want_terms the per-pixel terms [K, rows, W]"""
    ids, (nrm, pos, base), mat, par, L = _args(ids, nrm, pos, base, mat, par, dtype)
    gout = np.ascontiguousarray(gout, dtype)
    assert gout.shape == nrm.shape

    def fresh(n=3):
        if prefill is None:
            return np.zeros((n,) + ids.shape, dtype)
        assert dtype == np.float32
        return np.array(prefill[:n], np.uint32, copy=True, order="C").view(np.float32)
    gnrm, gpos, gbase, gmat = fresh(), fresh(), (fresh() if base is not None else None), fresh(2)
    terms = np.zeros((par_len(L),) + ids.shape, dtype) if want_terms else None
    fn = lib(tmpdir).mr32_grad if dtype == np.float32 else lib(tmpdir).mr64_grad
    fn(ids.size, n_tris, _p(ids), _p(nrm), _p(pos), _p(base), _p(mat), _p(par), L, _p(gout), int(fused), _p(gnrm), _p(gpos), _p(gbase),
       _p(gmat), _p(into.gsum) if into else None, _p(into.gabs) if into else None, _p(into.count) if into else None, _p(terms))
    return (gnrm, gpos, gbase, gmat, terms) if want_terms else (gnrm, gpos, gbase, gmat)


def classify(tmpdir, n_tris, ids, nrm, pos, mat, par):
    """([rows, W] uint8: OWNED | LIT | VIEW | NV_POS, [rows, W] uint8: the material's R_* / M_* bits, [L, rows, W] uint8: REACHED |
    SKIPPED | FACING | SPEC | NH_IN | VH_IN) by the binary32 rule"""
    ids, (nrm, pos, _), mat, par, L = _args(ids, nrm, pos, None, mat, par, np.float32)
    cls, mcls, lcls = np.zeros(ids.shape, np.uint8), np.zeros(ids.shape, np.uint8), np.zeros((L,) + ids.shape, np.uint8)
    lib(tmpdir).mr32_classify(ids.size, n_tris, _p(ids), _p(nrm), _p(pos), _p(mat), _p(par), L, _p(cls), _p(mcls), _p(lcls))
    return cls, mcls, lcls


# ------------------------------------------------------------------------------------------------ the rule in torch float64 ops
def torch_rule(nrm, pos, base, mat, lights, eye, amb):
    """the rule of include/srz.h on planes [..., 3, rows, W] (mat [..., 2, rows, W]) with torch ops in the tensors' dtype (no fmaf,
    torch's own order of operations), every pixel taken as owned; lights [L, 6], eye / amb [3].  Differentiable by autograd: the
    branches and clamps are held by torch.where on detached conditions, exactly the derivative the backward states."""
    import torch
    v3 = lambda t: t.reshape(3, 1, 1)  # noqa: E731
    dot = lambda a, b: (a * b).sum(-3, keepdim=True)  # noqa: E731
    ok = lambda x: (x > 0) & (x < float("inf"))  # noqa: E731
    zero = torch.zeros((), dtype=nrm.dtype, device=nrm.device)
    one = torch.ones((), dtype=nrm.dtype, device=nrm.device)
    safe = lambda x, m: torch.where(m, x, torch.ones_like(x))  # noqa: E731

    def clamp(x, lo, hi):  # lo where !(x > lo) (a NaN too), hi where !(x < hi), x inside: the gradient passes inside only
        xd = x.detach()
        return torch.where(xd > lo, torch.where(xd < hi, x, hi * one), lo * one)
    nn = dot(nrm, nrm)
    lit = ok(nn.detach())
    N = nrm / safe(nn, lit).sqrt()
    V = v3(eye) - pos
    vv = dot(V, V)
    view = ok(vv.detach())
    Vd = torch.where(view, V / safe(vv, view).sqrt(), zero)
    base = torch.ones_like(nrm) if base is None else base
    r, m = mat[..., 0:1, :, :], mat[..., 1:2, :, :]
    rc, mc = clamp(r, RMIN, 1.0), clamp(m, 0.0, 1.0)
    al = rc * rc
    a2 = al * al
    k = 0.5 * al
    F0 = mc * (base - float(np.float32(0.04))) + float(np.float32(0.04))
    cdif = base * (1 - mc)
    nv = torch.where(view, dot(N, Vd), zero)
    acc = torch.zeros_like(nrm)
    for l in range(lights.shape[0]):
        lpos, I = v3(lights[l, :3]), v3(lights[l, 3:])
        Lv = lpos - pos
        r2 = dot(Lv, Lv)
        on = ok(r2.detach())
        r2s = safe(r2, on)
        Ld = Lv / r2s.sqrt()
        E = I / r2s
        nl = dot(N, Ld)
        on = on & (nl.detach() > 0)
        Hs = Ld + Vd
        h2 = dot(Hs, Hs)
        spec = view & (h2.detach() > 0) & (nv.detach() > 0)
        H = Hs / safe(h2, spec).sqrt()
        nh, vh = clamp(dot(N, H), 0.0, 1.0), clamp(dot(Vd, H), 0.0, 1.0)
        t = nh * nh * (a2 - 1) + 1
        D = a2 * INV_PI / (t * t)
        gl, gv = nl * (1 - k) + k, nv * (1 - k) + k
        Vs = 0.25 / safe(gl * gv, spec & on)
        F = (1 - F0) * (1 - vh) ** 5 + F0
        f = torch.where(spec, cdif * INV_PI * (1 - F) + F * (D * Vs), cdif * INV_PI)
        acc = acc + torch.where(on, f * E * nl, zero)
    return torch.where(lit, v3(amb) * base + acc, zero)


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
def make_params(seed, n_lights, frames=None):
    """a parameter block [6 + 6 L] (or [frames, ...]) float32: the eye and the lights in front of the scene (z in 3 .. 6, x / y within
    +-2), amb and the intensities positive, deterministic"""
    rng = np.random.default_rng([seed, n_lights, 3])
    n = 1 if frames is None else frames
    par = np.zeros((n, par_len(n_lights)), np.float32)
    par[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    par[:, 2] = rng.uniform(3, 6, n)
    par[:, 3:6] = rng.uniform(0.02, 0.2, (n, 3))
    L = par[:, 6:].reshape(n, n_lights, 6)
    L[:, :, 0:2] = rng.uniform(-2, 2, (n, n_lights, 2))
    L[:, :, 2] = rng.uniform(3, 6, (n, n_lights))
    L[:, :, 3:6] = rng.uniform(2, 20, (n, n_lights, 3))
    return par[0] if frames is None else par


def make_planes(seed, shape):
    """(nrm, pos, base, mat, gout): [3, rows, W] float32 each, mat [2, rows, W]: normals of any length, tilted, facing +z (one in
    twenty: away), positions on a rough sheet around z = 0 within +-1 in x / y, base colour in (0.1, 1), roughness and metallic over
    [-0.1, 1.1] (both clamps of both are met), gout normal"""
    rng = np.random.default_rng([seed, *shape, 3])
    rows, W = shape
    nrm = rng.normal(0, 0.25, (3, rows, W))
    nrm[2] = np.abs(nrm[2]) + 0.6
    nrm *= rng.uniform(0.5, 3.0, (1, rows, W)) * np.where(rng.random((1, rows, W)) < 0.05, -1.0, 1.0)  # (one in twenty faces away)
    pos = rng.uniform(-1.0, 1.0, (3, rows, W))
    pos[2] *= 0.3
    base = rng.uniform(0.1, 1.0, (3, rows, W))
    # one draw in four over the whole of [-0.1, 1.1], the others inside (0.1, 0.95): drawn uniformly over the whole range, 6.7 % of each
    # plane would lie within well_conditioned's 0.02 of a clamp edge — 13 % of the pixels, more than the one in ten it may leave out
    mat = np.where(rng.random((2, rows, W)) < 0.25, rng.uniform(-0.1, 1.1, (2, rows, W)), rng.uniform(0.1, 0.95, (2, rows, W)))
    gout = rng.normal(0, 1, (3, rows, W))
    return tuple(np.ascontiguousarray(t, np.float32) for t in (nrm, pos, base, mat, gout))


def well_conditioned(nrm, pos, mat, par, margin=0.05, floor=0.25, edge=0.02):
    """[rows, W] bool by the rule in float64: nn, vv, every r2 and h2 >= floor, every raw cosine (nl, nv, nhr, vhr) at least `margin`
    away from 0, and roughness and metallic at least `edge` away from their clamp edges (RMIN, 1; 0, 1)"""
    n, P = np.float64(nrm), np.float64(pos)
    par, mat = np.float64(par), np.float64(mat)
    dot = lambda a, b: (a * b).sum(0)  # noqa: E731
    nn = dot(n, n)
    ok = nn >= floor
    N = n / np.sqrt(np.maximum(nn, 1e-300))
    V = par[0:3].reshape(3, 1, 1) - P
    vv = dot(V, V)
    ok &= vv >= floor
    Vd = V / np.sqrt(np.maximum(vv, 1e-300))
    ok &= np.abs(dot(N, Vd)) >= margin
    for x, edges in ((mat[0], (RMIN, 1.0)), (mat[1], (0.0, 1.0))):
        for e in edges:
            ok &= np.abs(x - e) >= edge
    for l in range((len(par) - 6) // 6):
        Lv = par[6 + 6 * l:9 + 6 * l].reshape(3, 1, 1) - P
        r2 = dot(Lv, Lv)
        Ld = Lv / np.sqrt(np.maximum(r2, 1e-300))
        Hs = Ld + Vd
        h2 = dot(Hs, Hs)
        H = Hs / np.sqrt(np.maximum(h2, 1e-300))
        ok &= (r2 >= floor) & (h2 >= floor) & (np.abs(dot(N, Ld)) >= margin) & (np.abs(dot(N, H)) >= margin) & (np.abs(dot(Vd, H)) >= margin)
    return ok


HOSTILE_KINDS = 13
SPECIALS = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0, 1e-40, -3e-42])
MAT_EDGES = np.float32([RMIN, np.nextafter(np.float32(RMIN), np.float32(1)), np.nextafter(np.float32(RMIN), np.float32(0)), 0.0, -0.0, 1.0,
                        np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)), -0.5, 7.0, 0.03,
                        np.nan, np.nan, np.nan, np.inf, -np.inf, 1e-40, -3e-42, 1e-45])  # (a NaN three times: one draw in six)


def hostile_params(seed):
    """three lights: the eye at (0.5, 0.25, 4) and light 0 at (0.5, 0.25, -2) on one vertical line, so that a position on it at z = 0 or
    z = 2 has Ld = -Vd exactly (both distances are powers of two); lights 1 and 2 as make_params has them"""
    par = make_params(seed, 3)
    par[0:3] = (0.5, 0.25, 4.0)
    par[6:9] = (0.5, 0.25, -2.0)
    return par


def hostile_planes(rng, shape, par):
    """(nrm, pos, base, mat, gout, kind) by hand for hostile_params' block; kind [rows, W] per pixel: 0 benign (one in five facing away:
    negative cosines), 1 a zero normal (+-0), 2 a NaN, inf or subnormal normal, 3 light 0 exactly at P, 4 the eye exactly at P,
    5 Ld + Vd = 0 for light 0, 6 r2 (and vv) overflowing to inf, 7 a cosine exactly 0 (the normal in the plane perpendicular to Ld of
    light 0, P under it), 8 non-finite base and gout, 9 roughness at or beyond a clamp edge or special (MAT_EDGES), 10 metallic the same,
    11 nv <= 0 with nl > 0: P at z = 3.5 between the eye above (z = 4) and light 0 below (z = -2), the normal pointing down,
    12 N = Vd = Ld for light 0 exactly: P on the line above the eye at z = 6, the normal (0, 0, -s), s a power of two — nhr = vhr = 1,
    both inner clamps at their upper edge"""
    rows, W = shape
    nrm, pos, base, mat, gout = (np.array(t, np.float32) for t in make_planes(int(rng.integers(1 << 30)), shape))
    kind = rng.integers(0, HOSTILE_KINDS, shape)
    flip = (kind == 0) & (rng.random(shape) < 0.2)
    nrm[:, flip] = -np.abs(nrm[:, flip])
    z = kind == 1
    nrm[:, z] = rng.choice(np.float32([0.0, -0.0]), (3, int(z.sum())))
    s = kind == 2
    what = rng.integers(0, 4, shape)
    nrm[0, s & (what == 0)] = np.nan
    nrm[1, s & (what == 1)] = rng.choice(np.float32([np.inf, -np.inf, 3e38]), int((s & (what == 1)).sum()))
    sub = s & (what == 2)  # all three subnormal: nn underflows to 0
    nrm[:, sub] = (rng.integers(-2000, 2001, (3, int(sub.sum()))) * np.float64(2.0 ** -149)).astype(np.float32)
    nrm[0, s & (what == 3)] = np.float32(1e-40)  # one subnormal component among ordinary ones: lit
    pos[:, kind == 3] = par[6:9].reshape(3, 1)
    pos[:, kind == 4] = par[0:3].reshape(3, 1)
    k5 = kind == 5
    pos[0, k5], pos[1, k5] = par[0], par[1]
    pos[2, k5] = rng.choice(np.float32([0.0, 2.0]), int(k5.sum()))
    k6 = kind == 6
    pos[:, k6] = (rng.choice(np.float32([1.5e19, -2e19, 3e25]), (3, int(k6.sum()))))
    k7 = kind == 7
    pos[0, k7], pos[1, k7], pos[2, k7] = par[0], par[1], rng.choice(np.float32([1.0, -1.0, 0.5]), int(k7.sum()))
    nrm[2, k7] = 0.0
    k8 = kind == 8
    for t in (base, gout):
        hit = k8[None] & (rng.random((3,) + shape) < 0.5)
        t[hit] = SPECIALS[rng.integers(0, 5, int(hit.sum()))]
    for plane, k in ((0, 9), (1, 10)):
        hit = kind == k
        mat[plane, hit] = MAT_EDGES[rng.integers(0, len(MAT_EDGES), int(hit.sum()))]
    k11 = kind == 11
    pos[2, k11] = 3.5
    nrm[:, k11] = np.float32([[0.05], [-0.05], [-1.5]])
    k12 = kind == 12
    pos[0, k12], pos[1, k12], pos[2, k12] = par[0], par[1], 6.0
    nrm[0, k12] = nrm[1, k12] = 0.0
    nrm[2, k12] = -rng.choice(np.float32([0.5, 1.0, 2.0, 4.0]), int(k12.sum()))
    return nrm, pos, base, mat, gout, kind


def rand_ids(rng, n, h, w, tris, holes=True):
    """owner id words [n, h, w] uint32: a triangle index + 1, four in ten with the S class bit, one in ten nobody's (0)"""
    ids = rng.integers(1, tris + 1, (n, h, w)).astype(np.uint32)
    ids |= (rng.random((n, h, w)) < 0.4).astype(np.uint32) << 31
    if holes:
        ids[rng.random((n, h, w)) < 0.1] = 0
    return ids


HOSTILE = dict(seed=41, n=2, h=64, w=96, tris=20)  # the hostile test's case: its branch counts are checked on the CPU, then it runs on the GPU


def hostile_case(seed, n, h, w, tris):
    """the hostile test's inputs, the same on the CPU (where the branch counts are checked) and on the GPU: (ids [n, h, w], par,
    nrm, pos, base, mat, gout, kind — each stacked over the n frames)"""
    rng = np.random.default_rng(seed)
    ids = rand_ids(rng, n, h, w, tris)
    par = hostile_params(2)
    planes = tuple(np.stack(t) for t in zip(*(hostile_planes(rng, (h, w), par) for _ in range(n))))
    return (ids, par) + planes


def branches(tmpdir, tris, ids, nrm, pos, base, mat, gout, kind, par):
    """name -> bool mask (over [n, h, w], or [n, L, h, w] for the per-light ones) of every branch of classify, and of the hostile
    values that take no branch of their own"""
    own = ((ids & 0x7fffffff) - np.uint32(1)) < tris
    cls, mcls, lcls = (np.stack(t) for t in zip(*(classify(tmpdir, tris, ids[i], nrm[i], pos[i], mat[i], par) for i in range(len(ids)))))
    lit, view = (cls & LIT) != 0, (cls & VIEW) != 0
    reached = (lcls & REACHED) != 0
    skipped, facing, spec = (lcls & SKIPPED) != 0, (lcls & FACING) != 0, (lcls & SPEC) != 0
    out = {"nobody": ~own, "not lit": own & ~lit, "lit": lit, "no view": lit & ~view, "nv <= 0": lit & view & ((cls & NV_POS) == 0),
           "nv > 0": (cls & NV_POS) != 0}
    for name, bit in (("roughness at or below RMIN", R_LOW), ("roughness at or above 1", R_HIGH), ("metallic at or below 0", M_LOW),
                      ("metallic at or above 1", M_HIGH), ("roughness NaN", R_NAN), ("metallic NaN", M_NAN)):
        out[name] = lit & ((mcls & bit) != 0)
    out["roughness inside"] = lit & ((mcls & (R_LOW | R_HIGH)) == 0)
    out["metallic inside"] = lit & ((mcls & (M_LOW | M_HIGH)) == 0)
    out["roughness +-inf"] = lit & np.isinf(mat[:, 0])
    out["metallic +-inf"] = lit & np.isinf(mat[:, 1])
    out["material subnormal"] = lit & ((np.abs(mat) < 1e-38) & (mat != 0)).any(1)
    out.update({"skipped": reached & skipped, "back-facing": reached & ~skipped & ~facing, "facing": facing, "diffuse only": facing & ~spec,
                "specular": spec, "nh inside": spec & ((lcls & NH_IN) != 0), "nh at its edge": spec & ((lcls & NH_IN) == 0),
                "vh inside": spec & ((lcls & VH_IN) != 0), "vh at its edge": spec & ((lcls & VH_IN) == 0),
                "cosine exactly 0": own & lit & (kind == 7), "r2 overflows": own & lit & (kind == 6),
                "non-finite base": own & lit & ~np.isfinite(base).all(1), "non-finite gout": own & lit & ~np.isfinite(gout).all(1)})
    return out
