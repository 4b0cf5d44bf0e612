"""The lighting pass's test reference (tests/light_ref.c holds the arithmetic, stated once in a `real` type and built as binary32 —
the rule itself — and as binary64): per pixel (owner id word, normal, position, albedo) and a parameter frame (eye ka ks, then per
light pos intensity) → the colour planes; backward, the gradient planes and the parameter gradient accumulated in double with
sum |term| and counts; and the branch every pixel took.  Built and loaded like tests/cuberef.py's library; nothing of the product is
involved.  Also here: the same rule in torch float64 ops (autograd differentiates it), and what the CPU and GPU tests share."""
import ctypes as C

import numpy as np

from support import ref_lib

OWNED, LIT, VIEW = 1, 2, 4  # classify()'s pixel bits
SKIPPED, DIFFUSE, SPEC_ENABLED, SPEC_ON, REACHED = 1, 2, 4, 8, 16  # and its per-light bits
LIGHT_MAX = 8
vp = C.c_void_p
_head = [C.c_size_t, C.c_uint32, vp, vp, vp, vp, vp, C.c_int, C.c_uint]
SIGNATURES = {}
for _b in ("lr32_", "lr64_"):
    SIGNATURES[_b + "forward"] = (None, _head + [C.c_int, vp])
    SIGNATURES[_b + "grad"] = (None, _head + [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp])
    SIGNATURES[_b + "classify"] = (None, [C.c_size_t, C.c_uint32, vp, vp, vp, vp, C.c_int, C.c_uint, vp, vp])


def par_len(n_lights):
    return 9 + 6 * n_lights


def lib(tmpdir):
    return ref_lib("light_ref", tmpdir, SIGNATURES)


def _args(ids, nrm, pos, kd, par, dtype):
    ids = np.ascontiguousarray(ids, np.uint32)
    planes = [None if t is None else np.ascontiguousarray(t, dtype) for t in (nrm, pos, kd)]
    for t in planes:
        assert t is None or t.shape == (3,) + ids.shape, (t.shape, ids.shape)
    par = np.ascontiguousarray(par, dtype).reshape(-1)
    n_lights = (len(par) - 9) // 6
    assert 1 <= n_lights <= LIGHT_MAX and len(par) == par_len(n_lights)
    return ids, planes, par, n_lights


def _p(a):
    return a.ctypes.data if a is not None else None


def forward(tmpdir, n_tris, ids, nrm, pos, kd, par, p, fused=True, prefill=None, dtype=np.float32):
    """ids [rows, W] uint32 (plane 1 of one frame's visibility buffer), nrm / pos / kd [3, rows, W] (kd may be None), par [9 + 6 L] →
    [3, rows, W] of dtype.  prefill: [3, rows, W] uint32 words the float32 planes start from (not fused: nobody's words stay)."""
    ids, (nrm, pos, kd), par, L = _args(ids, nrm, pos, kd, par, dtype)
    if prefill is None:
        out = np.zeros((3,) + ids.shape, dtype)
    else:
        assert dtype == np.float32
        out = np.array(prefill, np.uint32, copy=True, order="C").view(np.float32)
    fn = lib(tmpdir).lr32_forward if dtype == np.float32 else lib(tmpdir).lr64_forward
    fn(ids.size, n_tris, _p(ids), _p(nrm), _p(pos), _p(kd), _p(par), L, p, int(fused), _p(out))
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


def grad(tmpdir, n_tris, ids, nrm, pos, kd, par, p, gout, into=None, fused=True, prefill=None, want_terms=False, dtype=np.float32):
    """one frame's share: adds into `into` (a Grad, or None) and returns (gnrm, gpos, gkd) [3, rows, W] each (gkd None without kd),
    and with want_terms the per-pixel terms [K, rows, W]"""
    ids, (nrm, pos, kd), par, L = _args(ids, nrm, pos, kd, par, dtype)
    gout = np.ascontiguousarray(gout, dtype)
    assert gout.shape == nrm.shape

    def fresh():
        if prefill is None:
            return np.zeros(nrm.shape, dtype)
        assert dtype == np.float32
        return np.array(prefill, np.uint32, copy=True, order="C").view(np.float32)
    gnrm, gpos, gkd = fresh(), fresh(), (fresh() if kd is not None else None)
    terms = np.zeros((par_len(L),) + ids.shape, dtype) if want_terms else None
    fn = lib(tmpdir).lr32_grad if dtype == np.float32 else lib(tmpdir).lr64_grad
    fn(ids.size, n_tris, _p(ids), _p(nrm), _p(pos), _p(kd), _p(par), L, p, _p(gout), int(fused), _p(gnrm), _p(gpos), _p(gkd),
       _p(into.gsum) if into else None, _p(into.gabs) if into else None, _p(into.count) if into else None, _p(terms))
    return (gnrm, gpos, gkd, terms) if want_terms else (gnrm, gpos, gkd)


def classify(tmpdir, n_tris, ids, nrm, pos, par, p):
    """([rows, W] uint8: OWNED | LIT | VIEW, [L, rows, W] uint8: REACHED | SKIPPED | DIFFUSE | SPEC_ENABLED | SPEC_ON) by the binary32 rule"""
    ids, (nrm, pos, _), par, L = _args(ids, nrm, pos, None, par, np.float32)
    cls, lcls = np.zeros(ids.shape, np.uint8), np.zeros((L,) + ids.shape, np.uint8)
    lib(tmpdir).lr32_classify(ids.size, n_tris, _p(ids), _p(nrm), _p(pos), _p(par), L, p, _p(cls), _p(lcls))
    return cls, lcls


# ------------------------------------------------------------------------------------------------ the rule in torch float64 ops
def torch_rule(nrm, pos, kd, lights, eye, ka, ks, p):
    """the rule of include/srz.h on planes [..., 3, rows, W] with torch ops in the tensors' dtype (no fmaf, torch's own order of
    operations), every pixel taken as owned; lights [L, 6], eye / ka / ks [3].  Differentiable by autograd: the branches are held by
    torch.where on detached conditions, exactly the derivative the backward states."""
    import torch
    v3 = lambda t: t.reshape(3, 1, 1)  # noqa: E731
    dot = lambda a, b: (a * b).sum(-3, keepdim=True)  # noqa: E731
    ok = lambda x: (x > 0) & (x < float("inf"))  # noqa: E731
    zero = torch.zeros((), dtype=nrm.dtype, device=nrm.device)
    safe = lambda x, m: torch.where(m, x, torch.ones_like(x))  # noqa: E731
    nn = dot(nrm, nrm)
    lit = ok(nn.detach())
    N = nrm / safe(nn, lit).sqrt()
    V = v3(eye) - pos
    vv = dot(V, V)
    view = ok(vv.detach())
    Vd = torch.where(view, V / safe(vv, view).sqrt(), zero)
    kd = torch.ones_like(nrm) if kd is None else kd
    acc = torch.zeros_like(nrm)
    for l in range(lights.shape[0]):
        lpos, I = v3(lights[l, :3]), v3(lights[l, 3:])
        Lv = lpos - pos
        r2 = dot(Lv, Lv)
        on = ok(r2.detach())
        r2s = safe(r2, on)
        Ld = Lv / r2s.sqrt()
        cd = dot(N, Ld).clamp(min=0)
        Hs = Ld + Vd
        h2 = dot(Hs, Hs)
        spec = view & (h2.detach() > 0)
        H = Hs / safe(h2, spec).sqrt()
        cs = dot(N, H).clamp(min=0)
        sp = torch.where(spec, cs ** p, zero)
        E = I / r2s
        acc = acc + torch.where(on, kd * (E * cd + v3(ka) * I) + (v3(ks) * E) * sp, zero)
    return torch.where(lit, acc, zero)


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
def make_params(seed, n_lights, frames=None):
    """a parameter block [9 + 6 L] (or [frames, ...]) float32: the eye and the lights in front of the scene (z in 3 .. 6, x / y within
    +-2), ka, ks and the intensities positive, deterministic"""
    rng = np.random.default_rng([seed, n_lights])
    n = 1 if frames is None else frames
    par = np.zeros((n, par_len(n_lights)), np.float32)
    par[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    par[:, 2] = rng.uniform(3, 6, n)
    par[:, 3:6] = rng.uniform(0.02, 0.2, (n, 3))
    par[:, 6:9] = rng.uniform(0.2, 1.0, (n, 3))
    L = par[:, 9:].reshape(n, n_lights, 6)
    L[:, :, 0:2] = rng.uniform(-2, 2, (n, n_lights, 2))
    L[:, :, 2] = rng.uniform(3, 6, (n, n_lights))
    L[:, :, 3:6] = rng.uniform(2, 20, (n, n_lights, 3))
    return par[0] if frames is None else par


def make_planes(seed, shape):
    """(nrm, pos, kd, gout) [3, rows, W] float32 each: normals of any length, tilted, facing +z (one in twenty: away), positions on a
    rough sheet around z = 0 within +-1 in x / y, albedo in (0.1, 1), gout normal"""
    rng = np.random.default_rng([seed, *shape])
    rows, W = shape
    nrm = rng.normal(0, 0.25, (3, rows, W))
    nrm[2] = np.abs(nrm[2]) + 0.6
    nrm *= rng.uniform(0.5, 3.0, (1, rows, W)) * np.where(rng.random((1, rows, W)) < 0.05, -1.0, 1.0)  # (one in twenty faces away)
    pos = rng.uniform(-1.0, 1.0, (3, rows, W))
    pos[2] *= 0.3
    kd = rng.uniform(0.1, 1.0, (3, rows, W))
    gout = rng.normal(0, 1, (3, rows, W))
    return tuple(np.ascontiguousarray(t, np.float32) for t in (nrm, pos, kd, gout))


def well_conditioned(nrm, pos, par, margin=0.05, floor=0.25):
    """[rows, W] bool by the rule in float64: nn, vv, every r2 and h2 >= floor, and every raw cosine at least `margin` away from 0"""
    n, P = np.float64(nrm), np.float64(pos)
    par = np.float64(par)
    dot = lambda a, b: (a * b).sum(0)  # noqa: E731
    nn = dot(n, n)
    ok = nn >= floor
    N = n / np.sqrt(np.maximum(nn, 1e-300))
    V = par[0:3].reshape(3, 1, 1) - P
    vv = dot(V, V)
    ok &= vv >= floor
    Vd = V / np.sqrt(np.maximum(vv, 1e-300))
    for l in range((len(par) - 9) // 6):
        Lv = par[9 + 6 * l:12 + 6 * l].reshape(3, 1, 1) - P
        r2 = dot(Lv, Lv)
        Ld = Lv / np.sqrt(np.maximum(r2, 1e-300))
        Hs = Ld + Vd
        h2 = dot(Hs, Hs)
        H = Hs / np.sqrt(np.maximum(h2, 1e-300))
        ok &= (r2 >= floor) & (h2 >= floor) & (np.abs(dot(N, Ld)) >= margin) & (np.abs(dot(N, H)) >= margin)
    return ok


HOSTILE_KINDS = 9
SPECIALS = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0, 1e-40, -3e-42])


def hostile_params(seed):
    """three lights: the eye at (0.5, 0.25, 4) and light 0 at (0.5, 0.25, -2) on one vertical line, so that a position on it at z = 0 or
    z = 2 has Ld = -Vd exactly (both distances are powers of two); lights 1 and 2 as make_params has them"""
    par = make_params(seed, 3)
    par[0:3] = (0.5, 0.25, 4.0)
    par[9:12] = (0.5, 0.25, -2.0)
    return par


def hostile_planes(rng, shape, par):
    """(nrm, pos, kd, gout, kind) by hand for hostile_params' block; kind [rows, W] per pixel: 0 benign (one in five facing away:
    negative cosines), 1 a zero normal (+-0), 2 a NaN, inf or subnormal normal, 3 light 0 exactly at P, 4 the eye exactly at P,
    5 Ld + Vd = 0 for light 0, 6 r2 (and vv) overflowing to inf, 7 a cosine exactly 0 (the normal in the plane perpendicular to Ld of
    light 0, P under it), 8 non-finite kd and gout"""
    rows, W = shape
    nrm, pos, kd, gout = (np.array(t, np.float32) for t in make_planes(int(rng.integers(1 << 30)), shape))
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
    pos[:, kind == 3] = par[9:12].reshape(3, 1)
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
    for t in (kd, gout):
        hit = k8[None] & (rng.random((3,) + shape) < 0.5)
        t[hit] = SPECIALS[rng.integers(0, 5, int(hit.sum()))]
    return nrm, pos, kd, gout, kind
