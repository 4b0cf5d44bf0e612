"""The shadow-map lookup's test reference (tests/shadow_ref.c holds the arithmetic, stated once in a `real` type and built as binary32
— the rule itself — and as binary64): a float depth map [H, W] and per pixel (owner id word, sx, sy, sd) → the lit fraction; backward,
the gradient planes gsx, gsy, gsd and the map's gradient accumulated in double with sum |term| and counts.  Built and loaded like
tests/cuberef.py's library; nothing of the product is involved.  Also here: the same rule in torch float64 ops (autograd
differentiates it), and what the CPU and GPU tests share."""
import ctypes as C

import numpy as np

from support import ref_lib

OWNED, SAMPLED, MOVING, OUTSIDE = 1, 2, 4, 8  # classify()'s bits: owned, sampled, a corner on the ramp, a corner outside the map
vp = C.c_void_p
SIGNATURES = {}
for _b, _r in (("sr32_", C.c_float), ("sr64_", C.c_double)):
    _head = [vp, C.c_int, C.c_int, C.c_uint32, C.c_size_t, vp, vp, vp, vp]
    SIGNATURES[_b + "forward"] = (None, _head + [_r, _r, C.c_int, vp])
    SIGNATURES[_b + "grad"] = (None, _head + [vp, _r, _r, C.c_int, vp, vp, vp, vp])
    SIGNATURES[_b + "classify"] = (None, _head + [_r, _r, vp])
    SIGNATURES[_b + "taps"] = (None, [vp, C.c_int, C.c_int, C.c_size_t, vp, vp, vp, _r, _r, vp, vp, vp])


def lib(tmpdir):
    return ref_lib("shadow_ref", tmpdir, SIGNATURES)


def _fn(tmpdir, name, dtype):
    return getattr(lib(tmpdir), ("sr32_" if dtype == np.float32 else "sr64_") + name)


def _args(map, ids, sc, dtype):
    """map [H, W], ids [rows, W'] uint32, sc [3, rows, W'] → contiguous arrays of dtype"""
    map = np.ascontiguousarray(map, dtype)
    ids = np.ascontiguousarray(ids, np.uint32)
    sc = np.ascontiguousarray(sc, dtype)
    assert map.ndim == 2 and ids.ndim == 2 and sc.shape == (3,) + ids.shape, (map.shape, ids.shape, sc.shape)
    return map, ids, [np.ascontiguousarray(sc[k]) for k in range(3)]


def _p(a):
    return a.ctypes.data if a is not None else None


def forward(tmpdir, map, n_tris, ids, sc, bias, width, fused=True, prefill=None, dtype=np.float32):
    """map [H, W]; ids [rows, W'] uint32, plane 1 of one frame's visibility buffer; sc [3, rows, W'] → [1, rows, W'] of dtype.
    prefill: [1, rows, W'] uint32 words the float32 plane starts from (not fused: nobody's words stay)."""
    map, ids, s = _args(map, ids, sc, dtype)
    if prefill is None:
        out = np.zeros((1,) + ids.shape, dtype)
    else:
        assert dtype == np.float32
        out = np.array(prefill, np.uint32, copy=True, order="C").view(np.float32)
        assert out.shape == (1,) + ids.shape
    _fn(tmpdir, "forward", dtype)(_p(map), map.shape[1], map.shape[0], n_tris, ids.size, _p(ids), _p(s[0]), _p(s[1]), _p(s[2]), bias, width,
                                  int(fused), _p(out))
    return out


class Grad:
    """the map's gradient of any number of frames, accumulated in double: .gmap [H, W] float64, .gabs the sums of |term|, .count
    [H, W] the contributing adds per texel"""

    def __init__(self, map_shape):
        self.gmap, self.gabs = np.zeros(map_shape, np.float64), np.zeros(map_shape, np.float64)
        self.count = np.zeros(map_shape, np.uint32)

    def bound(self, extra=0):
        """per texel: gamma_n * sum |term|, gamma_n = n u / (1 - n u), u = 2^-24, n the texel's contributing adds (+ extra: the adds of
        a value the buffer held before, or of another rank's partial sum; one rounding per add; the terms are the float32 terms
        themselves)"""
        n = (self.count.astype(np.float64) + extra) * 2.0 ** -24
        return n / (1.0 - n) * self.gabs


def grad(tmpdir, map, n_tris, ids, sc, gout, bias, width, into=None, want_sc=True, fused=True, prefill=None, dtype=np.float32):
    """one frame's share: adds into `into` (a Grad, or None) and returns the gsc planes [3, rows, W'] of dtype (None if not wanted)"""
    map, ids, s = _args(map, ids, sc, dtype)
    gout = np.ascontiguousarray(gout, dtype).reshape(ids.shape)
    gsc = None
    if want_sc:
        if prefill is None:
            gsc = np.zeros((3,) + ids.shape, dtype)
        else:
            assert dtype == np.float32
            gsc = np.array(prefill, np.uint32, copy=True, order="C").view(np.float32)
            assert gsc.shape == (3,) + ids.shape
    if into is not None:
        assert into.gmap.shape == map.shape
    _fn(tmpdir, "grad", dtype)(_p(map), map.shape[1], map.shape[0], n_tris, ids.size, _p(ids), _p(s[0]), _p(s[1]), _p(s[2]), _p(gout), bias, width,
                               int(fused), _p(into.gmap) if into else None, _p(into.gabs) if into else None,
                               _p(into.count) if into else None, _p(gsc))
    return gsc


def classify(tmpdir, map, n_tris, ids, sc, bias, width, dtype=np.float32):
    """[rows, W'] uint8: OWNED | SAMPLED | MOVING | OUTSIDE"""
    map, ids, s = _args(map, ids, sc, dtype)
    cls = np.zeros(ids.shape, np.uint8)
    _fn(tmpdir, "classify", dtype)(_p(map), map.shape[1], map.shape[0], n_tris, ids.size, _p(ids), _p(s[0]), _p(s[1]), _p(s[2]), bias, width,
                                   _p(cls))
    return cls


def taps(tmpdir, map, sc, bias, width, dtype=np.float32):
    """sc [3, ...] → dict of xy0 [..., 2] int32 (INT32_MIN: unsampled), frac [..., 2] (tx, ty), q [..., 4] (the corners' ramp values;
    NaN: the corner is outside the map, or width == 0)"""
    sc = np.ascontiguousarray(sc, dtype)
    shape = sc.shape[1:]
    map = np.ascontiguousarray(map, dtype)
    s = [np.ascontiguousarray(sc[k]) for k in range(3)]
    r = dict(xy0=np.zeros(shape + (2,), np.int32), frac=np.zeros(shape + (2,), dtype), q=np.zeros(shape + (4,), dtype))
    _fn(tmpdir, "taps", dtype)(_p(map), map.shape[1], map.shape[0], s[0].size, _p(s[0]), _p(s[1]), _p(s[2]), bias, width, _p(r["xy0"]),
                               _p(r["frac"]), _p(r["q"]))
    return r


def one(tmpdir, map, sx, sy, sd, bias=0.0, width=0.0, g=1.0, dtype=np.float32):
    """one owned pixel → (out, (gsx, gsy, gsd), Grad)"""
    map = np.asarray(map, dtype)
    sc = np.array([sx, sy, sd], dtype).reshape(3, 1, 1)
    ids = np.ones((1, 1), np.uint32)
    out = forward(tmpdir, map, 1, ids, sc, bias, width, dtype=dtype)
    acc = Grad(map.shape)
    gsc = grad(tmpdir, map, 1, ids, sc, np.array([[g]], dtype), bias, width, into=acc, dtype=dtype)
    return out.reshape(()), tuple(gsc.reshape(3)), acc


# ------------------------------------------------------------------------------------------------ the rule in torch float64 ops
def torch_rule(map, sx, sy, sd, bias, width):
    """map [H, W] (or [n, H, W] with sx / sy / sd [n, ...]: frame i looks up map i), sx / sy / sd float tensors of one dtype (float64
    in the tests) → the lit fraction; every operation a torch op, so autograd gives the gradients with respect to map, sx, sy and sd
    (floor and the comparisons have none, the clamps stop theirs: the rule's in_x, in_y and `moving`)"""
    import torch
    H, W = map.shape[-2:]
    frame = torch.arange(map.shape[0], device=map.device).reshape((-1,) + (1,) * (sx.dim() - 1)) if map.dim() == 3 else None

    def axis(s, n):
        fx = s.clamp(-1.0, float(n))
        f0 = fx.detach().floor()
        return f0.long(), fx - f0

    x0, tx = axis(sx, W)
    y0, ty = axis(sy, H)
    v = []
    for r in (0, 1):
        for c in (0, 1):
            x, y = x0 + c, y0 + r
            inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            yc, xc = y.clamp(0, H - 1), x.clamp(0, W - 1)
            e = ((map[yc, xc] if frame is None else map[frame, yc, xc]) + bias) - sd
            val = (e / width + 0.5).clamp(0.0, 1.0) if width > 0 else (e >= 0).to(e.dtype)
            v.append(torch.where(inside, val, torch.ones_like(val)))
    top, bot = v[0] + tx * (v[1] - v[0]), v[2] + tx * (v[3] - v[2])
    return top + ty * (bot - top)


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
MAP_SIZES = ((1, 1), (2, 2), (5, 3), (64, 64), (160, 160))  # (map_w, map_h)
Z_LO, Z_HI = 40.0, 80.0  # the depths the generators draw maps and sd from: e = m - sd is spread over +-40
BIASES = (0.0, 0.375, -1.25)


def make_map(seed, w, h, frames=None):
    """a map [h, w] (or [frames, h, w]) of depths in [Z_LO, Z_HI), deterministic"""
    shape = (h, w) if frames is None else (frames, h, w)
    return np.random.default_rng([seed, w, h]).uniform(Z_LO, Z_HI, shape).astype(np.float32)


def make_coords(seed, shape, w, h):
    """coordinate planes [3, rows, W'] float32 for a w x h map: x0 uniform over [-1, w - 1] (so the corners outside the map on every
    side occur), the fraction uniform over [0.025, 0.975] (the generator does not aim at the lattice: the KATs and the hostile planes
    do), sd uniform over [Z_LO, Z_HI)"""
    rng = np.random.default_rng([seed, 77])
    sx = rng.integers(-1, w, shape) + rng.uniform(0.025, 0.975, shape)
    sy = rng.integers(-1, h, shape) + rng.uniform(0.025, 0.975, shape)
    return np.stack([sx, sy, rng.uniform(Z_LO, Z_HI, shape)]).astype(np.float32)


def well_conditioned(tmpdir, map, sc, bias, width, margin=0.02):
    """[rows, W'] bool: finite inputs, tx and ty at least `margin` from 0 and 1, and every inside corner's ramp value q at least
    `margin` away from 0 and from 1 — on the ramp, or clamped by at least that much — judged in the binary64 build"""
    t = taps(tmpdir, map, sc, bias, width, dtype=np.float64)
    ok = np.isfinite(sc).all(0) & (t["xy0"][..., 0] != np.iinfo(np.int32).min)
    ok &= ((t["frac"] >= margin) & (t["frac"] <= 1 - margin)).all(-1)
    q = t["q"]
    ok &= (np.isnan(q) | ((np.abs(q) >= margin) & (np.abs(q - 1) >= margin))).all(-1)
    return ok


# the coordinate and texel values of the hand KATs (tests/test_shadow_ref.py), which the GPU tests place in every lane of a quad
def kat_coords(w):
    return np.float32([-1.0, -0.5, w - 1.0, w - 0.5, w, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.0, -0.0, 0.5, 1.0])


KAT_TEXELS = np.float32([np.inf, -np.inf, np.nan])
TINY_WIDTH = 2.0 ** -120  # e / width overflows for every |e| >= 2^8: q = +-inf, v = 0 or 1, not moving


def hostile_coords(rng, shape, w, h):
    """coordinate planes [3, rows, W'] float32 by hand: make_coords' spread, and shares of exact texel hits (tx = 0), both borders from
    both sides, the KAT values in sx, sy and sd (NaN / inf / 1e30: unsampled or clamped), and sd equal to a map depth's neighbourhood"""
    rows, W = shape
    sc = make_coords(int(rng.integers(1 << 30)), shape, w, h)
    kind = rng.integers(0, 10, shape)
    on = kind == 1  # exactly on a texel, in one axis or both
    sc[0][on] = rng.integers(-1, w + 1, int(on.sum()))
    both = on & (rng.random(shape) < 0.5)
    sc[1][both] = rng.integers(-1, h + 1, int(both.sum()))
    edge = kind == 2  # within a texel of the borders, from both sides
    sc[0][edge] = rng.choice(np.float32([-1.5, -1.0, -0.75, -0.25, w - 1.25, w - 0.5, w, w + 0.5]), int(edge.sum()))
    e2 = edge & (rng.random(shape) < 0.5)
    sc[1][e2] = rng.choice(np.float32([-1.5, -1.0, -0.75, -0.25, h - 1.25, h - 0.5, h, h + 0.5]), int(e2.sum()))
    k = kind == 3  # the KAT values, in any of the three planes
    hit = rng.random((3,) + shape) < 0.4
    vals = np.stack([kat_coords(w)[rng.integers(0, 14, shape)], kat_coords(h)[rng.integers(0, 14, shape)],
                     rng.choice(np.float32([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, 60.0]), shape)])
    for p in range(3):
        sel = k & hit[p]
        sc[p][sel] = vals[p][sel]
    return np.ascontiguousarray(sc)


def hostile_map(rng, w, h, frames=None):
    """make_map's depths with a share of +inf (nobody in the light's view: lit), -inf and NaN texels"""
    m = make_map(int(rng.integers(1 << 30)), w, h, frames)
    sel = rng.random(m.shape) < 0.08
    m[sel] = rng.choice(np.float32([np.inf, np.inf, -np.inf, np.nan]), int(sel.sum()))
    return m
