"""The mipmapped cube lookup's test reference (tests/cubemip_ref.c holds the arithmetic): a cube's mip pyramid — a list of levels
[6, N_l, N_l, C] — and per pixel (owner id word, direction, level of detail) → the sampled planes; backward, the gradient planes with
respect to the direction and to the level and the pyramid's gradient accumulated in double; and the level from the footprint.  Built
twice: binary32 (dtype np.float32, the arithmetic the library is held to) and binary64 (np.float64, the same text in double).
Nothing of the product is involved."""
import ctypes as C
import os

import numpy as np

from support import build_c, ref_lib

OWNED, SAMPLED, CLAMP_LOW, CLAMP_HIGH, FRACTIONAL, CROSSED_ABOVE0 = 1, 2, 4, 8, 16, 32  # classify()'s bits
vp = C.c_void_p
_head = [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_size_t, vp, vp, vp, vp, vp]
SIGNATURES = {"cmr_real_bytes": (C.c_int, []),
              "cmr_classify": (None, [C.c_int, C.c_int, C.c_uint32, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
              "cmr_forward": (None, _head + [C.c_int, vp]),
              "cmr_grad": (None, _head + [vp, C.c_int, vp, vp, vp, vp, vp]),
              "cmr_level": (None, [C.c_int, C.c_int, C.c_uint32, C.c_size_t, vp, vp, vp, vp, vp, C.c_int, vp, vp])}
_lib64 = {}


def lib(tmpdir, dtype=np.float32):
    """the binary32 build (support.ref_lib's cache) or, dtype np.float64, the same file built with -DCMR_DOUBLE"""
    if np.dtype(dtype) == np.float32:
        L = ref_lib("cubemip_ref", tmpdir, SIGNATURES)
        assert L.cmr_real_bytes() == 4
        return L
    assert np.dtype(dtype) == np.float64
    if "L" not in _lib64:
        L = C.CDLL(build_c("cubemip_ref", os.path.join(str(tmpdir), "libcubemip_ref64.so"), "-O2", "-shared", "-fPIC", "-DCMR_DOUBLE"))
        for fn, (restype, argtypes) in SIGNATURES.items():
            getattr(L, fn).restype, getattr(L, fn).argtypes = restype, argtypes
        assert L.cmr_real_bytes() == 8
        _lib64["L"] = L
    return _lib64["L"]


def n_levels(n):
    """include/srz.h: level l + 1 exists iff n_l > 1 and n_l is even"""
    L = 1
    while n > 1 and n % 2 == 0:
        n, L = n // 2, L + 1
    return L


def build(cube, L=None):
    """cube [6, N, N, C] (or [frames, 6, N, N, C]) → the list of its levels 0 .. L - 1, every face box-filtered on its own:
    ((t00 + t01) + (t10 + t11)) * 0.25 in the cube's dtype (numpy's elementwise operations are the IEEE ones)"""
    cube = np.ascontiguousarray(cube)
    L = n_levels(cube.shape[-2]) if L is None else L
    levels = [cube]
    for _ in range(1, L):
        t = levels[-1]
        q = cube.dtype.type(0.25)
        levels.append(np.ascontiguousarray(((t[..., 0::2, 0::2, :] + t[..., 0::2, 1::2, :]) + (t[..., 1::2, 0::2, :] + t[..., 1::2, 1::2, :])) * q))
    return levels


def flat(levels, first=0):
    """the levels first .. of a pyramid as one flat array, level-major (first = 1: srz_cube_mip_build's layout)"""
    return np.concatenate([np.ascontiguousarray(l).ravel() for l in levels[first:]]) if len(levels) > first else np.zeros(0, levels[0].dtype)


def _args(levels, ids, dirs, lam, dtype):
    levels = [np.ascontiguousarray(l, dtype) for l in levels]
    N, n_ch, L = levels[0].shape[1], levels[0].shape[3], len(levels)
    assert all(l.shape == (6, N >> i, N >> i, n_ch) for i, l in enumerate(levels)) and 1 <= L <= n_levels(N)
    ids = np.ascontiguousarray(ids, np.uint32)
    dirs = np.ascontiguousarray(dirs, dtype)
    assert ids.ndim == 2 and dirs.shape == (3,) + ids.shape
    d = [np.ascontiguousarray(dirs[k]) for k in range(3)]
    if lam is not None:
        lam = np.ascontiguousarray(lam, dtype).reshape(ids.shape)
    assert lam is not None or L == 1
    return flat(levels), N, L, n_ch, ids, d, lam, ids.shape


def _p(a):
    return a.ctypes.data if a is not None else None


def classify(tmpdir, N, L, n_tris, ids, dirs, lam, dtype=np.float32):
    """→ (cls [rows, W] uint8 of OWNED | SAMPLED | CLAMP_LOW | CLAMP_HIGH | FRACTIONAL | CROSSED_ABOVE0, face [rows, W] uint8 (255: not
    sampled), l0 [rows, W] int32, f [rows, W])"""
    ids = np.ascontiguousarray(ids, np.uint32)
    dirs = np.ascontiguousarray(dirs, dtype)
    d = [np.ascontiguousarray(dirs[k]) for k in range(3)]
    lam = None if lam is None else np.ascontiguousarray(lam, dtype).reshape(ids.shape)
    rows, W = ids.shape
    cls, face, l0, f = np.zeros((rows, W), np.uint8), np.zeros((rows, W), np.uint8), np.zeros((rows, W), np.int32), np.zeros((rows, W), dtype)
    lib(tmpdir, dtype).cmr_classify(N, L, n_tris, rows * W, ids.ctypes.data, d[0].ctypes.data, d[1].ctypes.data, d[2].ctypes.data, _p(lam),
                                    cls.ctypes.data, face.ctypes.data, l0.ctypes.data, f.ctypes.data)
    return cls, face, l0, f


def forward(tmpdir, levels, n_tris, ids, dirs, lam, fused=True, prefill=None, dtype=np.float32):
    """levels: the pyramid's levels 0 .. L - 1, [6, N_l, N_l, C] each; ids [rows, W] uint32; dirs [3, rows, W]; lam [rows, W] (None at
    L == 1) → [C, rows, W].  prefill (binary32 only): [C, rows, W] uint32 words the planes start from"""
    pyr, N, L, n_ch, ids, d, lam, (rows, W) = _args(levels, ids, dirs, lam, dtype)
    if prefill is None:
        out = np.zeros((n_ch, rows, W), dtype)
    else:
        out = np.array(prefill, np.uint32, copy=True, order="C").view(np.float32)
    assert out.shape == (n_ch, rows, W)
    lib(tmpdir, dtype).cmr_forward(pyr.ctypes.data, N, L, n_ch, n_tris, rows * W, ids.ctypes.data, d[0].ctypes.data, d[1].ctypes.data,
                                   d[2].ctypes.data, _p(lam), int(fused), out.ctypes.data)
    return out


def sample(tmpdir, levels, dirs, lam, dtype=np.float32):
    """dirs [n, 3], lam [n] → [n, C]: every direction a pixel with an owner"""
    d = np.ascontiguousarray(dirs, dtype).reshape(-1, 3)
    lam = None if lam is None else np.ascontiguousarray(lam, dtype).reshape(1, -1)
    return forward(tmpdir, levels, 1, np.ones((1, len(d)), np.uint32), d.T.reshape(3, 1, -1), lam, dtype=dtype)[:, 0].T


class Grad:
    """the pyramid's gradient of any number of frames, accumulated in double: .g the levels 0 .. L - 1 flat (level 0 first), .gabs the
    sums of |product|, .count the contributing adds per texel"""

    def __init__(self, N, n_ch, L):
        self.N, self.n_ch, self.L = N, n_ch, L
        self.texels = [6 * (N >> l) ** 2 for l in range(L)]
        self.g, self.gabs = np.zeros(sum(self.texels) * n_ch, np.float64), np.zeros(sum(self.texels) * n_ch, np.float64)
        self.count = np.zeros(sum(self.texels), np.uint32)

    def level(self, a, l):
        """level l of .g / .gabs / .count as [6, N_l, N_l, C] ([6, N_l, N_l] for count)"""
        per = 1 if a is self.count else self.n_ch
        off, nl = sum(self.texels[:l]) * per, self.N >> l
        return a[off:off + self.texels[l] * per].reshape((6, nl, nl) if a is self.count else (6, nl, nl, self.n_ch))

    def bound(self, extra=0):
        """per element: gamma_n * sum |product|, gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing adds (+ extra: the
        adds of a value the buffer held before; one rounding per add; the products are the float32 products themselves)"""
        n = (np.repeat(self.count.astype(np.float64), self.n_ch) + extra) * 2.0 ** -24
        return n / (1.0 - n) * self.gabs


def grad(tmpdir, levels, n_tris, ids, dirs, lam, gout, into=None, want_dir=True, want_lam=True, fused=True, prefill=None, dtype=np.float32):
    """one frame's share: adds into `into` (a Grad, or None) and returns (gdir [3, rows, W], glam [rows, W]), None where not wanted.
    prefill (binary32 only): the uint32 word the planes start from"""
    pyr, N, L, n_ch, ids, d, lam, (rows, W) = _args(levels, ids, dirs, lam, dtype)
    gout = np.ascontiguousarray(gout, dtype)
    assert gout.shape == (n_ch, rows, W)

    def plane(shape):
        return np.zeros(shape, dtype) if prefill is None else np.full(shape, prefill, np.uint32).view(np.float32)
    gdir = plane((3, rows, W)) if want_dir else None
    glam = plane((rows, W)) if want_lam else None
    if into is not None:
        assert (into.N, into.n_ch, into.L) == (N, n_ch, L)
    lib(tmpdir, dtype).cmr_grad(pyr.ctypes.data, N, L, n_ch, n_tris, rows * W, ids.ctypes.data, d[0].ctypes.data, d[1].ctypes.data,
                                d[2].ctypes.data, _p(lam), gout.ctypes.data, int(fused), _p(into.g) if into else None,
                                _p(into.gabs) if into else None, _p(into.count) if into else None, _p(gdir), _p(glam))
    return gdir, glam


def level(tmpdir, N, L, n_tris, ids, dirs, dird, fused=True, prefill=None, dtype=np.float32, parts=False):
    """dirs [3, rows, W], dird [6, rows, W] → lam [rows, W]; parts: also (l0, f) in front of the sum, [rows, W, 2]"""
    ids = np.ascontiguousarray(ids, np.uint32)
    dirs, dird = np.ascontiguousarray(dirs, dtype), np.ascontiguousarray(dird, dtype)
    rows, W = ids.shape
    assert dirs.shape == (3, rows, W) and dird.shape == (6, rows, W)
    d = [np.ascontiguousarray(dirs[k]) for k in range(3)]
    out = np.zeros((rows, W), dtype) if prefill is None else np.full((rows, W), prefill, np.uint32).view(np.float32)
    l0f = np.zeros((rows, W, 2), dtype) if parts else None
    lib(tmpdir, dtype).cmr_level(N, L, n_tris, rows * W, ids.ctypes.data, d[0].ctypes.data, d[1].ctypes.data, d[2].ctypes.data, dird.ctypes.data,
                                 int(fused), out.ctypes.data, _p(l0f))
    return (out, l0f) if parts else out


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
HOSTILE_LAM = np.float32([np.nan, -np.inf, np.inf, -1.0, -0.0, 0.0, 1e-45, 0.5, 1.0, 1.5, 2.0, 2.9999998, 3.0, 14.0, 15.0, 3e38, -3e-39])


def hostile_lam(rng, shape, L):
    """a level plane that hits every clamp, the integers, fractions and HOSTILE_LAM"""
    lam = rng.uniform(-0.5, L - 0.5, shape).astype(np.float32)
    kind = rng.integers(0, 6, shape)
    lam = np.where(kind == 1, np.floor(lam), lam).astype(np.float32)  # integers (negative ones too)
    lam = np.where(kind == 2, HOSTILE_LAM[rng.integers(0, len(HOSTILE_LAM), shape)], lam).astype(np.float32)
    lam = np.where(kind == 3, np.float32(L - 1) * rng.choice(np.float32([1.0, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23]), shape), lam)
    return np.ascontiguousarray(lam, np.float32)
