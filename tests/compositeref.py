"""The depth-layer composite's test reference (tests/composite_ref.c holds the arithmetic): layers of id words, colours and alphas
composited front to back, and the backward.  Built twice: binary32 (dtype np.float32, the arithmetic the library is held to) and
binary64 (np.float64, the same text in double).  Nothing of the product is involved.

Shapes, as the library's: ids[k] [n, rows, W] uint32 (plane 1 of a visibility buffer), colors[k] [n, C, rows, W], alphas[k]
[n, 1, rows, W] or a Python float, bg [n, C, rows, W] or None, n_tris one count per frame."""
import ctypes as C
import os

import numpy as np

from support import build_c, ref_lib

MAX_LAYERS = 8
vp = C.c_void_p
SIGNATURES = {"cmr_real_bytes": (C.c_int, []),
              "cmr_cover": (None, [vp, C.c_size_t, C.c_uint32, vp]),
              "cmr_forward": (None, [C.c_int, C.c_int, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]),
              "cmr_grad": (None, [C.c_int, C.c_int, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp])}
_lib64 = {}


def lib(tmpdir, dtype=np.float32):
    """the binary32 build (support.ref_lib's cache) or, dtype np.float64, the same file built with -DCMR_DOUBLE"""
    if np.dtype(dtype) == np.float32:
        L = ref_lib("composite_ref", tmpdir, SIGNATURES)
        assert L.cmr_real_bytes() == 4
        return L
    assert np.dtype(dtype) == np.float64
    if "L" not in _lib64:
        L = C.CDLL(build_c("composite_ref", os.path.join(str(tmpdir), "libcomposite_ref64.so"), "-O2", "-shared", "-fPIC", "-DCMR_DOUBLE"))
        for fn, (restype, argtypes) in SIGNATURES.items():
            getattr(L, fn).restype, getattr(L, fn).argtypes = restype, argtypes
        assert L.cmr_real_bytes() == 8
        _lib64["L"] = L
    return _lib64["L"]


def cover(tmpdir, ids, n_tris):
    """ids [n, rows, W] uint32, n_tris per frame → bool [n, rows, W]: the id names an owner"""
    ids = np.ascontiguousarray(ids, np.uint32)
    cov = np.zeros(ids.shape, np.uint8)
    for f in range(ids.shape[0]):
        lib(tmpdir).cmr_cover(ids[f].ctypes.data, ids[f].size, int(n_tris[f]), cov[f].ctypes.data)
    return cov.astype(bool)


def _ptrs(arrays):
    return (vp * max(1, len(arrays)))(*[None if a is None else a.ctypes.data for a in arrays])


class _Call:
    """one frame's arguments as contiguous arrays and the pointer tables over them"""

    def __init__(self, f, covs, colors, alphas, bg, dtype):
        self.cov = [np.ascontiguousarray(c[f], np.uint8) for c in covs]
        self.col = [np.ascontiguousarray(c[f], dtype) for c in colors]
        self.alpha = [None if np.isscalar(a) else np.ascontiguousarray(a[f, 0], dtype) for a in alphas]
        self.opacity = np.array([dtype(a) if np.isscalar(a) else 0 for a in alphas], dtype)
        self.bg = None if bg is None else np.ascontiguousarray(bg[f], dtype)
        self.L, self.C, self.P = len(covs), colors[0].shape[1], self.cov[0].size
        self.head = (self.L, self.C, self.P, _ptrs(self.cov), _ptrs(self.col), _ptrs(self.alpha), self.opacity.ctypes.data,
                     None if self.bg is None else self.bg.ctypes.data)


def _check(covs, colors, alphas):
    assert 1 <= len(covs) <= MAX_LAYERS and len(covs) == len(colors) == len(alphas), (len(covs), len(colors), len(alphas))


def forward(tmpdir, covs, colors, alphas, bg=None, through=False, dtype=np.float32):
    """covs[k] bool [n, rows, W] → out [n, C (+ 1), rows, W]"""
    _check(covs, colors, alphas)
    dtype = np.dtype(dtype).type
    n, Cn, rows, W = colors[0].shape
    out = np.zeros((n, Cn + (1 if through else 0), rows, W), dtype)
    for f in range(n):
        c = _Call(f, covs, colors, alphas, bg, dtype)
        o, T = np.zeros((Cn, rows, W), dtype), np.zeros((rows, W), dtype)
        lib(tmpdir, dtype).cmr_forward(*c.head, o.ctypes.data, T.ctypes.data if through else None)
        out[f, :Cn] = o
        if through:
            out[f, Cn] = T
    return out


def grad(tmpdir, covs, colors, alphas, gout, bg=None, through=False, dtype=np.float32):
    """gout [n, C (+ 1), rows, W] → (gcolors, galphas, gbg): every layer's [n, C, rows, W] and [n, 1, rows, W], and bg's shape or None"""
    _check(covs, colors, alphas)
    dtype = np.dtype(dtype).type
    n, Cn, rows, W = colors[0].shape
    assert gout.shape == (n, Cn + (1 if through else 0), rows, W), gout.shape
    gcol = [np.zeros((n, Cn, rows, W), dtype) for _ in covs]
    galpha = [np.zeros((n, 1, rows, W), dtype) for _ in covs]
    gbg = None if bg is None else np.zeros((n, Cn, rows, W), dtype)
    for f in range(n):
        c = _Call(f, covs, colors, alphas, bg, dtype)
        g = np.ascontiguousarray(gout[f, :Cn], dtype)
        gT = np.ascontiguousarray(gout[f, Cn], dtype) if through else None
        gc = [np.zeros((Cn, rows, W), dtype) for _ in covs]
        ga = [np.zeros((rows, W), dtype) for _ in covs]
        gb = None if bg is None else np.zeros((Cn, rows, W), dtype)
        lib(tmpdir, dtype).cmr_grad(*c.head, g.ctypes.data, None if gT is None else gT.ctypes.data, _ptrs(gc), _ptrs(ga),
                                    None if gb is None else gb.ctypes.data)
        for k in range(len(covs)):
            gcol[k][f], galpha[k][f, 0] = gc[k], ga[k]
        if gb is not None:
            gbg[f] = gb
    return gcol, galpha, gbg


def numpy_forward(covs, colors, alphas, bg=None, through=False):
    """the forward rule restated op by op in numpy float32, whole planes at a time (np.where keeps a skipped layer's words out)"""
    f32 = np.float32
    n, Cn, rows, W = colors[0].shape
    T, acc = np.ones((n, 1, rows, W), f32), np.zeros((n, Cn, rows, W), f32)
    with np.errstate(all="ignore"):
        for cov, col, a in zip(covs, colors, alphas):
            cv = cov[:, None]
            a = np.full((n, 1, rows, W), a, f32) if np.isscalar(a) else a.astype(f32)
            w = (a * T).astype(f32)
            acc = np.where(cv, (acc + (col.astype(f32) * w).astype(f32)).astype(f32), acc)
            T = np.where(cv, (T * (f32(1) - a).astype(f32)).astype(f32), T)
        if bg is not None:
            acc = (acc + (bg.astype(f32) * T).astype(f32)).astype(f32)
    return np.concatenate([acc, T], axis=1) if through else acc


def numpy_grad(covs, colors, alphas, gout, bg=None, through=False):
    """the backward rule restated op by op in numpy float32; the fused multiply-adds are libm's fmaf, element by element (small
    inputs only)"""
    import ctypes.util
    f32 = np.float32
    n, Cn, rows, W = colors[0].shape
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = C.c_float, [C.c_float] * 3
    fmaf = np.frompyfunc(lambda x, y, z: libm.fmaf(float(x), float(y), float(z)), 3, 1)

    def fma(a, b, c):
        a, b, c = np.broadcast_arrays(a, b, c)
        return fmaf(a, b, c).astype(f32)
    L = len(covs)
    T = np.ones((n, 1, rows, W), f32)
    A, Tk = [], []
    with np.errstate(all="ignore"):
        for cov, a in zip(covs, alphas):
            a = np.full((n, 1, rows, W), a, f32) if np.isscalar(a) else a.astype(f32)
            A.append(a), Tk.append(T)
            T = np.where(cov[:, None], (T * (f32(1) - a)).astype(f32), T)
        g = gout[:, :Cn].astype(f32)
        S = gout[:, Cn:Cn + 1].astype(f32) if through else np.zeros((n, 1, rows, W), f32)
        gbg = None
        if bg is not None:
            for c in range(Cn):
                S = fma(g[:, c:c + 1], bg[:, c:c + 1].astype(f32), S)
            gbg = (g * T).astype(f32)
        gcol, galpha = [None] * L, [None] * L
        for k in range(L - 1, -1, -1):
            cv = covs[k][:, None]
            w = (A[k] * Tk[k]).astype(f32)
            d = np.zeros((n, 1, rows, W), f32)
            for c in range(Cn):
                d = fma(g[:, c:c + 1], colors[k][:, c:c + 1].astype(f32), d)
            gcol[k] = np.where(cv, (g * w).astype(f32), f32(0))
            galpha[k] = np.where(cv, (Tk[k] * (d - S).astype(f32)).astype(f32), f32(0))
            S = np.where(cv, fma(A[k], d, ((f32(1) - A[k]).astype(f32) * S).astype(f32)), S)
    return gcol, galpha, gbg


# The binary32 gradients against the binary64 ones, measured by tests/test_composite_ref.py (random inputs in [0, 1], every layer
# covering, C = 3, bg and the transmittance plane; four seeds of 32 x 32 pixels): the largest error of each kind of plane relative to
# the plane's largest magnitude, by the number of layers.  No bound is derived; the tests hold an error to 8 x these.
GRAD_ERR = {3: {"gcolor": 1.15e-7, "galpha": 2.41e-7, "gbg": 9.4e-8}, 8: {"gcolor": 1.64e-7, "galpha": 2.53e-7, "gbg": 1.71e-7}}
