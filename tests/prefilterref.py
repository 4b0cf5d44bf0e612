"""The cube prefilter's test reference (tests/prefilter_ref.c holds the arithmetic): a cube [6, N_s, N_s, C] (or [frames, 6, N_s,
N_s, C]) convolved into a cube of N_d x N_d faces with the cosine or the GGX lobe, the normaliser, the count of unskipped pairs per
output texel, and the backward (the exact transpose).  Built twice: binary32 (dtype np.float32, the arithmetic the library is held
to) and binary64 (np.float64, the same text in double).  Nothing of the product is involved."""
import ctypes as C
import os

import numpy as np

from support import build_c, ref_lib

COSINE, GGX = 0, 1
vp = C.c_void_p
SIGNATURES = {"pfr_real_bytes": (C.c_int, []),
              "pfr_geometry": (None, [C.c_int, vp, vp]),
              "pfr_forward": (None, [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_float, vp, vp, vp]),
              "pfr_grad": (None, [vp, vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_float, vp])}
_lib64 = {}


def lib(tmpdir, dtype=np.float32):
    """the binary32 build (support.ref_lib's cache) or, dtype np.float64, the same file built with -DPFR_DOUBLE"""
    if np.dtype(dtype) == np.float32:
        L = ref_lib("prefilter_ref", tmpdir, SIGNATURES)
        assert L.pfr_real_bytes() == 4
        return L
    assert np.dtype(dtype) == np.float64
    if "L" not in _lib64:
        L = C.CDLL(build_c("prefilter_ref", os.path.join(str(tmpdir), "libprefilter_ref64.so"), "-O2", "-shared", "-fPIC", "-DPFR_DOUBLE"))
        for fn, (restype, argtypes) in SIGNATURES.items():
            getattr(L, fn).restype, getattr(L, fn).argtypes = restype, argtypes
        assert L.pfr_real_bytes() == 8
        _lib64["L"] = L
    return _lib64["L"]


def _dims(cube):
    assert cube.ndim in (4, 5) and cube.shape[-4] == 6 and cube.shape[-3] == cube.shape[-2], cube.shape
    return (cube.shape[0] if cube.ndim == 5 else 1), cube.shape[-2], cube.shape[-1]


def geometry(tmpdir, n, dtype=np.float32):
    """→ (d [6, n, n, 3], jac [6, n, n]) of every texel of an n x n cube"""
    d, jac = np.zeros((6, n, n, 3), dtype), np.zeros((6, n, n), dtype)
    lib(tmpdir, dtype).pfr_geometry(n, d.ctypes.data, jac.ctypes.data)
    return d, jac


def forward(tmpdir, cube, n_dst, kind, roughness=1.0, cmin=0.0, dtype=np.float32):
    """cube [6, N, N, C] or [frames, 6, N, N, C] → (dst, the cube's shape at n_dst; den [6, n_dst, n_dst]; count [6, n_dst, n_dst]
    uint32, the pairs of each output texel that were not skipped)"""
    cube = np.ascontiguousarray(cube, dtype)
    frames, n_src, n_ch = _dims(cube)
    dst = np.zeros(cube.shape[:-3] + (n_dst, n_dst, n_ch), dtype)
    den, count = np.zeros((6, n_dst, n_dst), dtype), np.zeros((6, n_dst, n_dst), np.uint32)
    lib(tmpdir, dtype).pfr_forward(cube.ctypes.data, n_src, n_dst, n_ch, frames, kind, roughness, cmin, dst.ctypes.data, den.ctypes.data,
                                   count.ctypes.data)
    return dst, den, count


def grad(tmpdir, gdst, den, n_src, kind, roughness=1.0, cmin=0.0, dtype=np.float32):
    """gdst: the forward's output shape; den: as the forward returned it → gsrc, the cube's shape at n_src"""
    gdst, den = np.ascontiguousarray(gdst, dtype), np.ascontiguousarray(den, dtype)
    frames, n_dst, n_ch = _dims(gdst)
    assert den.shape == (6, n_dst, n_dst)
    gsrc = np.zeros(gdst.shape[:-3] + (n_src, n_src, n_ch), dtype)
    lib(tmpdir, dtype).pfr_grad(gdst.ctypes.data, den.ctypes.data, n_src, n_dst, n_ch, frames, kind, roughness, cmin, gsrc.ctypes.data)
    return gsrc


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
# (n_src, n_dst, kind, roughness, cmin) with a known share of output texels that no pair reaches (den == 0): between 0.1 and 0.6 for
# the first two, every texel for the third
EMPTY_CASES = [(3, 8, GGX, 0.5, 0.97), (2, 5, COSINE, 1.0, 0.9), (4, 8, COSINE, 1.0, 0.999)]


HOSTILE = np.float32([np.inf, -np.inf, np.nan, 1e-40, -3e-39, 3e38, -3e38])


def hostile_cube(rng, shape):
    """texels in [0, 1] with each of HOSTILE (+inf, -inf, NaN, subnormals, 3e38) at one seeded element: few enough that a cutoff
    leaves output texels none of them reaches"""
    cube = rng.uniform(0.0, 1.0, shape).astype(np.float32)
    cube.reshape(-1)[rng.choice(cube.size, len(HOSTILE), replace=False)] = HOSTILE
    return cube
