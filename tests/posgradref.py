"""The position gradient's test reference (tests/posgrad_ref.c holds the arithmetic): a frame's positions [triangle][9], per pixel
(owner id word, alpha, beta) and the gradient planes → the gradient with respect to the pixel's sample point, bit for bit, and the
gradient with respect to the positions accumulated in double.  Built and loaded like tests/interpref.py's library; nothing of the
product is involved."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "posgrad_ref.c")
_lib = None


def lib(tmpdir):
    global _lib
    if _lib is None:
        so = os.path.join(str(tmpdir), "libposgrad_ref.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        L = C.CDLL(so)
        vp = C.c_void_p
        L.pg_grad.argtypes = [vp, C.c_uint32, C.c_size_t, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
        L.pg_grad.restype = None
        _lib = L
    return _lib


class Grad:
    """the position gradient of one frame, accumulated in double: .gpos [T, 3, 3] float64 (triangle, corner, (x, y, z)), .gabs the
    sums of |term|, .count [T] the contributing pixels per triangle"""

    def __init__(self, tris):
        self.gpos, self.gabs = np.zeros((tris, 3, 3), np.float64), np.zeros((tris, 3, 3), np.float64)
        self.count = np.zeros(tris, np.uint32)

    def bound(self, calls=1):
        """per element: gamma_n * sum |term|, gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing pixels (one rounding
        per add; the terms are the float32 terms themselves); `calls`: the same call accumulated that many times"""
        n = calls * self.count.astype(np.float64)[:, None, None] * 2.0 ** -24
        return n / (1.0 - n) * (calls * self.gabs)


def frame_pos(frame):
    """[n, 9] float32: ax ay z0 bx by z1 cx cy z2 of every triangle of an abi.Frame, in stream order"""
    return np.ascontiguousarray(np.concatenate([t["pos"] for t in frame.tris]), np.float32).reshape(-1, 9)


def grad(tmpdir, pos, n_tris, vis_words, gbary=None, gz=None, into=None, want_pix=True, fused=True, prefill=None):
    """one frame: pos [T, 9] float32 (T >= n_tris, the frame's triangle count), vis_words [4, rows, W] uint32 of its visibility
    buffer, gbary [2, rows, W] and / or gz [1, rows, W] float32.  Adds into `into` (a Grad, or None) and returns the gpix planes
    [2, rows, W] float32 (None if not wanted).  prefill: [2, rows, W] uint32 words gpix starts from (not fused: nobody's words stay)."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    w = np.ascontiguousarray(vis_words, np.uint32)
    ids, al, be = (np.ascontiguousarray(w[p]) for p in (1, 2, 3))
    rows, W = w.shape[1:]
    assert pos.shape[0] >= n_tris and (gbary is not None or gz is not None)
    gb = None if gbary is None else np.ascontiguousarray(gbary, np.float32)
    g = None if gz is None else np.ascontiguousarray(gz, np.float32)
    assert gb is None or gb.shape == (2, rows, W)
    assert g is None or g.shape == (1, rows, W)
    assert into is None or into.gpos.shape[0] >= n_tris
    gp = None
    if want_pix:
        gp = np.zeros((2, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    lib(tmpdir).pg_grad(pos.ctypes.data, n_tris, rows * W, ids.ctypes.data, al.ctypes.data, be.ctypes.data, p(gb), p(g), int(fused),
                        p(into.gpos) if into else None, p(into.gabs) if into else None, p(into.count) if into else None, p(gp))
    return gp.view(np.float32) if gp is not None else None
