"""The position gradient's test reference (tests/posgrad_ref.c holds the arithmetic): a frame's positions [triangle][9], per pixel
(owner id word, alpha, beta) and the gradient planes → the gradient with respect to the pixel's sample point, bit for bit, and the
gradient with respect to the positions accumulated in double.  Built and loaded like tests/interpref.py's library; nothing of the
product is involved."""
import ctypes as C

import numpy as np

from support import ref_lib, word_planes

vp = C.c_void_p
SIGNATURES = {"pg_grad": (None, [vp, C.c_uint32, C.c_size_t, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp])}


def lib(tmpdir):
    return ref_lib("posgrad_ref", tmpdir, SIGNATURES)


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


def grad(tmpdir, pos, n_tris, vis_words, gbary=None, gz=None, into=None, want_pix=True, fused=True, prefill=None):
    """one frame: pos [T, 9] float32 (T >= n_tris, the frame's triangle count), vis_words [4, rows, W] uint32 of its visibility
    buffer, gbary [2, rows, W] and / or gz [1, rows, W] float32.  Adds into `into` (a Grad, or None) and returns the gpix planes
    [2, rows, W] float32 (None if not wanted).  prefill: [2, rows, W] uint32 words gpix starts from (not fused: nobody's words stay)."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    (_, ids, al, be), (rows, W) = word_planes(vis_words)
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
