"""The attribute interpolation's test reference (tests/interp_ref.c holds the arithmetic): the caller's attributes
[triangle][corner][channel] and per pixel (owner id word, alpha, beta) → the interpolated planes; and backward, the gradient planes
with respect to alpha and beta and the attribute gradient accumulated in double.  Built and loaded like tests/gbufref.py's library;
nothing of the product is involved."""
import ctypes as C

import numpy as np

from support import ref_lib, word_planes

vp = C.c_void_p
SIGNATURES = {"ir_forward": (None, [vp, C.c_uint32, C.c_uint32, C.c_size_t, vp, vp, vp, C.c_int, vp]),
              "ir_grad": (None, [vp, C.c_uint32, C.c_uint32, C.c_size_t, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp])}


def lib(tmpdir):
    return ref_lib("interp_ref", tmpdir, SIGNATURES)


def forward(tmpdir, attr, n_tris, vis_words, fused=True, prefill=None):
    """attr: [T, 3, C] float32 (T >= n_tris, the frame's triangle count); vis_words: [4, rows, W] uint32 of one frame's visibility
    buffer → [C, rows, W] float32.  prefill: [C, rows, W] uint32 words the planes start from (not fused: nobody's words stay)."""
    attr = np.ascontiguousarray(attr, np.float32)
    n_ch = attr.shape[2]
    (_, ids, al, be), (rows, W) = word_planes(vis_words)
    out = np.zeros((n_ch, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    assert out.shape == (n_ch, rows, W) and attr.shape[0] >= n_tris and attr.shape[1] == 3
    lib(tmpdir).ir_forward(attr.ctypes.data, n_ch, n_tris, rows * W, ids.ctypes.data, al.ctypes.data, be.ctypes.data, int(fused), out.ctypes.data)
    return out.view(np.float32)


class Grad:
    """the attribute gradient of any number of frames, accumulated in double: .gattr [T, 3, C] float64, .gabs the sums of |w * g|,
    .count [T] the contributing pixels per triangle"""

    def __init__(self, attr_shape):
        self.gattr, self.gabs = np.zeros(attr_shape, np.float64), np.zeros(attr_shape, np.float64)
        self.count = np.zeros(attr_shape[0], np.uint32)

    def bound(self):
        """per element: gamma_n * sum |w * g|, gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing pixels (one
        rounding per add; the products are the float32 products themselves)"""
        n = self.count.astype(np.float64)[:, None, None] * 2.0 ** -24
        return n / (1.0 - n) * self.gabs


def grad(tmpdir, attr, n_tris, vis_words, gout, into=None, want_bary=True, fused=True, prefill=None):
    """one frame's share: adds into `into` (a Grad, or None) and returns the gbary planes [2, rows, W] float32 (None if not wanted)"""
    attr = np.ascontiguousarray(attr, np.float32)
    n_ch = attr.shape[2]
    (_, ids, al, be), (rows, W) = word_planes(vis_words)
    gout = np.ascontiguousarray(gout, np.float32)
    assert gout.shape == (n_ch, rows, W) and attr.shape[0] >= n_tris
    gb = None
    if want_bary:
        gb = np.zeros((2, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    lib(tmpdir).ir_grad(attr.ctypes.data, n_ch, n_tris, rows * W, ids.ctypes.data, al.ctypes.data, be.ctypes.data, gout.ctypes.data, int(fused),
                        p(into.gattr) if into else None, p(into.gabs) if into else None, p(into.count) if into else None, p(gb))
    return gb.view(np.float32) if gb is not None else None


def frame_attr(frame, field):
    """[n, 3, k] float32: a field ("pos", "uv", "nrm") of every triangle of an abi.Frame, in stream order"""
    return np.ascontiguousarray(np.concatenate([t[field] for t in frame.tris]), np.float32)
