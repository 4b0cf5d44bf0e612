"""The texture pass's test reference (tests/tex_ref.c holds the arithmetic): a float texture [H, W, C] and per pixel (owner id word,
u, v) → the bilinearly sampled planes; and backward, the gradient planes with respect to u and v and the texture gradient
accumulated in double.  Built and loaded like tests/interpref.py's library; nothing of the product is involved."""
import ctypes as C

import numpy as np

from support import ref_lib

CLAMP, WRAP = 0, 1
OWNED, SAMPLED, OUTSIDE, WRAPPED = 1, 2, 4, 8  # classify()'s bits
vp = C.c_void_p
_head = [vp, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_size_t, vp, vp, vp]
SIGNATURES = {"tr_classify": (None, [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_size_t, vp, vp, vp, vp]),
              "tr_forward": (None, _head + [C.c_int, vp]),
              "tr_grad": (None, _head + [vp, C.c_int, vp, vp, vp, vp])}


def lib(tmpdir):
    return ref_lib("tex_ref", tmpdir, SIGNATURES)


def _planes(ids, uv):
    """ids [rows, W] uint32, uv [2, rows, W] float32 → contiguous planes and (rows, W)"""
    ids = np.ascontiguousarray(ids, np.uint32)
    uv = np.ascontiguousarray(uv, np.float32)
    assert ids.ndim == 2 and uv.shape == (2,) + ids.shape
    return ids, np.ascontiguousarray(uv[0]), np.ascontiguousarray(uv[1]), ids.shape


def _tex(tex):
    tex = np.ascontiguousarray(tex, np.float32)
    assert tex.ndim == 3
    return tex, tex.shape[0], tex.shape[1], tex.shape[2]


def classify(tmpdir, tex_hw, mode, n_tris, ids, uv):
    """[rows, W] uint8: OWNED | SAMPLED | OUTSIDE (sampled, CLAMP: in_x or in_y false) | WRAPPED (sampled, WRAP: x1 or y1 came back to 0)"""
    ids, u, v, (rows, W) = _planes(ids, uv)
    cls = np.zeros((rows, W), np.uint8)
    lib(tmpdir).tr_classify(tex_hw[1], tex_hw[0], mode, n_tris, rows * W, ids.ctypes.data, u.ctypes.data, v.ctypes.data, cls.ctypes.data)
    return cls


def forward(tmpdir, tex, mode, n_tris, ids, uv, fused=True, prefill=None):
    """tex: [H, W, C] float32; ids: [rows, W] uint32, plane 1 of one frame's visibility buffer; uv: [2, rows, W] float32 → [C, rows, W]
    float32.  prefill: [C, rows, W] uint32 words the planes start from (not fused: nobody's words stay)."""
    tex, H, W_, n_ch = _tex(tex)
    ids, u, v, (rows, W) = _planes(ids, uv)
    out = np.zeros((n_ch, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    assert out.shape == (n_ch, rows, W)
    lib(tmpdir).tr_forward(tex.ctypes.data, W_, H, n_ch, mode, n_tris, rows * W, ids.ctypes.data, u.ctypes.data, v.ctypes.data, int(fused),
                           out.ctypes.data)
    return out.view(np.float32)


class Grad:
    """the texture gradient of any number of frames, accumulated in double: .gtex [H, W, C] float64, .gabs the sums of |w * g|,
    .count [H, W] the contributing adds per texel"""

    def __init__(self, tex_shape):
        self.gtex, self.gabs = np.zeros(tex_shape, np.float64), np.zeros(tex_shape, np.float64)
        self.count = np.zeros(tex_shape[:2], np.uint32)

    def bound(self, extra=0):
        """per element: gamma_n * sum |w * g|, gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing adds (+ extra: the
        adds of a value the buffer held before; one rounding per add; the products are the float32 products themselves)"""
        n = (self.count.astype(np.float64)[:, :, None] + extra) * 2.0 ** -24
        return n / (1.0 - n) * self.gabs


def grad(tmpdir, tex, mode, n_tris, ids, uv, gout, into=None, want_uv=True, fused=True, prefill=None):
    """one frame's share: adds into `into` (a Grad, or None) and returns the guv planes [2, rows, W] float32 (None if not wanted)"""
    tex, H, W_, n_ch = _tex(tex)
    ids, u, v, (rows, W) = _planes(ids, uv)
    gout = np.ascontiguousarray(gout, np.float32)
    assert gout.shape == (n_ch, rows, W)
    guv = None
    if want_uv:
        guv = np.zeros((2, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    lib(tmpdir).tr_grad(tex.ctypes.data, W_, H, n_ch, mode, n_tris, rows * W, ids.ctypes.data, u.ctypes.data, v.ctypes.data, gout.ctypes.data,
                        int(fused), p(into.gtex) if into else None, p(into.gabs) if into else None, p(into.count) if into else None, p(guv))
    return guv.view(np.float32) if guv is not None else None


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
ZS = np.float32([1, 2, 3, 4])
TEX_SIZES = ((1, 1), (2, 2), (5, 7), (33, 1), (64, 64))  # (tex_w, tex_h)
FRAME_CASES = ("soup", "random", "uv-edge", "uv-overflow", "uv-nonfinite")
NON_FINITE_CASES = ("uv-nonfinite",)
# (frame case, mode) -> the texture sizes at which its uv do not reach the outermost half texel often enough for the border
# conditions of tests/test_tex_ref.py (a texture that fine under uv inside [0, 1]; uv of 3e38, whose fraction is 0: x0 wraps, not x1);
# every other combination is held to them, and every combination is compared on the GPU
NO_BORDER = {("soup", CLAMP): ((64, 64),), ("soup", WRAP): ((64, 64),), ("random", WRAP): ((64, 64),), ("uv-overflow", WRAP): ((5, 7), (64, 64)),
             ("uv-nonfinite", CLAMP): ((5, 7), (64, 64)), ("uv-nonfinite", WRAP): ((5, 7), (64, 64))}


def case_frame(name):
    """the 64 x 64 frame of a case: soup's uv lie inside [0, 1], random_frame's beyond it, the hostile families' at and far beyond the
    borders, and not finite"""
    import support
    from srz import abi
    if name == "soup":
        return support.frame(support.soup(0, 200, 64, 64, ZS), 64, 64)
    if name == "random":
        return support.random_frame(np.random.default_rng(5), 64, 64, 150, abi.FUSED_CLEAR)
    return support.hostile_shading_frame({"uv-edge": 0, "uv-overflow": 1, "uv-nonfinite": 3}[name], name)


def frame_uv(frame):
    """[n, 3, 2] float32: the uv of every triangle of an abi.Frame, in stream order"""
    return np.ascontiguousarray(np.concatenate([t["uv"] for t in frame.tris]), np.float32)


def make_tex(seed, w, h, n_ch, frames=None):
    """a texture [h, w, n_ch] (or [frames, h, w, n_ch]) of normal values, deterministic"""
    shape = (h, w, n_ch) if frames is None else (frames, h, w, n_ch)
    return np.random.default_rng([seed, w, h, n_ch]).normal(0, 3, shape).astype(np.float32)
