"""The perspective-correct barycentrics' test reference (tests/persp_ref.c holds the arithmetic): q [triangle][corner] and per pixel
(owner id word, alpha, beta) → the perspective buffer; backward, the gradient planes with respect to the screen-linear alpha, beta
and q's gradient accumulated in double; and the attribute derivatives under the rule.  Built and loaded like tests/interpref.py's
library; nothing of the product is involved."""
import ctypes as C

import numpy as np

import support
import vgkit
from support import ref_lib, word_planes

vp = C.c_void_p
SIGNATURES = {"pr_forward": (None, [vp, C.c_uint32, C.c_size_t, vp, vp, vp, vp, vp]),
              "pr_grad": (None, [vp, C.c_uint32, C.c_size_t, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]),
              "pr_deriv": (None, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_size_t, vp, vp, vp, C.c_int, vp])}
U = 2.0 ** -24
FLT_MIN = np.float32(2.0 ** -126)


def lib(tmpdir):
    return ref_lib("persp_ref", tmpdir, SIGNATURES)


def _q(q, n_tris):
    q = np.ascontiguousarray(q, np.float32)
    assert q.ndim == 2 and q.shape[1] == 3 and q.shape[0] >= n_tris
    return q


def forward(tmpdir, q, n_tris, vis_words):
    """q: [T, 3] float32 (T >= n_tris, the frame's triangle count); vis_words: [4, rows, W] uint32 of one frame's visibility buffer →
    the perspective buffer [4, rows, W] uint32, every word written"""
    q = _q(q, n_tris)
    (z, ids, al, be), (rows, W) = word_planes(vis_words)
    out = np.full((4, rows, W), 0xdeadbeef, np.uint32)
    lib(tmpdir).pr_forward(q.ctypes.data, n_tris, rows * W, z.ctypes.data, ids.ctypes.data, al.ctypes.data, be.ctypes.data, out.ctypes.data)
    return out


class Grad:
    """q's gradient of any number of frames, accumulated in double: .gq [T, 3] float64, .gabs the sums of |term|, .count [T] the
    contributing (valid) pixels per triangle"""

    def __init__(self, q_shape):
        self.gq, self.gabs = np.zeros(q_shape, np.float64), np.zeros(q_shape, np.float64)
        self.count = np.zeros(q_shape[0], np.uint32)

    def bound(self):
        """per element: gamma_n * sum |term|, gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing pixels (one
        rounding per add; the terms are the float32 products themselves)"""
        n = self.count.astype(np.float64)[:, None] * U
        return n / (1.0 - n) * self.gabs


def grad(tmpdir, q, n_tris, vis_words, gbp, into=None, want_bary=True, fused=True, prefill=None):
    """one frame's share: adds into `into` (a Grad, or None) and returns the gbary planes [2, rows, W] float32 (None if not wanted);
    gbp: [2, rows, W] float32, the gradient with respect to alpha', beta'"""
    q = _q(q, n_tris)
    (_, ids, al, be), (rows, W) = word_planes(vis_words)
    gbp = np.ascontiguousarray(gbp, np.float32)
    assert gbp.shape == (2, rows, W)
    gb = None
    if want_bary:
        gb = np.zeros((2, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    lib(tmpdir).pr_grad(q.ctypes.data, n_tris, rows * W, ids.ctypes.data, al.ctypes.data, be.ctypes.data, gbp.ctypes.data, int(fused),
                        p(into.gq) if into else None, p(into.gabs) if into else None, p(into.count) if into else None, p(gb))
    return gb.view(np.float32) if gb is not None else None


def deriv(tmpdir, q, pos, attr, n_tris, vis_words, fused=True, prefill=None):
    """pos: [T, 9] float32 screen positions; attr: [T, 3, C] float32 → the derivative planes [2 C, rows, W] float32"""
    q = _q(q, n_tris)
    pos, attr = np.ascontiguousarray(pos, np.float32).reshape(-1, 9), np.ascontiguousarray(attr, np.float32)
    n_ch = attr.shape[2]
    assert len(pos) >= n_tris and attr.shape[0] >= n_tris and attr.shape[1] == 3
    (_, ids, al, be), (rows, W) = word_planes(vis_words)
    out = np.zeros((2 * n_ch, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    assert out.shape == (2 * n_ch, rows, W)
    lib(tmpdir).pr_deriv(q.ctypes.data, pos.ctypes.data, attr.ctypes.data, n_ch, n_tris, rows * W, ids.ctypes.data, al.ctypes.data,
                         be.ctypes.data, int(fused), out.ctypes.data)
    return out.view(np.float32)


def valid32(q, s):
    """the rule's validity test on float32 values: q [..., 3], s [...]"""
    q, s = np.asarray(q, np.float32), np.asarray(s, np.float32)
    ok = lambda x: (x >= FLT_MIN) & (x < np.float32(np.inf))  # noqa: E731
    return ok(q[..., 0]) & ok(q[..., 1]) & ok(q[..., 2]) & ok(s)


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
# q values no pixel may be rewritten under; the last one is finite and positive, but overflows s with its like
HOSTILE_Q = np.float32([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan, 1e-40, 2.0 ** -149, 3e38])


def owners(vis_words, n_tris):
    """[rows, W] int64: the owner's triangle index, -1 where nobody (or a stranger) owns the pixel; and the S-class mask"""
    ids = np.asarray(vis_words[1], np.uint32)
    idx = (ids & np.uint32(0x7fffffff)).astype(np.int64) - 1
    own = (idx >= 0) & (idx < n_tris)
    return np.where(own, idx, -1), own & ((ids >> 31) != 0)


def make_q(seed, T, frames=None):
    """q [T, 3] (or [frames, T, 3]) uniform in [0.25, 4], deterministic"""
    shape = (T, 3) if frames is None else (frames, T, 3)
    return np.random.default_rng([seed, T]).uniform(0.25, 4.0, shape).astype(np.float32)


def hostile_q(seed, T):
    """make_q with a third of the triangles holding a HOSTILE_Q value in one, two or three corners"""
    rng = np.random.default_rng([seed, T, 7])
    q = make_q(seed, T)
    hit = rng.random(T) < 1.0 / 3
    mask = hit[:, None] & (rng.random((T, 3)) < 0.6)
    return np.where(mask, HOSTILE_Q[rng.integers(0, len(HOSTILE_Q), (T, 3))], q).astype(np.float32)


def tile_owner_counts(vis_words, n_tris, tile=32):
    """the number of distinct owners in every 32 x 32 tile → [tiles_y, tiles_x]"""
    idx, _ = owners(vis_words, n_tris)
    rows, W = idx.shape
    out = np.zeros(((rows + tile - 1) // tile, (W + tile - 1) // tile), np.int64)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            t = idx[ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile]
            out[ty, tx] = len(np.unique(t[t >= 0]))
    return out


# ------------------------------------------------------------------------------------------------ scenes under a real divide
def scene(pos, faces, m, w, h):
    """unit-coordinate mesh under ndc_mvp m → (abi.Frame, object positions [F, 3, 3] float64, q [F, 3] float32, m as float64 rows,
    the faces as they were wound)"""
    faces = vgkit.oriented(pos, faces, m)
    t = support.vertex_stage(vgkit.verts8(pos), faces, m, np.eye(4, dtype=np.float32).reshape(16), 1.0, 0.0)
    v = np.asarray(pos, np.float32)
    m32 = np.asarray(m, np.float32)
    r3 = (m32[3] * v[:, 0] + m32[7] * v[:, 1]) + (m32[11] * v[:, 2] + m32[15])  # (support.xform_div_w's fourth row, float32)
    assert r3.dtype == np.float32 and (r3 > 0).all()
    q = (np.float32(1) / r3)[faces.astype(np.int64)]
    rows = np.asarray(m, np.float64).reshape(4, 4).T
    return support.frame(t, w, h), v.astype(np.float64)[faces.astype(np.int64)], q.astype(np.float32), rows, faces


def quad_scene():
    """a flat unit quad receding along x: r3 runs from about 2 to 8 across it, so its far half is squeezed into a quarter of its
    width.  Cut into 3 x 2 cells (12 triangles), so that enough bounding boxes have scalar-tail columns"""
    pos, faces = vgkit.grid(4, 3, 0, z=0.5, jitter=0.0)
    pos[:, 2] = 0.5
    m = vgkit.perspective(190.0, 59.0, 1.5, 1.5, w=2.0, wx=6.0, wy=-0.25, wz=0.5)
    return scene(pos, faces, m, 64, 64)


def grid_scene():
    pos, faces = vgkit.grid(6, 5, 3)
    m = vgkit.perspective(70.0, 66.0, 2.0, 2.0, w=2.0, wx=1.5, wy=-0.25, wz=0.5)
    return scene(pos, faces, m, 64, 64)
