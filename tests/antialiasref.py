"""The silhouette antialiasing pass's test reference (tests/antialias_ref.c holds the arithmetic): a frame's positions [triangle][9],
its visibility buffer's z and id planes and the caller's planes → the blended planes and gin, bit for bit, the gradient with respect
to the positions accumulated in double with the sum of |term| and the count of contributing pairs per element, the pair counters, and
a double-precision restatement of the forward for finite differences.  Built and loaded like tests/posgradref.py's library; nothing
of the product is involved."""
import ctypes as C

import numpy as np

from support import ref_lib, word_planes

COUNTERS = ("differ", "target_n", "target_f", "horizontal", "vertical", "interior", "f_nobody", "no_edge")
vp = C.c_void_p
SIGNATURES = {"aa_forward": (None, [vp, C.c_uint32, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]),
              "aa_backward": (None, [vp, C.c_uint32, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]),
              "aa_forward64": (None, [vp, C.c_uint32, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp])}


def lib(tmpdir):
    return ref_lib("antialias_ref", tmpdir, SIGNATURES)


class Grad:
    """the position gradient of one frame, accumulated in double: .gpos [T, 3, 3] float64 (triangle, corner, (x, y, z)), .gabs the
    sums of |term|, .count [T, 3, 3] the contributing pairs per element, .counters the pair counts by name (COUNTERS)"""

    def __init__(self, tris):
        self.gpos, self.gabs = np.zeros((tris, 3, 3), np.float64), np.zeros((tris, 3, 3), np.float64)
        self.count = np.zeros((tris, 3, 3), np.uint32)
        self.raw = np.zeros(len(COUNTERS), np.uint64)

    @property
    def counters(self):
        return dict(zip(COUNTERS, (int(x) for x in self.raw)))

    def bound(self, calls=1):
        """per element: gamma_n * sum |term|, gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing pairs (one rounding
        per add; the terms are the float32 terms themselves); `calls`: the same call accumulated that many times"""
        n = calls * self.count.astype(np.float64) * 2.0 ** -24
        return n / (1.0 - n) * (calls * self.gabs)


def _planes(vis_words):
    (z, ids, _, _), (rows, W) = word_planes(vis_words)
    return z.view(np.float32), ids, rows, W


def _p(a):
    return a.ctypes.data if a is not None else None


def forward(tmpdir, pos, n_tris, vis_words, planes):
    """one frame: pos [T, 9] float32 (T >= n_tris, the frame's triangle count), vis_words [4, rows, W] uint32 of its visibility
    buffer, planes [C, rows, W] float32 → the blended planes [C, rows, W] float32"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    z, ids, rows, W = _planes(vis_words)
    c = np.ascontiguousarray(planes, np.float32)
    assert pos.shape[0] >= n_tris and c.shape[1:] == (rows, W)
    out = np.zeros_like(c)
    lib(tmpdir).aa_forward(_p(pos), n_tris, rows, W, _p(z), _p(ids), _p(c), c.shape[0], _p(out))
    return out


def backward(tmpdir, pos, n_tris, vis_words, planes, gout, into=None, want_gin=True, want_abs=False):
    """one frame: the gradient gout [C, rows, W] of the blended planes → gin [C, rows, W] float32 (None if not wanted; with want_abs
    also the per-word sums of |term| in float64), and the position gradient and the pair counters added into `into` (a Grad, or
    None)"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    z, ids, rows, W = _planes(vis_words)
    c, g = np.ascontiguousarray(planes, np.float32), np.ascontiguousarray(gout, np.float32)
    assert pos.shape[0] >= n_tris and c.shape[1:] == (rows, W) and g.shape == c.shape
    assert into is None or into.gpos.shape[0] >= n_tris
    gin = np.zeros_like(c) if want_gin else None
    mag = np.zeros(c.shape, np.float64) if want_gin and want_abs else None
    lib(tmpdir).aa_backward(_p(pos), n_tris, rows, W, _p(z), _p(ids), _p(c), _p(g), c.shape[0], _p(gin), _p(mag),
                            _p(into.gpos) if into else None, _p(into.gabs) if into else None, _p(into.count) if into else None,
                            _p(into.raw) if into else None)
    return (gin, mag) if want_abs else gin


def counters(tmpdir, pos, n_tris, vis_words):
    """the pair counts of one frame by name (COUNTERS)"""
    acc = Grad(max(n_tris, np.ascontiguousarray(pos).reshape(-1, 9).shape[0]))
    rows, W = np.asarray(vis_words).shape[1:]
    one = np.zeros((1, rows, W), np.float32)
    backward(tmpdir, pos, n_tris, vis_words, one, one, acc, want_gin=False)
    return acc.counters


def forward64(tmpdir, pos64, n_tris, vis_words, planes64):
    """the forward restated in float64 as a function of float64 positions [T, 9], owners and z held fixed → (planes [C, rows, W]
    float64, decision [2, rows, W] uint8: per pair with the right / lower neighbour, 0 = nothing, else which edge, which target
    and which pixel is nearer)"""
    pos = np.ascontiguousarray(pos64, np.float64).reshape(-1, 9)
    z, ids, rows, W = _planes(vis_words)
    c = np.ascontiguousarray(planes64, np.float64)
    assert pos.shape[0] >= n_tris and c.shape[1:] == (rows, W)
    out, dec = np.zeros_like(c), np.zeros((2, rows, W), np.uint8)
    lib(tmpdir).aa_forward64(_p(pos), n_tris, rows, W, _p(z), _p(ids), _p(c), c.shape[0], _p(out), _p(dec))
    return out, dec


# ------------------------------------------------------------------------------------------------ the scenes of the GPU tests
# (here, so that tests/test_antialias_ref.py can pin on the CPU the pair counts tests/test_gpu_antialias.py relies on)
ZS = np.float32([1, 2, 3, 4])
SIZES = [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6), (1, 1, 3), (1, 33, 6)]


def scene_tris(w, h, n, backdrop):
    """a soup of n triangles, in front of it two triangles that share a diagonal (an interior edge: identical vertex bits), and with
    `backdrop` one triangle behind everything that covers the frame — without it nobody's pixels border owners"""
    from support import ccw, soup
    s = min(w, h) * 0.2
    cx, cy = w * 0.5 + 0.3, h * 0.5 - 0.2
    a, b, c, d = (cx - s, cy - s), (cx + s, cy - s), (cx + s, cy + s), (cx - s, cy + s)
    quad = [ccw(a, b, d, z=0.5), ccw(b, c, d, z=0.5)]
    parts = [soup(2, n, w, h, ZS, big=w < 40)] + quad
    if backdrop:
        parts.append(ccw((-8, -8), (400, -8), (-8, 400), z=(80.0, 60.0, 70.0)))
    return np.concatenate(parts)


def relied_on(w, h, backdrop):
    """the counters (COUNTERS) that must be > 0 in every frame of scene (w, h, ., backdrop) for the GPU tests to exercise what they
    claim: what the frame's geometry allows — a single row has no vertical pair, a single column no horizontal one, a single pixel
    no pair at all; only without the backdrop does a nobody border an owner"""
    if w == 1 and h == 1:
        return ()
    if h == 1:
        return ("differ", "horizontal")
    if w == 1:
        return ("differ", "vertical")
    return ("differ", "target_n", "target_f", "horizontal", "vertical", "interior") + (() if backdrop else ("f_nobody",))
