"""The cube lookup's test reference (tests/cube_ref.c holds the arithmetic): a float cube map [6, N, N, C] and per pixel (owner id
word, direction) → the seamlessly, bilinearly sampled planes; and backward, the gradient planes with respect to the direction and the
cube's gradient accumulated in double.  Built and loaded like tests/texref.py's library; nothing of the product is involved."""
import ctypes as C

import numpy as np

from support import ref_lib

OWNED, SAMPLED, CROSSED, VERTEX = 1, 2, 4, 8  # classify()'s bits
FACES = ("+X", "-X", "+Y", "-Y", "+Z", "-Z")
# face -> (n, su, sv): include/srz.h's table
AXES = (((1, 0, 0), (0, 0, -1), (0, -1, 0)), ((-1, 0, 0), (0, 0, 1), (0, -1, 0)), ((0, 1, 0), (1, 0, 0), (0, 0, 1)),
        ((0, -1, 0), (1, 0, 0), (0, 0, -1)), ((0, 0, 1), (1, 0, 0), (0, -1, 0)), ((0, 0, -1), (-1, 0, 0), (0, -1, 0)))
vp = C.c_void_p
_head = [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_size_t, vp, vp, vp, vp]
SIGNATURES = {"cr_resolve": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, vp]),
              "cr_taps": (None, [C.c_int, C.c_int, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]),
              "cr_classify": (None, [C.c_int, C.c_uint32, C.c_size_t, vp, vp, vp, vp, vp, vp]),
              "cr_forward": (None, _head + [C.c_int, C.c_int, vp]),
              "cr_grad": (None, _head + [vp, C.c_int, C.c_int, vp, vp, vp, vp])}


def lib(tmpdir):
    return ref_lib("cube_ref", tmpdir, SIGNATURES)


def resolve(tmpdir, N, face, x, y):
    """texel (x, y) of `face`, x and y in [-1, N] → (face, x, y) resolved, and whether it lay outside in both axes"""
    out = np.zeros(3, np.int32)
    both = lib(tmpdir).cr_resolve(N, face, x, y, out.ctypes.data)
    return (int(out[0]), int(out[1]), int(out[2])), bool(both)


def taps(tmpdir, N, dirs, force=-1):
    """dirs [n, 3] float32 → dict of face [n] (-1: unsampled), st [n, 2], x0y0 [n, 2], frac [n, 2], at [n, 4] (texel index in the
    cube), w [n, 4]; force >= 0: through that face"""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    n = len(d)
    r = dict(face=np.zeros(n, np.int32), st=np.zeros((n, 2), np.float32), x0y0=np.zeros((n, 2), np.int32), frac=np.zeros((n, 2), np.float32),
             at=np.zeros((n, 4), np.uint32), w=np.zeros((n, 4), np.float32))
    lib(tmpdir).cr_taps(N, force, n, d.ctypes.data, *(r[k].ctypes.data for k in ("face", "st", "x0y0", "frac", "at", "w")))
    return r


def _planes(ids, dirs):
    """ids [rows, W] uint32, dirs [3, rows, W] float32 → contiguous planes and (rows, W)"""
    ids = np.ascontiguousarray(ids, np.uint32)
    dirs = np.ascontiguousarray(dirs, np.float32)
    assert ids.ndim == 2 and dirs.shape == (3,) + ids.shape
    return ids, [np.ascontiguousarray(dirs[k]) for k in range(3)], ids.shape


def _cube(cube):
    cube = np.ascontiguousarray(cube, np.float32)
    assert cube.ndim == 4 and cube.shape[0] == 6 and cube.shape[1] == cube.shape[2]
    return cube, cube.shape[1], cube.shape[3]


def classify(tmpdir, N, n_tris, ids, dirs):
    """([rows, W] uint8: OWNED | SAMPLED | CROSSED (a corner on another face) | VERTEX (a corner outside in both axes), [rows, W]
    uint8: the face of a sampled pixel, else 255)"""
    ids, d, (rows, W) = _planes(ids, dirs)
    cls, face = np.zeros((rows, W), np.uint8), np.zeros((rows, W), np.uint8)
    lib(tmpdir).cr_classify(N, n_tris, rows * W, ids.ctypes.data, d[0].ctypes.data, d[1].ctypes.data, d[2].ctypes.data, cls.ctypes.data,
                            face.ctypes.data)
    return cls, face


def forward(tmpdir, cube, n_tris, ids, dirs, fused=True, prefill=None, force=-1):
    """cube: [6, N, N, C] float32; ids: [rows, W] uint32, plane 1 of one frame's visibility buffer; dirs: [3, rows, W] float32 →
    [C, rows, W] float32.  prefill: [C, rows, W] uint32 words the planes start from (not fused: nobody's words stay)."""
    cube, N, n_ch = _cube(cube)
    ids, d, (rows, W) = _planes(ids, dirs)
    out = np.zeros((n_ch, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    assert out.shape == (n_ch, rows, W)
    lib(tmpdir).cr_forward(cube.ctypes.data, N, n_ch, n_tris, rows * W, ids.ctypes.data, d[0].ctypes.data, d[1].ctypes.data, d[2].ctypes.data,
                           int(fused), force, out.ctypes.data)
    return out.view(np.float32)


def sample(tmpdir, cube, dirs, force=-1):
    """dirs [n, 3] → [n, C]: every direction a pixel with an owner"""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    out = forward(tmpdir, cube, 1, np.ones((1, len(d)), np.uint32), d.T.reshape(3, 1, -1), force=force)
    return out[:, 0].T


class Grad:
    """the cube's gradient of any number of frames, accumulated in double: .gtex [6, N, N, C] float64, .gabs the sums of |w * g|,
    .count [6, N, N] the contributing adds per texel"""

    def __init__(self, cube_shape):
        self.gtex, self.gabs = np.zeros(cube_shape, np.float64), np.zeros(cube_shape, np.float64)
        self.count = np.zeros(cube_shape[:3], np.uint32)

    def bound(self, extra=0):
        """per element: gamma_n * sum |w * g|, gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing adds (+ extra: the
        adds of a value the buffer held before; one rounding per add; the products are the float32 products themselves)"""
        n = (self.count.astype(np.float64)[..., None] + extra) * 2.0 ** -24
        return n / (1.0 - n) * self.gabs


def grad(tmpdir, cube, n_tris, ids, dirs, gout, into=None, want_dir=True, fused=True, prefill=None, force=-1):
    """one frame's share: adds into `into` (a Grad, or None) and returns the gdir planes [3, rows, W] float32 (None if not wanted)"""
    cube, N, n_ch = _cube(cube)
    ids, d, (rows, W) = _planes(ids, dirs)
    gout = np.ascontiguousarray(gout, np.float32)
    assert gout.shape == (n_ch, rows, W)
    gdir = None
    if want_dir:
        gdir = np.zeros((3, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    lib(tmpdir).cr_grad(cube.ctypes.data, N, n_ch, n_tris, rows * W, ids.ctypes.data, d[0].ctypes.data, d[1].ctypes.data, d[2].ctypes.data,
                        gout.ctypes.data, int(fused), force, p(into.gtex) if into else None, p(into.gabs) if into else None,
                        p(into.count) if into else None, p(gdir))
    return gdir.view(np.float32) if gdir is not None else None


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
CUBE_SIZES = (1, 2, 5, 8, 64)
SPECIALS = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0, 1.0, -1.0, 0.5, 1e-40, -3e-42])


def make_cube(seed, n, n_ch, frames=None):
    """a cube [6, n, n, n_ch] (or [frames, 6, n, n, n_ch]) of normal values, deterministic"""
    shape = (6, n, n, n_ch) if frames is None else (frames, 6, n, n, n_ch)
    return np.random.default_rng([seed, n, n_ch]).normal(0, 3, shape).astype(np.float32)


def edge_dirs():
    """the 12 edges x 29 dyadic directions (+-1, +-1, k / 16), |k| <= 14, in all three axis pairs → ([348, 3] float32, face A [348],
    face B [348]): the two faces that meet in the edge"""
    d, fa, fb = [], [], []
    for m1, m2 in ((0, 1), (0, 2), (1, 2)):
        for s1 in (1, -1):
            for s2 in (1, -1):
                for k in range(-14, 15):
                    v = np.zeros(3, np.float32)
                    v[m1], v[m2], v[3 - m1 - m2] = s1, s2, k / 16.0
                    d.append(v), fa.append(2 * m1 + (s1 < 0)), fb.append(2 * m2 + (s2 < 0))
    return np.stack(d), np.array(fa), np.array(fb)


def hostile_dirs(rng, shape, n):
    """direction planes [3, rows, W] float32 by hand that hit every face, every edge from both sides, the vertex regions, the ties,
    +-0 and the values that are not sampled or nearly not: uniform directions, a share of them snapped onto edges (two components of
    equal magnitude, the third small), vertices (three of nearly equal magnitude), axes with signed zeros, and SPECIALS"""
    rows, W = shape
    d = rng.normal(0, 1, (rows, W, 3)).astype(np.float32)
    kind = rng.integers(0, 10, (rows, W))
    e = kind == 1  # near an edge, from both sides: a second component within a texel of the major one
    for r, c in np.argwhere(e):
        o = rng.permutation(3)
        m = np.float32(rng.uniform(0.5, 2))
        d[r, c, o[0]] = m * rng.choice([-1, 1])
        d[r, c, o[1]] = m * rng.choice([-1, 1]) * np.float32(1 - rng.choice([0, 0, 0.3, 1, 1.7]) * rng.uniform(0, 1) / n)
        d[r, c, o[2]] = m * np.float32(rng.uniform(-1, 1))
    v = kind == 2  # the vertex regions: all three within half a texel or so
    d[v] = (rng.choice([-1.0, 1.0], (int(v.sum()), 3)) * (1 - rng.uniform(0, 1.2, (int(v.sum()), 3)) / n)).astype(np.float32)
    t = kind == 3  # exact ties and signed zeros
    d[t] = rng.choice(np.float32([-1, 1, 0.0, -0.0, 0.5, -0.5]), (int(t.sum()), 3))
    s = kind == 4
    hit = rng.random((rows, W, 3)) < 0.5
    sp = SPECIALS[rng.integers(0, len(SPECIALS), (rows, W, 3))]
    d[s] = np.where(hit[s], sp[s], d[s])
    sub = kind == 5  # subnormal directions: sampled, by IEEE division
    d[sub] = (rng.integers(-2000, 2001, (int(sub.sum()), 3)) * np.float64(2.0 ** -149)).astype(np.float32)
    return np.ascontiguousarray(d.transpose(2, 0, 1))
