"""The background pass's test reference (tests/background_ref.c holds the arithmetic; the cube lookup inside it is tests/cube_ref.c's,
included): a ray block [9] (r0, rx, ry), a float cube [6, N, N, C] and one frame's owner ids → the planes the pass writes at the
pixels nobody owns (or at all pixels); and backward, the cube's gradient accumulated in double and the ray block's gradient in the
fixed tree, with the exact sums and the magnitudes the bounds are derived from.  Built and loaded like tests/cuberef.py's library;
nothing of the product is involved."""
import ctypes as C

import numpy as np

from support import ref_lib

NOBODY, ALL = 0, 1  # `where`
PASS, SAMPLED, CROSSED, VERTEX = 1, 2, 4, 8  # classify()'s bits
vp = C.c_void_p
SIGNATURES = {"br_dirs": (None, [vp, C.c_int, C.c_int, vp]),
              "br_classify": (None, [C.c_int, C.c_uint32, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp]),
              "br_forward": (None, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp]),
              "br_tree": (None, [C.c_int, C.c_int, vp, vp, vp]),
              "br_fold": (None, [C.c_int, vp, vp]),
              "br_grad_box": (None, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int,
                                     C.c_int]),
              "br_grad": (None, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp])}


def lib(tmpdir):
    return ref_lib("background_ref", tmpdir, SIGNATURES)


def _cube(cube):
    cube = np.ascontiguousarray(cube, np.float32)
    assert cube.ndim == 4 and cube.shape[0] == 6 and cube.shape[1] == cube.shape[2]
    return cube, cube.shape[1], cube.shape[3]


def _ray(ray):
    ray = np.ascontiguousarray(ray, np.float32).reshape(-1)
    assert ray.shape == (9,)
    return ray


def _ids(ids, shape, where):
    """ids [H, W] uint32, or None with where == ALL → (array or None, pointer, (H, W))"""
    if ids is None:
        assert where == ALL and shape is not None
        return None, None, tuple(shape)
    ids = np.ascontiguousarray(ids, np.uint32)
    assert ids.ndim == 2
    return ids, ids.ctypes.data, ids.shape


def dirs(tmpdir, ray, shape):
    """the direction planes [3, H, W] float32 the rule computes: d_c = fmaf(y, ry_c, fmaf(x, rx_c, r0_c))"""
    H, W = shape
    out = np.zeros((3, H, W), np.float32)
    lib(tmpdir).br_dirs(_ray(ray).ctypes.data, W, H, out.ctypes.data)
    return out


def classify(tmpdir, N, n_tris, ids, ray, where=NOBODY, shape=None):
    """([H, W] uint8: PASS | SAMPLED | CROSSED | VERTEX, [H, W] uint8: the face of a sampled pixel, else 255, [H, W, 4] uint32: the
    resolved texels of a sampled pixel)"""
    ids, ip, (H, W) = _ids(ids, shape, where)
    cls, face, at = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8), np.zeros((H, W, 4), np.uint32)
    lib(tmpdir).br_classify(N, n_tris, W, H, ip, _ray(ray).ctypes.data, where, cls.ctypes.data, face.ctypes.data, at.ctypes.data)
    return cls, face, at


def forward(tmpdir, cube, n_tris, ids, ray, where=NOBODY, fused=True, prefill=None, shape=None):
    """cube [6, N, N, C]; ids [H, W] uint32, plane 1 of one frame's visibility buffer (None with ALL: pass shape) → [C, H, W] float32.
    prefill: [C, H, W] uint32 words the planes start from (NOBODY, not fused: the owned words stay)."""
    cube, N, n_ch = _cube(cube)
    ids, ip, (H, W) = _ids(ids, shape, where)
    out = np.zeros((n_ch, H, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    assert out.shape == (n_ch, H, W)
    lib(tmpdir).br_forward(cube.ctypes.data, N, n_ch, n_tris, W, H, ip, _ray(ray).ctypes.data, where, int(fused), out.ctypes.data)
    return out.view(np.float32)


class Grad:
    """the gradients of any number of frames: .gtex [6, N, N, C] float64 with .gabs, the sums of |w * g|, and .count [6, N, N], the
    contributing adds per texel (cuberef.Grad's); .gsum [9] float64, the exact sum of the ray block's float32 terms, with .gmag, the
    sums of their magnitudes, and .n, the contributing pixels; .rows: the frames' rows [9] float32 in the fixed tree, in call order"""

    def __init__(self, cube_shape):
        self.gtex, self.gabs = np.zeros(cube_shape, np.float64), np.zeros(cube_shape, np.float64)
        self.count = np.zeros(cube_shape[:3], np.uint32)
        self.gsum, self.gmag, self.n = np.zeros(9, np.float64), np.zeros(9, np.float64), np.zeros(1, np.uint64)
        self.rows = []

    def bound(self, extra=0):
        """gtex, per element: gamma_n * sum |w * g|, gamma_n = n u / (1 - n u), u = 2^-24, n the element's contributing adds (+ extra:
        the adds of a value the buffer held before; one rounding per add; the products are the float32 products themselves)"""
        n = (self.count.astype(np.float64)[..., None] + extra) * 2.0 ** -24
        return n / (1.0 - n) * self.gabs

    def ray_bound(self):
        """gray, per entry: gamma_n * sum |term| with n the contributing pixels — the bound of any summation tree over n float32
        terms (include/srz.h, srz_frameset_light_grad)"""
        n = float(self.n[0]) * 2.0 ** -24
        return n / (1.0 - n) * self.gmag


def grad(tmpdir, cube, n_tris, ids, ray, gout, into, where=NOBODY, want_ray=True, shape=None):
    """one frame's share: adds into `into` (a Grad) and, want_ray, appends the frame's row to into.rows and returns it with the per
    pixel terms [9, H, W] float32 and the mask of contributing pixels [H, W]"""
    cube, N, n_ch = _cube(cube)
    ids, ip, (H, W) = _ids(ids, shape, where)
    gout = np.ascontiguousarray(gout, np.float32)
    assert gout.shape == (n_ch, H, W)
    term = smp = None
    if want_ray:
        term, smp = np.zeros((9, H, W), np.float32), np.zeros((H, W), np.uint8)
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    L = lib(tmpdir)
    L.br_grad(cube.ctypes.data, N, n_ch, n_tris, W, H, ip, _ray(ray).ctypes.data, where, gout.ctypes.data, p(into.gtex), p(into.gabs),
              p(into.count), p(term), p(smp), p(into.gsum), p(into.gmag), p(into.n))
    if not want_ray:
        return None
    row = tree(tmpdir, term, smp)
    into.rows.append(row)
    return row, term, smp.astype(bool)


def grad_box(tmpdir, cube, n_tris, ids, ray, gout, into, rows, cols, where=NOBODY, shape=None):
    """the cube's share of the pixels of the row and column slices alone (one tile's), added into `into`'s gtex, gabs and count"""
    cube, N, n_ch = _cube(cube)
    ids, ip, (H, W) = _ids(ids, shape, where)
    gout = np.ascontiguousarray(gout, np.float32)
    assert gout.shape == (n_ch, H, W)
    lib(tmpdir).br_grad_box(cube.ctypes.data, N, n_ch, n_tris, W, H, ip, _ray(ray).ctypes.data, where, gout.ctypes.data, into.gtex.ctypes.data,
                            into.gabs.ctypes.data, into.count.ctypes.data, cols.start, rows.start, cols.stop, rows.stop)


def tree(tmpdir, term, smp):
    """terms [9, H, W] float32 of the pixels smp [H, W] marks → their sums [9] float32 in the fixed tree"""
    term, smp = np.ascontiguousarray(term, np.float32), np.ascontiguousarray(smp, np.uint8)
    H, W = smp.shape
    row = np.zeros(9, np.float32)
    lib(tmpdir).br_tree(W, H, term.ctypes.data, smp.ctypes.data, row.ctypes.data)
    return row


def fold(tmpdir, rows):
    """rows [n, 9] float32 summed in order from +0: a shared block's frames"""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 9)
    out = np.zeros(9, np.float32)
    lib(tmpdir).br_fold(len(rows), rows.ctypes.data, out.ctypes.data)
    return out


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
def camera_block(w, h, seed=0, spread=1.0):
    """a ray block [9] float32 of a pinhole camera over a w x h frame, turned at random: the rays of the frame's pixels spread over
    about `spread` of a 90 degree field of view, so they cross faces, edges and, at spread >= 1.5, cube vertices"""
    rng = np.random.default_rng([seed, w, h])
    q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
    s = 2.0 * spread / max(w, h, 2)
    r0 = q[:, 2] - 0.5 * s * (w * q[:, 0] + h * q[:, 1])
    return np.concatenate([r0, s * q[:, 0], s * q[:, 1]]).astype(np.float32)


def sweep_block(step_texels, N):
    """a block whose rays step `step_texels` texels of an N x N face per pixel in x and in y across the +Z face's neighbourhood,
    starting near a corner of it: a 32 x 32 tile then spans 32 * step texels each way"""
    s = np.float32(2.0 * step_texels / N)
    return np.float32([-0.97, 0.93, 1.0, s, 0.0, 0.0, 0.0, -s, 0.0])


def vertex_block(w, h, corner, spread=2.0):
    """a pinhole block over a w x h frame that looks at the cube vertex `corner` (three signs): its rays cross the vertex region and
    the three edges that meet there, from both of their faces"""
    f = np.float64(corner) / np.sqrt(3.0)
    a = np.cross(f, [0.3, 0.5, 0.8])
    a /= np.linalg.norm(a)
    b = np.cross(f, a)
    s = 2.0 * spread / max(w, h, 2)
    r0 = f - 0.5 * s * (w * a + h * b)
    return np.concatenate([r0, s * a, s * b]).astype(np.float32)


CORNERS = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]


# the reference's camera in binary64, mathematical layout (S @ (P, 1) = (x w, y w, z w, w)): glm's lookAtLH and perspectiveLH_NO and the
# host layer's NDC-to-screen matrix, restated
def look_at_lh(eye, center, up):
    f = (center - eye) / np.linalg.norm(center - eye)
    s = np.cross(up, f)
    s /= np.linalg.norm(s)
    u = np.cross(f, s)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, f
    m[:3, 3] = -m[:3, :3] @ eye
    return m


def perspective_lh_no(fovy, aspect, near, far):
    t = np.tan(fovy / 2)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1], m[2, 2], m[3, 2], m[2, 3] = 1 / (aspect * t), 1 / t, (far + near) / (far - near), 1.0, -2 * far * near / (far - near)
    return m


def screen(w, h):
    m = np.eye(4)
    m[0, 0], m[1, 1], m[0, 3], m[1, 3] = w / 2 * (w / h), h / 2, w / 2, h / 2
    return m


def camera_matrix(eye, center, up, fovy, w, h, near=0.1, far=100.0):
    """screen <- world of the reference's camera → [4, 4] float64"""
    eye, center, up = np.float64(eye), np.float64(center), np.float64(up)
    return screen(w, h) @ perspective_lh_no(fovy, w / h, near, far) @ look_at_lh(eye, center, up)
