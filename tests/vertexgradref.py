"""The test reference of the vertex stage's backward (tests/vertex_grad_ref.c holds the rule, verbatim): the gradient of the triangles'
screen positions → the gradient of a mesh's vertex positions in float32, bit for bit, and of each draw's matrix and depth mapping
accumulated in double, with what the bound needs.  It makes its own corner lists.  Built and loaded like tests/posgradref.py's library;
nothing of the product is involved."""
import ctypes as C

import numpy as np

from support import ref_lib

vp, u32 = C.c_void_p, C.c_uint32
SIGNATURES = {"vg_corner_lists": (None, [vp, u32, u32, vp, vp, vp]),
              "vg_draw": (None, [vp, u32, vp, vp, vp, u32, vp, C.c_float, vp, vp, vp, vp])}


def lib(tmpdir):
    return ref_lib("vertex_grad_ref", tmpdir, SIGNATURES)


def corner_lists(tmpdir, faces, n_verts):
    """(off [n_verts + 1], corners [3 * n_faces]) uint32 of a face list: vertex v is named by corners[off[v]:off[v + 1]], each
    3 * face + k, increasing"""
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    assert f.size == 0 or int(f.max()) < n_verts
    off, corners, scratch = np.zeros(n_verts + 1, np.uint32), np.zeros(max(1, f.size), np.uint32), np.zeros(max(1, n_verts), np.uint32)
    lib(tmpdir).vg_corner_lists(f.ctypes.data, len(f), n_verts, off.ctypes.data, corners.ctypes.data, scratch.ctypes.data)
    return off, corners[:f.size]


class DrawGrad:
    """the gradient of every draw's 18 values (ndc_mvp's 16 in its own order, zscale, zoffset), accumulated in double: .gdraw
    [n_frames, D, 18] float64, .gabs the sums of |term|, .count [n_frames, D] the contributing vertices per draw"""

    def __init__(self, n_frames, n_draws):
        self.gdraw, self.gabs = np.zeros((n_frames, n_draws, 18), np.float64), np.zeros((n_frames, n_draws, 18), np.float64)
        self.count = np.zeros((n_frames, n_draws), np.uint32)

    def bound(self):
        """per element: gamma_n * sum |term|, gamma_n = n u / (1 - n u), u = 2^-24, n the draw's contributing vertices (one rounding per
        add whatever the order and tree; the terms are the float32 terms themselves) — posgradref.Grad.bound's form"""
        n = self.count.astype(np.float64)[:, :, None] * 2.0 ** -24
        return n / (1.0 - n) * self.gabs


def grad(tmpdir, verts8, faces, frames, mesh_id, gpos, gverts=None, into=None):
    """one mesh.  verts8 [V, 8] float32, faces [F, 3]; frames: per frame its draws in draw order, each (mesh slot, face count, ndc_mvp
    [16], zscale); gpos [n_frames, T, 9] float32, triangle index frame-local.  The draws that name mesh_id take part.  gverts: a
    [n_frames, V, 3] float32 array ADDED into by the rule (None: not wanted); into: a DrawGrad added into (None: not wanted)."""
    v8 = np.ascontiguousarray(verts8, np.float32).reshape(-1, 8)
    V = len(v8)
    off, corners = corner_lists(tmpdir, faces, V)
    corners = np.ascontiguousarray(np.concatenate([corners, np.zeros(1, np.uint32)]))  # (never empty: a pointer to pass)
    gpos = np.ascontiguousarray(gpos, np.float32).reshape(len(frames), -1, 9)
    assert gverts is None or (gverts.dtype == np.float32 and gverts.shape == (len(frames), V, 3) and gverts.flags.c_contiguous)
    n_faces = len(np.asarray(faces).reshape(-1, 3))
    for f, draws in enumerate(frames):
        first = 0
        for j, (slot, nf, mvp, zs) in enumerate(draws):
            if slot == mesh_id:
                assert nf == n_faces and first + nf <= gpos.shape[1]
                m = np.ascontiguousarray(mvp, np.float32).reshape(16)
                p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
                lib(tmpdir).vg_draw(v8.ctypes.data, V, off.ctypes.data, corners.ctypes.data, gpos[f].ctypes.data, first, m.ctypes.data,
                                    float(np.float32(zs)), p(gverts[f]) if gverts is not None else None,
                                    p(into.gdraw[f, j]) if into else None, p(into.gabs[f, j]) if into else None,
                                    p(into.count[f, j:j + 1]) if into else None)
            first += nf
    return gverts
