"""The G-buffer's test reference (tests/gbuf_ref.c holds the arithmetic): a frame's triangle records, its batch table with the
textures, and per pixel (owner id word, alpha, beta) → the nine planes of every group, as uint32 words.  Built and loaded like
tests/visref.py's library; nothing of the product is involved."""
import ctypes as C

import numpy as np

from srz import abi
from support import ref_lib, word_planes

GROUPS = ((abi.GB_NORMAL, (0, 1, 2)), (abi.GB_UV, (3, 4)), (abi.GB_BATCH, (5,)), (abi.GB_ALBEDO, (6, 7, 8)))


class GrBatch(C.Structure):
    _fields_ = [("shader", C.c_int32), ("tw", C.c_int32), ("th", C.c_int32), ("_pad", C.c_int32), ("bgr", C.c_void_p)]


vp = C.c_void_p
SIGNATURES = {"gr_gbuffer": (None, [vp, C.c_uint32, vp, C.POINTER(GrBatch), C.c_size_t, vp, vp, vp, C.c_int, vp])}


def lib(tmpdir):
    return ref_lib("gbuf_ref", tmpdir, SIGNATURES)


def planes_of(what):
    """indices into the nine planes of the groups in `what`, in buffer order"""
    return [i for bit, idx in GROUPS if what & bit for i in idx]


def expected(tmpdir, frame, textures, vis_words, fused=True, prefill=None, shading=None):
    """vis_words: [4, rows, W] uint32 of one frame's visibility buffer (planes z, id, alpha, beta) → [9, rows, W] uint32.
    textures: slot -> (h, w, 3) uint8; shading: [(shader, tex_id)] per batch instead of the frame's own; prefill: [9, rows, W] uint32
    the planes start from (not fused: nobody's words stay)."""
    L = lib(tmpdir)
    sizes = [len(t) for t in frame.tris]
    n = sum(sizes)
    tris = np.ascontiguousarray(np.concatenate(frame.tris)).view(np.float32).reshape(-1, 24) if n else np.zeros((1, 24), np.float32)
    tri_batch = np.ascontiguousarray(np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)) if n else np.zeros(1, np.int32)
    shading = shading or [(int(frame._batches[b].shader), int(frame._batches[b].tex_id)) for b in range(len(sizes))]
    keep = []
    table = (GrBatch * max(1, len(sizes)))()
    for b, (sh, slot) in enumerate(shading):
        tex = textures.get(slot) if sh in (abi.SHADER_TEXTURE, abi.SHADER_BUMP, abi.SHADER_DISPLACEMENT) else None
        if tex is None:
            table[b] = GrBatch(sh, 1, 1, 0, None)
        else:
            t = np.ascontiguousarray(tex, np.uint8)
            keep.append(t)
            table[b] = GrBatch(sh, t.shape[1], t.shape[0], 0, t.ctypes.data)
    (_, ids, al, be), (rows, W) = word_planes(vis_words)
    out = np.zeros((9, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    L.gr_gbuffer(tris.ctypes.data, n, tri_batch.ctypes.data, table, rows * W, ids.ctypes.data, al.ctypes.data, be.ctypes.data, int(fused),
                 out.ctypes.data)
    return out


# ---- the oracle anchors: what the built-in shaders make of the G-buffer's values, restated in numpy float32 (every step one correctly
# rounded binary32 operation) -------------------------------------------------------------------------------------------------------
def normal_colour(n, s_class):
    """the NORMAL shader's colour [3, ...] float32 of normals n [3, ...] float32 (the G-buffer's) per class.  V (src/Shader.cpp:157-174):
    min(max((n + 1) * 0.5, 0), 1) * 255; S: glm::normalize once more (scalar applyFragmentShader), (n + 1) / 2, clamp, * 255, truncated"""
    n = np.asarray(n, np.float32)
    one, half, two, c255 = np.float32(1), np.float32(0.5), np.float32(2), np.float32(255)
    cv = (n + one) * half
    cv = np.where(cv > 0, cv, np.float32(0))
    v = np.where(cv < one, cv, one) * c255
    with np.errstate(all="ignore"):
        dot = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        inv = one / np.sqrt(dot)
        cs = ((n * inv) + one) / two
        cs = np.where(cs < 0, np.float32(0), np.where(one < cs, one, cs)) * c255
        s = np.trunc(cs)
    out = np.where(s_class, s, v).astype(np.float32)
    assert out.dtype == np.float32 and cv.dtype == np.float32 and cs.dtype == np.float32 and dot.dtype == np.float32
    return out


def albedo_colour(kd, s_class):
    """the colour of albedo_frame's pixels from the G-buffer's albedo: kd * 255 (V), trunc(kd * 255) (S)"""
    c = np.asarray(kd, np.float32) * np.float32(255)
    return np.where(s_class, np.trunc(c), c).astype(np.float32)


def albedo_frame(f, remap=None):
    """frame f relit so that its colour IS its albedo: every batch TEXTURE (its slot kept), every normal (0, 0, -1), ks = 0,
    ka = (0.5, 0.5, 0.5), one light of intensity (2, 2, 2) above the image (z > 0, off the pixel grid).  Diffuse and specular terms
    are exactly 0 (both cosines are clamped negatives), ka * I is exactly 1: colour = clamp(kd) * 255, truncated in S pixels.
    remap: texture slot -> the slot the batch names instead."""
    remap = remap or {}
    batches = []
    for b, t in enumerate(f.tris):
        t2 = t.copy()
        t2["nrm"] = [0.0, 0.0, -1.0]
        slot = int(f._batches[b].tex_id)
        batches.append((abi.SHADER_TEXTURE, remap.get(slot, slot), t2))
    lights = np.float32([[[f.width * 0.31 + 0.37, f.height * 0.27 + 0.21, 300.0], [2.0, 2.0, 2.0]]])
    return abi.Frame(f.width, f.height, tuple(f.c.eye), lights, batches, f.c.flags, ka=(0.5, 0.5, 0.5), ks=(0.0, 0.0, 0.0), p=f.c.p,
                     kh=f.c.kh, kn=f.c.kn)
