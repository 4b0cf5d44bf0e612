"""The texture-set pass's test reference: no arithmetic of its own, a COMPOSITION of tests/texref.py (tests/tex_ref.c).  For each
slot s, texref.forward / texref.grad run on the frame's id plane with the id words of every pixel whose slot is not s set to 0
(nobody), chained through `prefill`, not fused, so that the other slots' words stay.  Pixels that have an owner and no slot (their
batch lies beyond the map, or the map's byte names no slot) take one further pass with their uv set to NaN: "owned, unsampled".
That pass comes first and carries the fused clear.  One texref.Grad per slot (per texture frame where the slot's texture is per
frame).  Pinned on the CPU by tests/test_texset_ref.py; nothing of the product is involved."""
import numpy as np

import texref
from texref import CLAMP, WRAP

NONE = 0xff
TG_SLOTS = 2048  # the capacity of the gradient kernels' table of distinct texels per tile
TILE = 32


def n_tris(f):
    return sum(len(t) for t in f.tris)


def batch_plane(frame, ids):
    """[rows, W] int64: the batch within `frame` (an abi.Frame) of every pixel's owner, -1 where nobody owns the pixel"""
    ids = np.asarray(ids, np.uint32)
    idx = ((ids & np.uint32(0x7fffffff)) - np.uint32(1)).astype(np.int64)  # (0 wraps to 2^32 - 1)
    ends = np.cumsum([len(t) for t in frame.tris])
    own = idx < (ends[-1] if len(ends) else 0)
    return np.where(own, np.searchsorted(ends, np.where(own, idx, 0), side="right"), -1)


def slot_plane(frame, ids, batch_slot, n_slots):
    """[rows, W] int64: the slot of every pixel by the rule of include/srz.h — -1 where nobody owns it, NONE where its owner has no
    slot (s = b < len(batch_slot) ? batch_slot[b] : NONE; s >= n_slots counts as NONE)"""
    b = batch_plane(frame, ids)
    m = np.asarray([NONE if s is None else int(s) for s in batch_slot], np.int64)
    s = np.where((b >= 0) & (b < len(m)), m[np.clip(b, 0, len(m) - 1)], NONE)
    s = np.where(s >= n_slots, NONE, s)
    return np.where(b < 0, -1, s)


def tex_of(t, i):
    return t[i] if t.ndim == 4 else t


def _none_pass(ids, uv, slots):
    """the id plane and the uv of the "owned, unsampled" pass"""
    nan_uv = np.array(uv, np.float32, copy=True)
    nan_uv[:, slots == NONE] = np.nan
    return np.where(slots == NONE, ids, 0).astype(np.uint32), nan_uv


def forward(tmpdir, frame, texs, modes, batch_slot, ids, uv, fused=True, prefill=None):
    """one frame: texs a list of [H, W, C] float32 → [C, rows, W] float32"""
    n, n_ch = n_tris(frame), texs[0].shape[-1]
    ids = np.ascontiguousarray(ids, np.uint32)
    slots = slot_plane(frame, ids, batch_slot, len(texs))
    ids0, uv0 = _none_pass(ids, uv, slots)
    out = texref.forward(tmpdir, texs[0], modes[0], n, ids0, uv0, fused, prefill if prefill is not None else np.zeros((n_ch,) + ids.shape, np.uint32))
    for s, (tex, mode) in enumerate(zip(texs, modes)):
        out = texref.forward(tmpdir, tex, mode, n, np.where(slots == s, ids, 0).astype(np.uint32), uv, False, out.view(np.uint32))
    return out


def grad(tmpdir, frame, texs, modes, batch_slot, ids, uv, gout, into=None, want_uv=True, fused=True, prefill=None):
    """one frame's share: adds into into[s] (a texref.Grad or None per slot; into None: none) → guv [2, rows, W] float32 or None"""
    n = n_tris(frame)
    ids = np.ascontiguousarray(ids, np.uint32)
    slots = slot_plane(frame, ids, batch_slot, len(texs))
    ids0, uv0 = _none_pass(ids, uv, slots)
    pre = prefill if prefill is not None else np.zeros((2,) + ids.shape, np.uint32)
    guv = texref.grad(tmpdir, texs[0], modes[0], n, ids0, uv0, gout, None, want_uv, fused, pre)
    for s, (tex, mode) in enumerate(zip(texs, modes)):
        acc = into[s] if into is not None else None
        guv = texref.grad(tmpdir, tex, mode, n, np.where(slots == s, ids, 0).astype(np.uint32), uv, gout, acc, want_uv, False,
                          guv.view(np.uint32) if want_uv else None)
    return guv


class Grads:
    """one texref.Grad per slot and texture frame: .acc[s] is a list of one Grad (a shared texture) or one per frame"""

    def __init__(self, texs):
        self.acc = [[texref.Grad(t.shape[-3:]) for _ in range(t.shape[0] if t.ndim == 4 else 1)] for t in texs]

    def at(self, i):
        """→ the per-slot Grads frame i adds into"""
        return [a[i] if len(a) > 1 else a[0] for a in self.acc]


def forward_set(tmpdir, frames, v, uvw, texs, modes, batch_slot, fused=True, fill=0):
    """v: the visibility buffer's words [n, 4, rows, W]; uvw: float32 [n, 2, rows, W]; texs: [H, W, C] or [n, H, W, C] each; the
    planes start from the word `fill` → float32 [n, C, rows, W]"""
    out = []
    for i, f in enumerate(frames):
        pre = np.full((texs[0].shape[-1],) + v.shape[2:], fill, np.uint32)
        out.append(forward(tmpdir, f, [tex_of(t, i) for t in texs], modes, batch_slot, v[i, 1], uvw[i], fused, pre))
    return np.stack(out)


def grad_set(tmpdir, frames, v, uvw, gout, texs, modes, batch_slot, fused=True, fill=0):
    """→ (Grads, guv float32 [n, 2, rows, W])"""
    g, gu = Grads(texs), []
    for i, f in enumerate(frames):
        pre = np.full((2,) + v.shape[2:], fill, np.uint32)
        gu.append(grad(tmpdir, f, [tex_of(t, i) for t in texs], modes, batch_slot, v[i, 1], uvw[i], gout[i], g.at(i), True, fused, pre))
    return g, np.stack(gu)


def touched(tmpdir, frame, tex_hw, mode, ids, uv, slots, s, tile):
    """the flat texel indices slot s touches within tile (ty, tx) of the frame, by the reference's own counts"""
    rows, W = ids.shape
    ty, tx = tile
    inside = np.zeros((rows, W), bool)
    inside[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = True
    acc = texref.Grad(tuple(tex_hw) + (1,))
    texref.grad(tmpdir, np.zeros(tuple(tex_hw) + (1,), np.float32), mode, n_tris(frame), np.where(inside & (slots == s), ids, 0).astype(np.uint32),
                uv, np.ones((1, rows, W), np.float32), acc, False)
    return set(np.flatnonzero(acc.count.reshape(-1)).tolist())


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
ZS = texref.ZS


def _split(t, k):
    """triangles dealt round robin into k batches: every batch lies all over the frame, at every depth"""
    from srz import abi
    return [(abi.SHADER_NORMAL, -1, np.ascontiguousarray(t[i::k])) for i in range(k)]


def three_frame(seed=2, **kw):
    """64 x 64, three batches interleaved in depth: the batches alternate within rows"""
    import support
    return support.frame(_split(support.soup(seed, 150, 64, 64, ZS), 3), 64, 64, **kw)


THREE_MAP = (2, 0, 1)


def holes_frame(**kw):
    """the same triangles in five batches, for a map with NONE in it that is also shorter than the batch count"""
    import support
    return support.frame(_split(support.soup(2, 150, 64, 64, ZS), 5), 64, 64, **kw)


HOLES_MAP = (1, 0, None, 2)  # batch 2 has no slot, batch 4 lies beyond the map
HOLES_MAP_200 = (1, 0, 200, 2)  # a byte that names no slot of three


def shared_frame():
    """two batches under two slots of SHARED_TEX texels each, uv by centre_uv: both slots touch the same texel indices in every tile"""
    import support
    return support.frame(_split(support.soup(4, 120, 64, 64, ZS), 2), 64, 64)


SHARED_TEX = (8, 8)  # (tex_w, tex_h), a power of two: (i + 0.5) / 8 is exact


def centre_uv(seed, n, rows, W, tw, th):
    """[n, 2, rows, W] float32: every pixel on the centre of a texel of its own choice, ((i + 0.5) / tw, (j + 0.5) / th) — with sizes
    that are powers of two every weight is 0 or 1 exactly"""
    rng = np.random.default_rng([seed, tw, th])
    return np.stack([(rng.integers(0, tw, (n, rows, W)) + 0.5) / tw, (rng.integers(0, th, (n, rows, W)) + 0.5) / th], 1).astype(np.float32)


def overflow_frame():
    """two batches whose uv run two texels of a 64 x 64 texture per pixel (u = x / 32, v = y / 32): every pixel of a tile touches
    four texels of its own.  The batches are the two halves of the frame along its diagonal, cut into strips so that both classes of
    pixel occur: each slot touches at most 2048 texels of tile (0, 0), the two together more than that.  In CLAMP mode, so that the
    other tiles (uv beyond 1) touch border texels only"""
    import support
    from srz import abi
    strips = [[], []]
    for j in range(8):  # strips of 8 rows; in strip j batch 0 lies left of x = 8 j + 4, batch 1 right of it
        y0, y1, xm = 8.0 * j, 8.0 * j + 8.0, 8.0 * j + 4.0
        for b, (xa, xb) in enumerate(((0.0, xm), (xm, 64.0))):
            for verts in (((xa, y0), (xa, y1), (xb, y0)), ((xb, y0), (xa, y1), (xb, y1))):  # (support.ccw's winding)
                strips[b].append(support.tri(*verts, z=10.0 + j, uv=tuple((x / 32.0, y / 32.0) for x, y in verts)))
    return support.frame([(abi.SHADER_NORMAL, -1, np.concatenate(s)) for s in strips], 64, 64)
