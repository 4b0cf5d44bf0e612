"""Depth peeling's test reference (srz_frameset_peel_visibility), built on the unchanged CPU oracle through visref.Reference: layer
k + 1 of a frame is, per pixel, what the oracle renders when that pixel's owners in layers 1..k are not drawn.

Layer 1 is visref's expected buffer of the frame.  For layer k + 1 the pixels are grouped by their set of previous owners; for every
distinct set the oracle renders the frame without those triangles (the batches keep their places, the remaining triangles their
order and the flat normals the full frame's Reference gave them — a subset of normals that are SEP levels apart stays so) and
visref decodes it; the ids are mapped back to the original indices and the results stitched per pixel.  A pixel visref leaves
ambiguous in some layer is LEFT OUT from that layer on (`keep` is False there).  Nothing here restates the visibility rule; the
one restatement, next_after(), is what the hostile-input test compares with, on fragments this reference found."""
import types

import numpy as np

import visref
from srz import abi
from support import frame, soup, stack

Z_INF = 0x7f800000
MAX_LEFT_OUT = 0.02  # of a layer's owned + left-out pixels
ZS = np.float32([1.0, 2.0, 2.0, 3.0, 0.5])  # (the soups' depths: ties between triangles, as tests/test_gpu_visibility.py)

# every scene the GPU tests peel: name -> frame.  The soups' seeds (odd: quarter-pixel vertices; 3 | seed: one depth per triangle)
# were chosen on the CPU so that the reference alone meets the conditions tests/test_peel_ref.py asserts
SCENES = {
    "stack12": lambda: stack(12),
    "stack40": lambda: stack(40),
    "stack150": lambda: stack(150),
    "soup96x80": lambda: frame(soup(SOUP_SEED_A, SOUP_N, 96, 80, ZS, big=True), 96, 80),
    "soup70x45": lambda: frame(soup(SOUP_SEED_B, SOUP_N, 70, 45, ZS, big=True), 70, 45),
    "soup96x80-unified": lambda: frame(soup(SOUP_SEED_A, SOUP_N, 96, 80, ZS, big=True), 96, 80, flags=abi.FUSED_CLEAR | abi.UNIFIED),
}
SOUP_SEED_A, SOUP_SEED_B, SOUP_N = 3, 2, 150
CLASS_SCENES = ("stack150", "soup96x80", "soup70x45")  # held to >= MIN_CLASS owned pixels of each class in layers 1 and 2 (the small stacks own fewer pixels than that; the unified soup has one class)


class _Without(visref.Reference):
    """base's frame without the triangles where keep is False: base's normals, boxes and positions, the batches in place"""

    def __init__(self, base, keep):  # (no Reference.__init__: nothing is assigned anew)
        self.W, self.H, self.L, self.unified = base.W, base.H, base.L, base.unified
        self.index = np.flatnonzero(keep)
        n = len(self.index)
        self.pos = np.ascontiguousarray(base.pos[self.index])
        self.box = np.ascontiguousarray(base.box[self.index]) if n else np.zeros((1, 4), np.int32)
        self.tlev = np.ascontiguousarray(base.tlev[self.index]) if n else np.zeros((1, 3))
        f, batches, k = base.orc_frame, [], 0
        for b, t in enumerate(f.tris):
            batches.append((abi.SHADER_NORMAL, -1, t[keep[k:k + len(t)]]))
            k += len(t)
        self.sizes = [len(t) for _, _, t in batches]
        kw = dict(ka=tuple(f.c.ka), ks=tuple(f.c.ks), p=f.c.p, kh=f.c.kh, kn=f.c.kn)
        self.orc_frame = abi.Frame(self.W, self.H, tuple(f.c.eye), f.lights.view(np.float32).reshape(-1, 2, 3), batches, f.c.flags, **kw)


def _expected(ref, orc):
    """visref's words of ref's frame, the pixels it owns, and the pixels the oracle drew but visref names no owner for"""
    words, out, amb, _, own = ref.expected(orc)
    drawn = ~((out[0] == np.inf) & (out[1] == 0) & (out[2] == 0) & (out[3] == 0))
    ambiguous = drawn & ~own
    assert int(ambiguous.sum()) == amb, (int(ambiguous.sum()), amb)
    return words, own, ambiguous


def nobody(H, W):
    w = np.zeros((4, H, W), np.uint32)
    w[0] = Z_INF
    return w


def owner_of(words):
    """[H, W] int64: the owner's index in the frame, -1 = nobody"""
    return (words[1] & 0x7fffffff).astype(np.int64) - 1


def peel(tmp_path, orc, f, max_layers=None):
    """the frame's layers, nearest first, until one is all nobody (that one included) or max_layers are made -> a namespace: layers,
    a list of namespaces (words [4, H, W] uint32, keep [H, W]: the pixels the reference vouches for in that layer, own: the kept
    pixels somebody owns); left, the pixels left out in the end; n, the triangle count; base, the frame's visref.Reference (the GPU
    renders base.gpu_frame); complete: the last layer is all nobody"""
    base = visref.Reference(tmp_path, f)
    n, H, W = len(base.pos), base.H, base.W
    words, own, amb = _expected(base, orc)
    left = amb.copy()
    layers, owners = [], []

    def push(words, own):
        own = own & ~left
        layers.append(types.SimpleNamespace(words=words, keep=~left, own=own))
        owners.append(np.where(own, owner_of(words), -1))

    push(words, own)
    while layers[-1].own.any() and (max_layers is None or len(layers) < max_layers):
        live = layers[-1].own  # (a pixel without an owner in layer k has ended; a left-out one is not followed)
        prev = np.sort(np.stack([o[live] for o in owners], 1), 1)  # [pixels, k]: each pixel's set of previous owners
        sets, which = np.unique(prev, axis=0, return_inverse=True)
        which = which.reshape(-1)
        ys, xs = np.nonzero(live)
        words = nobody(H, W)
        own = np.zeros((H, W), bool)
        for g, s in enumerate(sets):
            keep = np.ones(n, bool)
            keep[s] = False
            sub = _Without(base, keep)
            w, o, a = _expected(sub, orc)
            back = np.concatenate([[0], sub.index + 1]).astype(np.uint32)  # id word's index part: sub frame -> this frame
            w[1] = back[w[1] & 0x7fffffff] | (w[1] & 0x80000000)
            py, px = ys[which == g], xs[which == g]
            words[:, py, px] = w[:, py, px]
            own[py, px] = o[py, px]
            left[py, px] |= a[py, px]
        push(words, own)
    return types.SimpleNamespace(layers=layers, left=left, n=n, base=base, complete=not layers[-1].own.any())


def fragments_at(tmp_path, orc, base, mask):
    """[H, W] int: how many triangles the oracle draws at each pixel of `mask` when it draws them one at a time"""
    count = np.zeros((base.H, base.W), np.int64)
    ys, xs = np.nonzero(mask)
    for t in range(len(base.pos)):
        x0, y0, x1, y1 = (int(v) for v in base.box[t])
        if not ((xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)).any():
            continue
        keep = np.zeros(len(base.pos), bool)
        keep[t] = True
        _, own, amb = _expected(_Without(base, keep), orc)
        count += (own | amb) & mask
    return count


_cache = {}


def reference(tmp_path, orc, name):
    """peel() of SCENES[name] until empty, made once per session"""
    if name not in _cache:
        _cache[name] = peel(tmp_path, orc, SCENES[name]())
    return _cache[name]


def tie_break(idx, s_class):
    """the place of a fragment among those of one depth at its pixel: S fragments first, the later the earlier; then V fragments, the
    earlier the earlier (uint32 arrays)"""
    idx = np.asarray(idx, np.uint32)
    return np.where(s_class, np.uint32(0x7ffffffe) - idx, np.uint32(0x80000000) | idx).astype(np.uint32)


def next_after(ref, prev, n_tris):
    """THE RULE of include/srz.h restated in numpy on the fragments the reference found (ref.layers; their order is not used): the
    words the peel of `prev` ([4, H, W] uint32, any words at all) must give -> (words, keep)"""
    zp, idp = prev[0].view(np.float32), prev[1]
    wp = (idp & 0x7fffffff) - np.uint32(1)
    ended = (idp == 0) | (wp >= np.uint32(n_tris)) | np.isnan(zp)
    tp = tie_break(wp, (idp >> 31) != 0)
    H, W = zp.shape
    out = nobody(H, W)
    bz, bt = np.full((H, W), np.inf, np.float32), np.full((H, W), 0xffffffff, np.uint32)
    keep = ~ref.left
    with np.errstate(invalid="ignore"):
        for lay in ref.layers:
            z, idw = lay.words[0].view(np.float32), lay.words[1]
            tb = tie_break((idw & 0x7fffffff) - np.uint32(1), (idw >> 31) != 0)
            after = (z > zp) | ((z == zp) & (tb > tp))
            before = (z < bz) | ((z == bz) & (tb < bt))
            take = lay.own & ~ended & after & before
            bz, bt = np.where(take, z, bz), np.where(take, tb, bt)
            out = np.where(take[None], lay.words, out)
    return out, keep
