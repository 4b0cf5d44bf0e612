"""The mip passes' test reference (tests/mip_ref.c holds the arithmetic): the pyramid of a float texture (levels, build, fold), the
screen-space derivatives of interpolated attributes, the level rule, the trilinear lookup and its backward with the texel gradients
of every level accumulated in double.  Built and loaded like tests/texref.py's library; nothing of the product is involved.  A
sampled frame's texture is [H, W, C] and its pyramid that of one frame; build and fold also take [F, H, W, C]."""
import ctypes as C

import numpy as np

from support import ref_lib

CLAMP, WRAP = 0, 1
vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
_head = [vp, vp, i32, i32, u32, i32, u32, u32, C.c_size_t, vp, vp, vp, vp]  # tex, mip, W, H, C, mode, L, n_tris, n_px, id, u, v, uvd
SIGNATURES = {"mr_levels": (u32, [i32, i32]),
              "mr_level": (None, [i32, i32, u32, vp, vp, vp]),
              "mr_build": (None, [vp, i32, i32, u32, u32, u32, vp]),
              "mr_fold": (None, [vp, i32, i32, u32, u32, u32, vp]),
              "mr_deriv": (None, [vp, u32, vp, u32, C.c_size_t, vp, i32, vp]),
              "mr_lod": (None, [i32, i32, u32, C.c_size_t, vp, vp, vp]),
              "mr_forward": (None, _head + [i32, vp]),
              "mr_grad": (None, _head + [vp, i32, vp, vp, vp, vp])}


def lib(tmpdir):
    return ref_lib("mip_ref", tmpdir, SIGNATURES)


def levels(tmpdir, w, h):
    return int(lib(tmpdir).mr_levels(w, h))


def level(tmpdir, w, h, l):
    """(w_l, h_l, the build's factor into level l — 0 for level 0)"""
    wl, hl, k = C.c_int(), C.c_int(), C.c_float()
    lib(tmpdir).mr_level(w, h, l, C.byref(wl), C.byref(hl), C.byref(k))
    return wl.value, hl.value, k.value


def sizes(tmpdir, w, h, n_levels):
    return [level(tmpdir, w, h, l)[:2] for l in range(n_levels)]


def _tex(tex):
    tex = np.ascontiguousarray(tex, np.float32)
    assert tex.ndim in (3, 4)
    return tex, (tex.shape[0] if tex.ndim == 4 else 1), tex.shape[-3], tex.shape[-2], tex.shape[-1]


def mip_floats(tmpdir, tex_shape, n_levels):
    F = tex_shape[0] if len(tex_shape) == 4 else 1
    return sum(F * hl * wl * tex_shape[-1] for (wl, hl) in sizes(tmpdir, tex_shape[-2], tex_shape[-3], n_levels)[1:])


def build(tmpdir, tex, n_levels):
    """tex [H, W, C] or [F, H, W, C] float32 → the flat pyramid (levels 1 .. n_levels - 1, level-major) float32"""
    tex, F, H, W, n_ch = _tex(tex)
    mip = np.zeros(mip_floats(tmpdir, tex.shape, n_levels), np.float32)
    lib(tmpdir).mr_build(tex.ctypes.data, W, H, n_ch, F, n_levels, mip.ctypes.data)
    return mip


def views(tmpdir, mip, tex_shape, n_levels):
    """the levels 1 .. n_levels - 1 of a flat pyramid as arrays of level 0's rank"""
    F = tex_shape[0] if len(tex_shape) == 4 else 1
    out, off = [], 0
    for (wl, hl) in sizes(tmpdir, tex_shape[-2], tex_shape[-3], n_levels)[1:]:
        n = F * hl * wl * tex_shape[-1]
        out.append(mip[off:off + n].reshape(((F,) if len(tex_shape) == 4 else ()) + (hl, wl, tex_shape[-1])))
        off += n
    assert off == mip.size
    return out


def frame_mip(tmpdir, mip, tex_shape, n_levels, i):
    """the one-frame pyramid of texture frame i out of the flat pyramid of a [F, H, W, C] texture"""
    if len(tex_shape) == 3:
        return mip
    parts = [v[i].ravel() for v in views(tmpdir, mip, tex_shape, n_levels)]
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, mip.dtype)


def fold(tmpdir, gmip, tex_shape, n_levels, gtex):
    """gmip (flat float32, build's layout) folded into a copy of gtex (float32, tex_shape) → that copy"""
    gmip, out = np.ascontiguousarray(gmip, np.float32), np.array(gtex, np.float32, copy=True, order="C")
    assert out.shape == tuple(tex_shape) and gmip.size == mip_floats(tmpdir, tex_shape, n_levels)
    F = tex_shape[0] if len(tex_shape) == 4 else 1
    lib(tmpdir).mr_fold(gmip.ctypes.data, tex_shape[-2], tex_shape[-3], tex_shape[-1], F, n_levels, out.ctypes.data)
    return out


def deriv(tmpdir, attr, pos, n_tris, ids, fused=True, prefill=None):
    """attr [T, 3, C], pos [T, 9] float32 (T >= n_tris), ids [rows, W] uint32 → [2 C, rows, W] float32"""
    attr, pos, ids = np.ascontiguousarray(attr, np.float32), np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(ids, np.uint32)
    n_ch, (rows, W) = attr.shape[2], ids.shape
    assert attr.shape[0] >= n_tris and pos.shape[0] >= n_tris and pos.shape[1] == 9
    out = np.zeros((2 * n_ch, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    assert out.shape == (2 * n_ch, rows, W)
    lib(tmpdir).mr_deriv(attr.ctypes.data, n_ch, pos.ctypes.data, n_tris, rows * W, ids.ctypes.data, int(fused), out.ctypes.data)
    return out.view(np.float32)


def lod(tmpdir, tex_hw, n_levels, uvd):
    """uvd [4, ...] float32 (ux, uy, vx, vy) → (l0 uint32, f float32) of uvd's trailing shape"""
    uvd = np.ascontiguousarray(uvd, np.float32)
    assert uvd.shape[0] == 4
    l0, f = np.zeros(uvd.shape[1:], np.uint32), np.zeros(uvd.shape[1:], np.float32)
    lib(tmpdir).mr_lod(tex_hw[1], tex_hw[0], n_levels, l0.size, uvd.ctypes.data, l0.ctypes.data, f.ctypes.data)
    return l0, f


def _planes(ids, uv, uvd, n_levels):
    ids, uv = np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(uv, np.float32)
    assert ids.ndim == 2 and uv.shape == (2,) + ids.shape
    if n_levels > 1:
        uvd = np.ascontiguousarray(uvd, np.float32)
        assert uvd.shape == (4,) + ids.shape
    else:
        uvd = None
    return ids, np.ascontiguousarray(uv[0]), np.ascontiguousarray(uv[1]), uvd, ids.shape


def _p(a):
    return a.ctypes.data if a is not None else None


def forward(tmpdir, tex, mip, mode, n_levels, n_tris, ids, uv, uvd, fused=True, prefill=None):
    """tex [H, W, C], mip its flat one-frame pyramid (build's; None with n_levels == 1, like uvd [4, rows, W]) → [C, rows, W] float32"""
    tex, _, H, W_, n_ch = _tex(tex)
    assert tex.ndim == 3
    ids, u, v, uvd, (rows, W) = _planes(ids, uv, uvd, n_levels)
    mip = np.ascontiguousarray(mip, np.float32) if n_levels > 1 else None
    out = np.zeros((n_ch, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    assert out.shape == (n_ch, rows, W)
    lib(tmpdir).mr_forward(tex.ctypes.data, _p(mip), W_, H, n_ch, mode, n_levels, n_tris, rows * W, ids.ctypes.data, u.ctypes.data, v.ctypes.data,
                           _p(uvd), int(fused), out.ctypes.data)
    return out.view(np.float32)


class Grad:
    """the texel gradients of one texture frame over its WHOLE pyramid, accumulated in double over any number of frames: .g and .gabs
    (the sums of |product|) flat float64, level 0 [H, W, C] first, then the levels 1 .. in build's layout; .count per texel"""

    def __init__(self, tmpdir, tex_shape, n_levels):
        assert len(tex_shape) == 3
        self.shape, self.n_levels = tuple(tex_shape), n_levels
        self.sizes = sizes(tmpdir, tex_shape[1], tex_shape[0], n_levels)
        texels = sum(w * h for (w, h) in self.sizes)
        self.g, self.gabs = np.zeros(texels * tex_shape[2], np.float64), np.zeros(texels * tex_shape[2], np.float64)
        self.count = np.zeros(texels, np.uint32)

    def level(self, l):
        """(g, gabs [h_l, w_l, C], count [h_l, w_l]) of level l: views"""
        off = sum(w * h for (w, h) in self.sizes[:l])
        (w, h), n_ch = self.sizes[l], self.shape[2]
        sl = slice(off * n_ch, (off + w * h) * n_ch)
        return self.g[sl].reshape(h, w, n_ch), self.gabs[sl].reshape(h, w, n_ch), self.count[off:off + w * h].reshape(h, w)


def grad(tmpdir, tex, mip, mode, n_levels, n_tris, ids, uv, uvd, gout, into=None, want_uv=True, fused=True, prefill=None):
    """one frame's share: adds into `into` (a Grad, or None) and returns the guv planes [2, rows, W] float32 (None if not wanted)"""
    tex, _, H, W_, n_ch = _tex(tex)
    ids, u, v, uvd, (rows, W) = _planes(ids, uv, uvd, n_levels)
    mip = np.ascontiguousarray(mip, np.float32) if n_levels > 1 and mip is not None else None
    gout = np.ascontiguousarray(gout, np.float32)
    assert gout.shape == (n_ch, rows, W) and (not want_uv or n_levels == 1 or mip is not None)
    guv = None
    if want_uv:
        guv = np.zeros((2, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    lib(tmpdir).mr_grad(tex.ctypes.data, _p(mip), W_, H, n_ch, mode, n_levels, n_tris, rows * W, ids.ctypes.data, u.ctypes.data, v.ctypes.data,
                        _p(uvd), gout.ctypes.data, int(fused), _p(into.g) if into else None, _p(into.gabs) if into else None,
                        _p(into.count) if into else None, _p(guv))
    return guv.view(np.float32) if guv is not None else None


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
ZS = np.float32([1, 2, 3, 4])
# (tex_w, tex_h): six levels stopping at 3 x 2; one extent reaching 1 first; two levels; one level; ...
TEX_SIZES = ((64, 64), (96, 64), (32, 8), (100, 70), (5, 7), (1, 1))
LEVELS = {(1024, 1024): 11, (16384, 16384): 15, (100, 70): 2, (96, 64): 6, (32, 8): 6, (5, 7): 1, (1, 1): 1, (0, 4): 0, (16385, 2): 0, (64, 64): 7}


def backdrop():
    """the triangle behind the soup, as tests/test_gpu_texture.py has it: the whole frame under one magnified owner"""
    import support
    return support.ccw((-8, -8), (400, -8), (-8, 400), z=80.0, uv=((0.1, 0.2), (0.9, 0.3), (0.4, 0.95)))


def soup_frames(w=64, h=64, n=90, k=2, uv_scale=1.0, flags=None):
    """k frames of soup(1, n, w, h) in front of the backdrop; uv_scale scales the soup's uv (not the backdrop's)"""
    import support
    from srz import abi
    t = support.soup(1, n, w, h, ZS, big=w < 40)
    t["uv"] *= np.float32(uv_scale)
    t = np.concatenate([t, backdrop()])
    return [support.frame(t, w, h, flags=abi.FUSED_CLEAR if flags is None else flags) for _ in range(k)]


def make_tex(seed, w, h, n_ch, frames=None):
    shape = (h, w, n_ch) if frames is None else (frames, h, w, n_ch)
    return np.random.default_rng([seed, w, h, n_ch]).normal(0, 3, shape).astype(np.float32)


TG_SLOTS = 2048  # the capacity of k_tex_mip_grad's table of distinct texels per tile and level
TILE = 32


def overflow_planes(w=64, h=64, tw=256, th=256):
    """the planes of k_tex_mip_grad's no-slot case, two frames of w x h: uv steps 2.5 texels of a tw x th texture per pixel, so no two
    pixels of a tile share a corner at level 0; frame 0's uvd gives a footprint of half a texel (l0 = 0, f = 0), frame 1's rho = 1.5
    exactly along both axes (levels 0 and 1) → (uv [2, 2, h, w], uvd [2, 4, h, w]) float32"""
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    uv = np.stack([np.stack([(2.5 * xs + 0.85) / tw, (2.5 * ys + 1.1) / th]).astype(np.float32)] * 2)
    uvd = np.zeros((2, 4, h, w), np.float32)
    uvd[0, 0], uvd[0, 3] = 0.5 / tw, 0.5 / th
    uvd[1, 0], uvd[1, 3] = 1.5 / tw, 1.5 / th
    return uv, uvd


def tile_texels(tmpdir, ids, uv, uvd, tex_hw, mode, n_levels, n_tris):
    """the distinct texels each TILE x TILE tile of one frame adds into, per level, counted from the reference's own accumulators (each
    add names its texel) → int [tiles_y, tiles_x, n_levels]"""
    rows, W = ids.shape
    out = np.zeros(((rows + TILE - 1) // TILE, (W + TILE - 1) // TILE, n_levels), np.int64)
    zero = np.zeros(tuple(tex_hw) + (1,), np.float32)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            sl = (slice(ty * TILE, (ty + 1) * TILE), slice(tx * TILE, (tx + 1) * TILE))
            probe = Grad(tmpdir, zero.shape, n_levels)
            grad(tmpdir, zero, None, mode, n_levels, n_tris, ids[sl], uv[(slice(None),) + sl], uvd[(slice(None),) + sl],
                 np.ones((1,) + ids[sl].shape, np.float32), probe, False)
            out[ty, tx] = [int((probe.level(l)[2] > 0).sum()) for l in range(n_levels)]
    return out
