"""What the tests of the tile walk beyond the grid's cap share (tests/test_gpu_pass_walk.py, tests/test_gpu_pass_walk_lit.py, and on
the CPU tests/test_walk_checkers.py): the two sets that cross tile_grid's cap, the World that makes everything the passes read once,
and the checkers with their stated bounds — `same` for the deterministic planes, `check_sum` for the float-atomic sums, `teeth` for
the condition under which check_sum's bound can see one tile's contribution lost, doubled or misplaced.  A plain module like
tests/support.py: importable without a GPU; torch is imported by the functions that need it."""
import functools

import numpy as np

from srz import abi
from support import SENTINEL, ccw, frame, padded_positions, soup, stream, visibility, words

F = abi.FUSED_CLEAR
CAP = 16384  # tile_grid's cap on the workgroups of a pass
ZS = np.float32([1, 2, 3, 4])
U = 2.0 ** -24
BACK_UV = ((0.1, 0.2), (0.9, 0.3), (0.4, 0.95))
TEX_W, TEX_H = 16, 16
SHAPES = ("many", "large")
CHANNELS = {"many": 5, "large": 2}  # (many: a full register chunk of channels and a tail)
UV_SCALE = {"many": 3.0, "large": 60.0}  # (both reach the levels above 0 of a 16 x 16 texture)
TILE = 32


def many_frames():
    """a soup of five small triangles in front of a triangle that covers the lower right of the frame (the partial column, the
    partial band and the corner tile) and leaves the upper left to the soup and to nobody; soup and shift differ from frame to frame"""
    out = []
    for i in range(6144):
        back = ccw((44, 41), (-16, 41), (44, -19), z=80.0, uv=BACK_UV)
        back["pos"][:, :, :2] += np.float32([i % 7 - 3, i // 7 % 5 - 2])
        out.append(frame(np.concatenate([soup(i, 5, 36, 33, ZS), back]), 36, 33, flags=0))
    return out


def large_frames():
    """a soup of ten triangles some hundred pixels across in front of a triangle that covers the frame but its upper left corner"""
    out = []
    for i in range(7):
        t = soup(i, 10, 98, 98, ZS, big=True)
        t["pos"][:, :, :2] *= np.float32(16)
        back = ccw((1576, 1576), (-424 + 16 * i, 1576), (1576, -424 - 16 * i), z=80.0, uv=BACK_UV)
        out.append(frame(np.concatenate([t, back]), 1568, 1568, flags=0))
    return out


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


class World:
    """one shape's set with everything the passes read, each thing made once on first use"""

    def __init__(self, ctx, name):
        self.ctx, self.name, self.C = ctx, name, CHANNELS[name]
        self.frames = many_frames() if name == "many" else large_frames()
        self.n = len(self.frames)
        self.fs = ctx.frameset(self.frames)
        w, h = self.fs.width, self.fs.height
        tiles = self.n * ((w + 31) // 32) * ((h + 31) // 32)
        assert tiles > CAP and (name != "many" or tiles >= 1.25 * CAP), tiles
        self.vis = visibility(self.fs)
        self.v = words(self.vis)
        self.n_tris = [f.n_tris for f in self.frames]
        self.T = max(self.n_tris)
        self.own = ((self.v[:, 1] & np.uint32(0x7fffffff)) - np.uint32(1)) < np.uint32(self.n_tris)[:, None, None]
        # owners and nobody's pixels exist in (nearly) every frame; many: in each of the four kinds of tile
        per = lambda m: m.reshape(self.n, -1).any(1)  # noqa: E731
        parts = [self.own, ~self.own]
        if name == "many":
            parts += [self.own[:, :32, :32], self.own[:, :32, 32:], self.own[:, 32:, :32], self.own[:, 32:, 32:]]
        assert all(per(m).mean() >= 0.9 for m in parts), [per(m).mean() for m in parts]
        some = range(0, self.n, max(1, self.n // 64))
        assert len({self.v[i, 1].tobytes() for i in some}) >= 0.9 * len(some)  # the frames differ (a culled soup leaves the shift alone)

    def rng(self, salt):
        return np.random.default_rng([salt, self.n])

    def shape(self, n_ch):
        return self.fs.interpolate_shape(n_ch)

    @functools.cached_property
    def pos(self):
        return padded_positions(self.frames, self.T)

    @functools.cached_property
    def attr(self):
        return self.rng(1).normal(0, 3, (self.n, self.T, 3, self.C)).astype(np.float32)

    @functools.cached_property
    def gout(self):
        """[n, C, rows, W] float32, NaN at nobody's pixels (their words may hold anything), and its copy on the device"""
        g = self.rng(2).normal(0, 2, self.shape(self.C)).astype(np.float32)
        g[np.broadcast_to(~self.own[:, None], g.shape)] = np.nan
        return g, dev(g)

    @functools.cached_property
    def planes(self):
        """antialias's input planes [n, C, rows, W] float32 and their copy on the device"""
        c = self.rng(3).normal(0, 1, self.shape(self.C)).astype(np.float32)
        return c, dev(c)

    @functools.cached_property
    def uv(self):
        """the GPU's interpolate and interpolate_deriv of the frames' own uv, scaled → (uv [n, 2, rows, W], uvd [n, 4, rows, W]) on
        the device and as float32 arrays"""
        import texref
        import torch
        a = np.zeros((self.n, self.T, 3, 2), np.float32)
        for i, f in enumerate(self.frames):
            a[i, :f.n_tris] = texref.frame_uv(f) * np.float32(UV_SCALE[self.name])
        a_dev, fs = dev(a), self.fs
        uv, uvd = torch.zeros(self.shape(2), dtype=torch.float32, device="cuda"), torch.zeros(self.shape(4), dtype=torch.float32, device="cuda")
        fs.interpolate(self.vis.data_ptr(), a_dev.data_ptr(), 2, self.n, self.T, uv.data_ptr(), fs.interpolate_bytes(2), F, stream())
        fs.interpolate_deriv(self.vis.data_ptr(), a_dev.data_ptr(), 2, self.n, self.T, uvd.data_ptr(), fs.interpolate_bytes(4), F, stream())
        torch.cuda.synchronize()
        return uv, uvd, uv.cpu().numpy(), uvd.cpu().numpy()

    @functools.cached_property
    def tex(self):
        """one texture for every frame [h, w, C], its copy on the device, the level count and the GPU's pyramid"""
        import srz
        import texref
        import torch
        t = texref.make_tex(3, TEX_W, TEX_H, self.C)
        L = srz.mip_levels(TEX_W, TEX_H)
        nbytes = srz.mip_bytes(TEX_W, TEX_H, self.C, 1, L)
        t_dev, mip = dev(t), torch.zeros((nbytes // 4,), dtype=torch.float32, device="cuda")
        self.ctx.mip_build(t_dev.data_ptr(), TEX_W, TEX_H, self.C, 1, L, mip.data_ptr(), nbytes, stream())
        torch.cuda.synchronize()
        assert L > 1
        return t, t_dev, L, mip

    # ---- for the inputs of the newer passes (tests/test_gpu_pass_walk_lit.py makes them, each once per world)
    def memo(self, key, make):
        """make(self), made on first use and kept under `key`"""
        if key not in self.__dict__.setdefault("_memo", {}):
            self._memo[key] = make(self)
        return self._memo[key]

    def nobody_nan(self, a):
        """a [n, k, rows, W] float32 with NaN written over nobody's pixels (their words may hold anything) → (a, its copy on the device)"""
        a = np.ascontiguousarray(a, np.float32)
        a[np.broadcast_to(~self.own[:, None], a.shape)] = np.nan
        return a, dev(a)

    def seeded(self, salt, n_ch, scale=1.0):
        """[n, n_ch, rows, W] float32 normal values, NaN at nobody's pixels, and its copy on the device"""
        return self.nobody_nan((self.rng(salt).normal(0, 1, self.shape(n_ch)) * scale).astype(np.float32))

    def interpolated(self, a, deriv=False):
        """the GPU's own interpolate (deriv: interpolate_deriv) of the attributes a [n, T, 3, k], NaN written over nobody's pixels →
        (the planes as float32, their copy on the device)"""
        import torch
        k, fs = a.shape[-1], self.fs
        planes = 2 * k if deriv else k
        a_dev, out = dev(a), torch.zeros(self.shape(planes), dtype=torch.float32, device="cuda")
        (fs.interpolate_deriv if deriv else fs.interpolate)(self.vis.data_ptr(), a_dev.data_ptr(), k, self.n, self.T, out.data_ptr(),
                                                           fs.interpolate_bytes(planes), F, stream())
        torch.cuda.synchronize()
        return self.nobody_nan(out.cpu().numpy())

    @functools.cached_property
    def tile_of(self):
        """[n, rows, W] int64: the set-wide tile index of every pixel"""
        return tile_index(self.n, *self.v.shape[2:])

    def tiles(self):
        """tile_boxes of the set — large: every 7th tile and all tiles of frame 6 (the frame of the walk's second trip), which keeps
        the per-tile pass of the reference short; what is stated about tiles is then stated about that sample"""
        return tile_boxes(self.n, *self.v.shape[2:], sample=None if self.name == "many" else (7, self.n - 1))


def make_worlds(ctx):
    """the body of a module's `worlds` fixture: yields get(name) → the World, made on first use; closes their sets afterwards"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = World(ctx, name)
        return made[name]
    yield get
    for w in made.values():
        w.fs.close()


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def check_sum(got, ref, mag, cnt, what):
    """a float-atomic sum against the reference's double: ref the sums, mag the sums of |term|, cnt the terms per element"""
    got, cnt = got.reshape(ref.shape), np.broadcast_to(cnt, ref.shape).astype(np.float64)
    assert np.isfinite(ref).all() and (cnt > 1).any(), what
    nu = cnt * U
    assert nu.max() < 1.0, (what, cnt.max())  # (the bound's domain)
    bound = nu / (1.0 - nu) * mag
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{what}: max err {err.max():.3e}, max err / bound {np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0:.3f}, "
          f"max n {int(cnt.max())}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    one = cnt == 1
    same((got + np.float32(0))[one], (ref.astype(np.float32) + np.float32(0))[one], what + " (n = 1)")
    assert (got[cnt == 0] == 0).all(), what


def check_nobody(w, got, fused, what):
    """nobody's words: zeros with the fused clear, else the sentinel the buffer started from"""
    nobody = np.broadcast_to(~w.own[:len(got), None], got.shape)
    assert (got[nobody] == (0 if fused else SENTINEL)).all() and (got[~nobody] != SENTINEL).any(), what


def pre(w, n_planes):
    return np.full((n_planes,) + w.v.shape[2:], SENTINEL, np.uint32)


# ------------------------------------------------------------------------------------------------------ teeth
class Shares:
    """per element of a summed output, the smallest non-zero sum |term| that one tile adds into it.  add(tile_mag): the sums of
    |term| of one tile's pixels alone, an array of the output's shape (or of the part `at` indexes)"""

    def __init__(self, shape):
        self.least = np.full(shape, np.inf)
        self.tiles = np.zeros(shape, np.int64)

    def add(self, tile_mag, at=...):
        m = np.asarray(tile_mag, np.float64)
        hit = m > 0
        self.least[at] = np.where(hit, np.minimum(self.least[at], m), self.least[at])
        self.tiles[at] += hit


def teeth(shares, mag, cnt, what, require=True, single=True):
    """the condition under which check_sum's bound sees a tile: gamma_n(e) <= share_min(e) / 4 on at least 90 % of the touched
    elements e, share_min(e) = the smallest non-zero per-tile sum |term| into e over the whole sum |term| of e — from the reference
    alone.  Prints the 90th percentile of gamma_n / share_min; asserts (require) that it is at most 1 / 4, and (single too) that the
    output has elements of one term and of several.  → the elements that have teeth"""
    cnt = np.broadcast_to(cnt, mag.shape).astype(np.float64)
    touched = (cnt > 0) & (mag > 0) & np.isfinite(shares.least)
    assert touched.any(), what
    nu = cnt * U
    assert nu.max() < 1.0, (what, cnt.max())
    ratio = np.full(mag.shape, np.inf)
    ratio[touched] = (nu[touched] / (1.0 - nu[touched])) / (shares.least[touched] / mag[touched])
    p90 = float(np.quantile(ratio[touched], 0.9))
    print(f"{what}: teeth: 90th percentile of gamma_n / share_min {p90:.3e} over {int(touched.sum())} touched elements, "
          f"n = 1 in {int((cnt == 1).sum())}, n > 1 in {int((cnt > 1).sum())}, most tiles into one element {int(shares.tiles.max())}")
    if require:
        assert p90 <= 0.25, (what, p90)
        assert not single or ((cnt == 1).any() and (cnt > 1).any()), what
    return touched & (ratio <= 0.25)


def check_bound(got, ref, mag, cnt, what, extra=0):
    """a sum reduced in any tree against the reference's double, by the reference's own Grad.bound(extra): gamma_(n + extra) *
    sum |term|; bit for bit where n = 1, exactly 0 where n = 0.  Prints max err / bound → that ratio"""
    got, cnt = got.reshape(ref.shape), np.broadcast_to(cnt, ref.shape).astype(np.float64)
    assert np.isfinite(ref).all(), what
    nu = (cnt + extra) * U
    assert nu.max() < 1.0, (what, cnt.max())  # (the bound's domain)
    bound = nu / (1.0 - nu) * mag
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    print(f"{what}: max err {err.max():.3e}, max err / bound {ratio:.3f}, max n {int(cnt.max())}, untouched {int((cnt == 0).sum())}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} entries beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    one = cnt == 1
    same((got + np.float32(0))[one], (ref.astype(np.float32) + np.float32(0))[one], what + " (n = 1)")
    assert (got[cnt == 0] == 0).all(), what
    return ratio


def check_gpar(got, accs, what, extra=0):
    """light_grad's / microfacet_grad's d_gpar rows against one Grad per row (tests/lightref.py, tests/microfacetref.py), with the
    extra their own tests use"""
    return check_bound(got, np.stack([a.gsum for a in accs]), np.stack([a.gabs for a in accs]), np.stack([a.count for a in accs]), what, extra)


def check_gtab(got, acc, what, extra=1):
    """ibl_grad's d_gtab against iblref.TabGrad, with the extra its own test uses: the add into the caller's word"""
    return check_bound(got, acc.gsum, acc.gabs, acc.count, what, extra)


# ------------------------------------------------------------------------------------------------------ tiles, and dealing inputs to them
def tile_boxes(n, rows, W, sample=None):
    """(set-wide tile index, frame, row slice, column slice) of the tiles of n frames of rows x W, frame-major, then tile rows, then
    tile columns — the order of the walk.  sample = (k, frame): every k-th tile and all tiles of that frame only"""
    tx, ty = (W + TILE - 1) // TILE, (rows + TILE - 1) // TILE
    for f in range(n):
        for j in range(ty):
            for i in range(tx):
                t = (f * ty + j) * tx + i
                if sample is None or t % sample[0] == 0 or f == sample[1]:
                    yield t, f, slice(j * TILE, min(rows, (j + 1) * TILE)), slice(i * TILE, min(W, (i + 1) * TILE))


def tile_index(n, rows, W):
    """[n, rows, W] int64: every pixel's set-wide tile index (tile_boxes' order)"""
    tx, ty = (W + TILE - 1) // TILE, (rows + TILE - 1) // TILE
    t = (np.arange(rows)[:, None] // TILE) * tx + np.arange(W)[None, :] // TILE
    return np.arange(n)[:, None, None] * (tx * ty) + t[None]


def mix(a):
    """a 32-bit hash of non-negative integers (the finaliser of MurmurHash3), elementwise"""
    h = np.asarray(a, np.uint64) & np.uint64(0xffffffff)
    for shift, mul in ((16, 0x85ebca6b), (13, 0xc2b2ae35), (16, 1)):
        h ^= h >> np.uint64(shift)
        h = (h * np.uint64(mul)) & np.uint64(0xffffffff)
    return h


IBL_DUMP = -1  # deal_ibl's cell of a tile whose pixels go on and beyond the upper clamps


def deal_ibl(counts, t, salt=0):
    """the cell (cx along nv, cy along the roughness) of an ibl table of side t that each tile's pixels land in, so that gtab's bound
    can see a tile: a table word then collects from a handful of tiles of one size class only.  counts [tiles]: the owned pixels of
    every tile.  A word's n is the pixels of its (up to) four cells, 4 k P for k tiles of at most P pixels a cell, and a tile's share of
    its sum |term| about 1 / (16 k) or more; gamma_n <= share / 4 then asks k^2 <= 2^24 / (256 P) — less a margin for the spread of the
    weights and of |gout|: k = sqrt(45875 / P) / 1.6, 4 tiles a cell at P = 1024.  The classes (P = 4, 16, .. 1024) take bands of cell
    rows, the largest class first, an empty row between two bands (no word mixes two classes); row 0 is left to the single pixels of
    ibl_coords, row 1 empty; within a band the tiles are dealt in the order of hash(tile) to cell rank mod cells.  Every sixteenth tile
    in that order, the tiles that no band has room for and the cell of the last row and column go to IBL_DUMP.  → (cx [tiles], cy [tiles])"""
    counts = np.asarray(counts, np.int64)
    h = mix(np.arange(len(counts)) * 2 + 1 + (salt << 20))
    cx, cy = np.full(len(counts), IBL_DUMP, np.int64), np.full(len(counts), IBL_DUMP, np.int64)
    cls = np.where(counts > 0, np.ceil(np.log2(np.maximum(counts, 1)) / 2).astype(np.int64), -1)  # P = 4^cls: 1 .. 4 → 1, 5 .. 16 → 2, ...
    cls = np.maximum(cls, np.where(counts > 0, 1, -1))
    rank = np.empty(len(counts), np.int64)
    rank[np.argsort(h, kind="stable")] = np.arange(len(counts))
    live = (counts > 0) & (rank % 16 != 15)
    row, side = 2, t - 1
    for c in sorted(set(cls[live].tolist()), reverse=True):
        members = np.flatnonzero(live & (cls == c))
        k = max(1, int(np.sqrt(45875.0 / 4 ** c) / 1.6))
        rows = min(-(-len(members) // (k * side)), side - row)
        if rows <= 0:
            break
        cells = [(x, y) for x in range(row, row + rows) for y in range(side) if (x, y) != (side - 1, side - 1)]
        members = members[np.argsort(h[members], kind="stable")][:k * len(cells)]
        at = np.arange(len(members)) % len(cells)
        cx[members], cy[members] = np.array(cells)[at, 0], np.array(cells)[at, 1]
        row += rows + 1
    return cx, cy


def ibl_coords(tile_of, own, cx, cy, t, rng):
    """(nv [n, 1, rows, W], roughness [n, rows, W]) float32 from deal_ibl's cells: a live tile's pixels lie in its cell with a jitter of
    their own in (0.05, 0.95) of it, so the interpolation weights vary; a dumped tile's lie on and beyond the upper clamps, 1 exactly or
    in [1.03, 1.2], both coordinates on their own.  The first owned pixels of three live tiles go to cells (0, 0), (0, 2) and (0, 4)
    (as far as the table has them): words of a single term.  tile_of [n, rows, W]: the pixels' tile; own: the owned pixels"""
    import iblref
    shape = tile_of.shape
    px, py = cx[tile_of].astype(np.float64), cy[tile_of].astype(np.float64)
    dump = px < 0

    def beyond():
        return np.where(rng.random(shape) < 0.5, 1.0, rng.uniform(1.03, 1.2, shape))
    singles = [y for y in (0, 2, 4) if y + 1 < t - 1 or y == 0]
    flat_own = np.flatnonzero((own & ~dump).ravel())
    picks = flat_own[np.linspace(0, len(flat_own) - 1, len(singles) + 2).astype(np.int64)[1:-1]] if len(flat_own) > len(singles) + 2 else []
    for y, at in zip(singles, picks):
        px.ravel()[at], py.ravel()[at] = 0, y
    nv = np.where(dump, beyond(), (px + rng.uniform(0.05, 0.95, shape)) / (t - 1))
    r = np.where(dump, beyond(), iblref.RMIN + iblref.RSPAN * (py + rng.uniform(0.05, 0.95, shape)) / (t - 1))
    return np.ascontiguousarray(nv[:, None], np.float32), np.ascontiguousarray(r, np.float32)


def deal_one_each(n_tiles, n_cells, salt=0):
    """a cell of its own for every tile, where there are more cells than tiles: the tiles in the order of hash(tile) take the cells in
    the order of hash(cell) → the cell of each tile [n_tiles].  A texel between four cells then collects from four tiles at most"""
    assert n_cells >= n_tiles, (n_cells, n_tiles)
    rank = np.empty(n_tiles, np.int64)
    rank[np.argsort(mix(np.arange(n_tiles) * 2 + 1 + (salt << 20)), kind="stable")] = np.arange(n_tiles)
    return np.argsort(mix(np.arange(n_cells) * 2 + (salt << 21)), kind="stable")[rank]


def cube_dirs(tile_of, n_tiles, N, rng, salt=0):
    """direction planes [n, 3, rows, W] float32 for a cube of N x N faces, dealt per tile: every tile's directions lie between the four
    texel centres (x, y) .. (x + 1, y + 1) of one face, x and y from 1 on (row and column 0 stay free for what a test places by hand),
    with a jitter of their own in (0.05, 0.95) of the cell and any length in (0.5, 2).  → (dirs, face [tiles], x [tiles], y [tiles])"""
    import cuberef
    side = N - 2
    cell = deal_one_each(n_tiles, 6 * side * side, salt)
    face, x, y = cell // (side * side), 1 + cell % (side * side) // side, 1 + cell % side
    shape = tile_of.shape
    s = ((x[tile_of] + rng.uniform(0.05, 0.95, shape) + 0.5) / N) * 2 - 1
    t = ((y[tile_of] + rng.uniform(0.05, 0.95, shape) + 0.5) / N) * 2 - 1
    axes = np.float64(cuberef.AXES)[face[tile_of]]  # [n, rows, W, 3 (n, su, sv), 3]
    d = (axes[..., 0, :] + s[..., None] * axes[..., 1, :] + t[..., None] * axes[..., 2, :]) * rng.uniform(0.5, 2.0, shape)[..., None]
    return np.ascontiguousarray(np.moveaxis(d, -1, 1), np.float32), face, x, y


def shadow_coords(tile_of, n_tiles, m, sd, rng, salt=0):
    """coordinate planes [n, 3, rows, W] float32 for an m x m map, dealt per tile: every tile's sx, sy lie between the four texels
    (x, y) .. (x + 1, y + 1), x below m - 4 (the last columns stay free for what a test places by hand), with a jitter of their own in
    (0.05, 0.95); sd [n, rows, W] as given"""
    cell = deal_one_each(n_tiles, (m - 4) * (m - 1), salt)
    x, y = cell // (m - 1), cell % (m - 1)
    shape = tile_of.shape
    return np.ascontiguousarray(np.stack([x[tile_of] + rng.uniform(0.05, 0.95, shape), y[tile_of] + rng.uniform(0.05, 0.95, shape), sd], 1), np.float32)
