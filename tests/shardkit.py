"""What the tests of the passes over a visibility buffer on band shards share (tests/test_gpu_pass_shards.py,
tests/test_gpu_pass_shards_lit.py, and on the CPU tests/test_shard_kit.py): the two frame sizes and the three shard layouts on which a
rank's local band `lb` is not band `lb * world + rank`, the Shard that scatters whole-frame planes into a rank's rows and gathers them
back, the Geo that makes a geometry's set, its unsharded render and its ten shards once, and the checkers — check_planes for the
per-pixel outputs (the owned rows are the whole frame's rows word for word, every padding word keeps what it held), masked for the
reference of a rank's part of a summed output, check_rank_sum for the ranks' parts together.  A plain module like tests/walkkit.py:
importable without a GPU; torch and srz are imported by the functions that need them."""
import functools

import numpy as np

from srz import parallel
from support import SENTINEL, ccw, frame, padded_positions, soup, visibility, words
from walkkit import U, Shares, check_bound, dev, same, teeth

BAND = parallel.BAND
H = 197  # 7 bands, the last one 5 rows
GEOMETRIES = {"w72": (72, H), "w70": (70, H)}  # w72: 16-byte quads, a last tile column 8 wide; w70: W % 4 == 2, scalar accesses, 6 wide
LAYOUTS = ((3, (0, 1, 2)), (5, (0, 1, 2, 3, 4)), (8, (6, 7)))  # (world, the ranks run); world 8: the other six repeat worlds 3 and 5
SUM_WORLDS = (3, 5)  # the worlds whose ranks' parts are summed against the whole frame's reference
ZS = np.float32([1, 2, 3, 4])
N_FRAMES = 2
ACC_FILL = 3.25  # what a float-atomic output holds before the call on the rank without a band


def bands_of(height, rank, world):
    return tuple(b for (_, b, _, _) in parallel.band_rows(height, rank, world))


def check_layouts(height=H):
    """the facts about the three layouts that the shard tests rely on, from srz.parallel's formulas; a change of THE BAND MAP that loses
    them fails here, before any GPU work"""
    assert (height + BAND - 1) // BAND == 7 and height - 6 * BAND == 5
    assert parallel.band_rot(3) == 5 and parallel.band_rot(5) == 1 and parallel.band_rot(8) == 5
    own = {(w, r): bands_of(height, r, w) for w, ranks in LAYOUTS for r in range(w)}
    assert own[3, 0] == (0, 4) and own[3, 1] == (1, 5, 6) and own[3, 2] == (2, 3)  # rank 1: the ragged band at lb 2
    assert parallel.shard_layout(height, 0, 3)["bands_per_rank"] == 3  # ranks 0 and 2 are one local band short of it
    assert own[5, 1] == (1, 5) and own[5, 2] == (2, 6)  # rank 2: the ragged band at lb 1
    assert own[5, 0] == (0,) and own[5, 3] == (3,) and own[5, 4] == (4,)  # one band of two
    assert parallel.shard_layout(height, 0, 5)["bands_per_rank"] == 2
    assert own[8, 6] == (6,) and own[8, 7] == ()  # the 5-row band alone; a rank without any band
    for w, _ in LAYOUTS:  # the ranks' bands partition the frame's
        assert sorted(b for r in range(w) for b in own[w, r]) == list(range(7))
    # a local band >= 1 that is not band lb * world + rank exists in worlds 3 and 5: the rotation is exercised
    for w in SUM_WORLDS:
        assert any(b != lb * w + r for r in range(w) for (lb, b, _, _) in parallel.band_rows(height, r, w) if lb >= 1), w
    return own


def rotated_rows(height, rank, world):
    """the owned rows of (rank, world) at local bands >= 1 whose band is not lb * world + rank"""
    return sum(r1 - r0 for (lb, b, r0, r1) in parallel.band_rows(height, rank, world) if lb >= 1 and b != lb * world + rank)


class Shard:
    """one (world, rank) of a frame height: where its rows are.  open() adds its srz.Context(0, rank, world), its frameset and its own
    visibility render; world 1 is the unsharded frame (ctx given: the module's own)."""

    def __init__(self, world, rank, height=H):
        self.world, self.rank, self.height = world, rank, height
        self.rows = parallel.band_rows(height, rank, world)
        self.local_rows = parallel.shard_layout(height, rank, world)["local_rows"]
        # frame_rows[i]: the frame row of the i-th owned row in local order; local_at[i]: its local row
        if world == 1:
            self.frame_rows = self.local_at = np.arange(height)
        else:
            self.frame_rows = np.concatenate([np.arange(r0, r1) for (_, _, r0, r1) in self.rows] + [np.zeros(0, np.int64)]).astype(np.int64)
            self.local_at = np.concatenate([lb * BAND + np.arange(r1 - r0) for (lb, _, r0, r1) in self.rows] + [np.zeros(0, np.int64)]).astype(np.int64)
        self.is_pad = np.ones(self.local_rows, bool)
        self.is_pad[self.local_at] = False
        self.mine = np.zeros(height, bool)  # the frame's rows this rank owns
        self.mine[self.frame_rows] = True
        self.late = self.local_at >= BAND  # the owned rows at lb >= 1
        self.ctx = self.fs = self.vis = None
        self._own_ctx = False

    def __repr__(self):
        return f"rank {self.rank} of {self.world}"

    def open(self, frames, ctx=None):
        import srz
        self._own_ctx = ctx is None
        self.ctx = srz.Context(0, self.rank, self.world) if ctx is None else ctx
        self.fs = self.ctx.frameset(frames)
        assert self.fs.local_rows == self.local_rows, (self, self.fs.local_rows, self.local_rows)
        self.vis = visibility(self.fs)
        return self

    def close(self):
        if self.fs is not None:
            self.fs.close()
        if self._own_ctx and self.ctx is not None:
            self.ctx.close()
        self.ctx = self.fs = self.vis = None

    def local(self, a, fill=None):
        """a whole-frame array [n, k, H, W] → the rank's [n, k, local_rows, W], every row outside the rank's bands `fill` (default: NaN
        for a float array, SENTINEL for words)"""
        a = np.asarray(a)
        assert a.ndim == 4 and a.shape[2] == self.height, a.shape
        if fill is None:
            fill = np.nan if a.dtype.kind == "f" else SENTINEL
        out = np.full(a.shape[:2] + (self.local_rows, a.shape[3]), fill, a.dtype)
        out[:, :, self.local_at] = a[:, :, self.frame_rows]
        return out

    def owned(self, a):
        """the rank's rows of a local array [n, k, local_rows, W], in frame order"""
        a = np.asarray(a)
        assert a.ndim == 4 and a.shape[2] == self.local_rows, (a.shape, self.local_rows)
        return a[:, :, self.local_at]

    def padding(self, a):
        """the rows of a local array outside the rank's bands"""
        a = np.asarray(a)
        assert a.ndim == 4 and a.shape[2] == self.local_rows, (a.shape, self.local_rows)
        return a[:, :, self.is_pad]

    def dev(self, a, fill=None):
        """local(a, fill) on the device"""
        import torch
        return torch.as_tensor(np.ascontiguousarray(self.local(a, fill))).cuda()

    def acc(self, shape):
        """a float32 buffer on the device for a float-atomic sum: zeros — or, on a rank without a band, ACC_FILL in every word, so that
        "exactly as it was" tells a rank that adds nothing from one that clears or writes +0"""
        import torch
        return torch.full(tuple(shape), 0.0 if self.rows else ACC_FILL, dtype=torch.float32, device="cuda")

    def out(self, k, n=N_FRAMES, fill=SENTINEL):
        """an output buffer [n, k, local_rows, W] on the device, every word `fill`"""
        from support import filled
        return filled((n, k, self.local_rows, self.fs.width), fill)


def check_planes(shard, got_local, whole, what, before=SENTINEL):
    """a per-pixel output of a rank: the owned rows are the whole frame's rows word for word (a NaN for a NaN), and every padding word
    still holds what the buffer held before the call (`before`: one word, or the local array).  Prints and → (owned rows compared at
    lb >= 1, padding words checked)"""
    got, whole = np.ascontiguousarray(got_local).view(np.uint32), np.ascontiguousarray(whole).view(np.uint32)
    assert got.ndim == 4 and got.shape[2] == shard.local_rows and whole.shape[2] == shard.height, (what, got.shape, whole.shape)
    same(shard.owned(got), whole[:, :, shard.frame_rows], f"{what}, {shard}: owned rows")
    pad = shard.padding(got)
    held = before if np.isscalar(before) else shard.padding(np.ascontiguousarray(before).view(np.uint32))
    bad = pad != held
    assert not bad.any(), f"{what}, {shard}: {int(bad.sum())} padding words written, first {np.argwhere(bad)[:4].tolist()}: {pad[bad][:4]}"
    late = int(shard.late.sum())
    print(f"{what}, {shard}: owned rows at lb >= 1 compared {late}, padding words untouched {pad.size}")
    return late, pad.size


def mask_rows(v, rows, keep=0):
    """the whole frame's visibility words [n, 4, H, W] with the id plane of every row outside `rows` ([H] bool) set to `keep`"""
    m = np.array(v, np.uint32, copy=True)
    m[:, 1][:, ~rows] = keep
    return m


def masked_ids(v, shard, keep=0):
    """the whole frame's visibility words with the id plane of every row that is not the rank's set to `keep` (0: nobody, which takes
    those rows out of an owner pass) — what the pass's reference runs on for the rank's part of a sum"""
    return mask_rows(v, shard.mine, keep)


def check_rank_sum(parts, ref, mag, cnt, what, extra=0):
    """the float64 sum of the ranks' parts of a world against the whole frame's reference, within the whole frame's bound
    gamma_(n + extra) * sum |term| (each rank's sum lies within the bound of its own adds; the ranks' bounds add up to at most the
    whole frame's); exactly 0 where no pixel contributes.  Prints max err / bound → that ratio"""
    total = np.sum([np.asarray(p, np.float64).reshape(ref.shape) for p in parts], 0)
    cnt = np.broadcast_to(cnt, ref.shape).astype(np.float64)
    nu = (cnt + extra) * U
    assert np.isfinite(ref).all() and nu.max() < 1.0, what
    bound = nu / (1.0 - nu) * mag
    err = np.abs(total - ref)
    ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    print(f"{what}: the ranks together: max err {err.max():.3e}, max err / bound {ratio:.3f}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    assert (total[cnt == 0] == 0).all(), what
    return ratio


def band_masks(height=H):
    """[bands, H] bool: the rows of each band"""
    r = np.arange(height) // BAND
    return np.stack([r == b for b in range((height + BAND - 1) // BAND)])


# ------------------------------------------------------------------------------------------------------ the frames, the geometry
def make_frames(w, h=H):
    """two frames with different triangles: a soup in front of a backdrop that covers the lower right and leaves the upper left, down to
    the last band, to the soup and to nobody.  The frames do not clear: without SRZ_FUSED_CLEAR nobody's words stay"""
    out = []
    for i in range(N_FRAMES):
        back = ccw((w + 9, h + 8), (12 + 9 * i, h + 8), (w + 9, -60 - 30 * i), z=80.0, uv=((0.1, 0.2), (0.9, 0.3), (0.4, 0.95)))
        out.append(frame(np.concatenate([soup(20 + i, 40, w, h, ZS, big=True), back]), w, h, flags=0))
    return out


class Geo:
    """one geometry: its frames, the unsharded set (`whole`, a Shard of world 1 on the module's context) with everything the passes
    read, and the shards of the three layouts, each made on first use"""

    def __init__(self, ctx, name):
        self.name, (self.W, self.H) = name, GEOMETRIES[name]
        check_layouts(self.H)
        self.frames = make_frames(self.W, self.H)
        self.n = len(self.frames)
        self.whole = Shard(1, 0, self.H).open(self.frames, ctx)
        self.fs, self.vis = self.whole.fs, self.whole.vis
        self.whole.vis_in = self.vis
        self.v = words(self.vis)
        self.n_tris = [f.n_tris for f in self.frames]
        self.T = max(self.n_tris) + 2  # (the caller's arrays are longer than either frame's stream)
        assert self.T < 60
        self.own = ((self.v[:, 1] & np.uint32(0x7fffffff)) - np.uint32(1)) < np.uint32(self.n_tris)[:, None, None]
        for m in band_masks(self.H):  # owners and nobody's pixels in every band of every frame, in the last tile column too
            for part in (self.own[:, m], ~self.own[:, m], self.own[:, m][:, :, 64:]):
                assert part.reshape(self.n, -1).any(1).all(), name
        assert self.v[0, 1].tobytes() != self.v[1, 1].tobytes()
        self._shards = {}

    def shard(self, world, rank):
        """the shard with its own render checked against the whole frame's, and .vis_in: the rank's rows of the whole buffer written by
        hand, NaN in the padding's float planes and SENTINEL in its id plane — what the passes are given, so that a read of a padding
        row shows"""
        if (world, rank) not in self._shards:
            s = self._shards[world, rank] = Shard(world, rank, self.H).open(self.frames)
            check_planes(s, words(s.vis), self.v, "render_visibility", before=0)  # (local_rows is zero-padded: include/srz.h)
            hand = s.local(self.v.view(np.float32))
            hand[:, 1][:, s.is_pad] = np.uint32(SENTINEL).view(np.float32)
            s.vis_in = dev(hand)
        return self._shards[world, rank]

    def shards(self, worlds=None):
        """the ten shards, in the order of LAYOUTS (worlds: of those worlds only)"""
        return [self.shard(w, r) for w, ranks in LAYOUTS for r in ranks if worlds is None or w in worlds]

    def close(self):
        for s in self._shards.values():
            s.close()
        self.whole.close()

    def rng(self, salt):
        return np.random.default_rng([salt, self.W])

    def memo(self, key, make):
        if key not in self.__dict__.setdefault("_memo", {}):
            self._memo[key] = make(self)
        return self._memo[key]

    @functools.cached_property
    def pos(self):
        return padded_positions(self.frames, self.T)

    def planes(self, salt, k, scale=1.0, nan=None):
        """[n, k, H, W] float32 normal values; nan: a mask [n, H, W] of the pixels whose words are never read, which get NaN"""
        a = (self.rng(salt).normal(0, 1, (self.n, k, self.H, self.W)) * scale).astype(np.float32)
        if nan is not None:
            a[np.broadcast_to(nan[:, None], a.shape)] = np.nan
        return a


def make_geos(ctx):
    """the body of a module's `geos` fixture: yields get(name) → the Geo, made on first use; closes everything afterwards"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = Geo(ctx, name)
        return made[name]
    yield get
    for g in made.values():
        g.close()


def band_shares(shape, per_band_mag):
    """walkkit.Shares over the bands: per element of a summed output, the smallest non-zero sum |term| that one band adds into it.
    per_band_mag: one array of `shape` per band"""
    s = Shares(shape)
    for m in per_band_mag:
        s.add(np.asarray(m).reshape(shape))
    return s


# ------------------------------------------------------------------------------------------------------ one pass on every shard
def hold_pass(tmp, g, name, run, ref, fused_options):
    """One pass on one geometry, all three layouts.  run(tmp, g, S, fused) → (planes, sums) of the call on the Shard S (the unsharded
    g.whole included): planes name → local words, or (local words, the word its padding held before the call); sums name → float32
    array.  ref(tmp, g, rows, fused) → (planes name → whole-frame words, sums name → (ref, mag, cnt, extra)) of the pass's own
    reference on the whole frame with the rows outside `rows` ([H] bool) taken out of the pass (owner_pass: their ids written to
    nobody).
    1. the anchor: the unsharded call against the reference on every row — the planes word for word, the sums within their bound;
    2. every shard's planes through check_planes against the anchor, for every entry of fused_options;
    3. the sums (first entry of fused_options): teeth over the bands from the reference alone; every rank against the reference on its
       rows — bit for bit for a sum named in TREES —; the ranks of worlds 3 and 5 together against the whole frame's."""
    every = np.ones(g.H, bool)
    for first, fused in enumerate(fused_options):
        want_p, want_s = ref(tmp, g, every, fused)
        got_p, got_s = run(tmp, g, g.whole, fused)
        assert set(got_p) == set(want_p) and set(got_s) == set(want_s) and (want_p or want_s), name
        for k, w in want_p.items():
            same(_words(got_p[k])[0], w, f"{name} {k}, {g.name}, fused {fused}: the whole frame against the reference")
            assert (np.asarray(w).view(np.uint32) != SENTINEL).any(), (name, k)
        sums = bool(want_s) and first == 0
        if sums:
            per_band = [ref(tmp, g, m, fused)[1] for m in band_masks(g.H)]
            for k, (r, mag, cnt, extra) in want_s.items():
                if k.split()[0] in TREES:
                    same(got_s[k], r, f"{name} {k}, {g.name}: the whole frame against the reference's tree")
                elif not np.any(cnt):
                    assert not got_s[k].any(), (name, k)
                else:
                    teeth(band_shares(mag.shape, [pb[k][1] for pb in per_band]), mag, cnt, f"{name} {k}, {g.name}", single=False)
                    check_bound(got_s[k], r, mag, cnt, f"{name} {k}, {g.name}, whole frame", extra)
        late, pad = dict.fromkeys([w for w, _ in LAYOUTS], 0), dict.fromkeys([w for w, _ in LAYOUTS], 0)
        parts = {}
        for S in g.shards():
            p, s = run(tmp, g, S, fused)
            for k in want_p:
                got, before = _words(p[k])
                a, b = check_planes(S, got, _words(got_p[k])[0], f"{name} {k}, {g.name}, fused {fused}", before)
                late[S.world], pad[S.world] = late[S.world] + a, pad[S.world] + b
            if not sums:
                continue
            if not S.rows:  # the rank without a band adds nothing (a tree writes +0)
                for k in want_s:  # (Shard.acc: the atomic sums start from ACC_FILL on this rank)
                    held = np.float32(0.0 if k.split()[0] in TREES else ACC_FILL).view(np.uint32)
                    assert (np.ascontiguousarray(s[k], np.float32).view(np.uint32) == held).all(), f"{name} {k}: {S} wrote something"
                print(f"{name}, {g.name}, {S}: every float-atomic sum exactly as it was ({ACC_FILL} in every word), every tree +0")
                continue
            mine = ref(tmp, g, S.mine, fused)[1]
            for k, (r, mag, cnt, extra) in mine.items():
                if k.split()[0] in TREES:
                    same(s[k], r, f"{name} {k}, {g.name}, {S}: against the reference's tree on the rank's rows")
                    assert np.asarray(r).any(), (name, k, S)
                else:
                    check_bound(s[k], r, mag, cnt, f"{name} {k}, {g.name}, {S}", extra)
            assert any(cnt is None or np.any(np.asarray(cnt) > 0) for (_, _, cnt, _) in mine.values()), (name, S)
            parts.setdefault(S.world, []).append(s)
        if want_p:
            for w, _ in LAYOUTS:  # (ranks 6 and 7 of world 8 have no local band >= 1: theirs is the ragged band alone, and no band)
                print(f"{name}, {g.name}, fused {fused}, world {w}: owned rows at lb >= 1 compared {late[w]}, padding words untouched {pad[w]}")
                assert pad[w] > 0 and (late[w] > 0 or w not in SUM_WORLDS)
        for w in SUM_WORLDS if sums else ():
            assert len(parts[w]) == w
            for k, (r, mag, cnt, extra) in want_s.items():
                if k.split()[0] not in TREES:
                    check_rank_sum([p[k] for p in parts[w]], r, mag, cnt, f"{name} {k}, {g.name}, world {w}", extra)


def _words(x):
    return x if isinstance(x, tuple) else (x, SENTINEL)


def owner_pass(ref):
    """a reference that takes visibility words → hold_pass's ref: the rows outside `rows` get id 0, nobody, which takes them out of a
    pass over the owned pixels"""
    return lambda tmp, g, rows, fused: ref(tmp, g, mask_rows(g.v, rows), fused)


TREES = ("gpar", "gray")  # the sums reduced in a fixed tree (include/srz.h): bit-reproducible for a given shard layout
