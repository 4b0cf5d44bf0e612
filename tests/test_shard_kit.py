"""The shard kit bites: on the CPU, without the library.  tests/test_gpu_pass_shards.py and tests/test_gpu_pass_shards_lit.py hold every
pass over a visibility buffer to its whole-frame words on the band shards of tests/shardkit.py; this file pins the kit itself — the
layout facts the two modules rely on, from srz.parallel's formulas; that local / owned / padding round-trip and partition a rank's
buffer; and that check_planes and check_rank_sum raise on what they are there to see: a wrong row, a write into the padding, a band
stored at the wrong local band, the frame's row confused with the shard-local one, a rank's part lost or added twice.  The last
test runs shardkit.hold_pass itself on the background pass by its reference alone: the reference's own results pass; the shard-local
row in the ray, a rank's sums without one of its bands, a rank that writes the whole frame's gray, and a rank without a band that
clears the caller's accumulator are each seen."""
import numpy as np
import pytest

import shardkit
from shardkit import BAND, H, LAYOUTS, Shard, check_planes, check_rank_sum
from srz import parallel
from support import SENTINEL

W, N, K = 70, 2, 3
ALL = [(w, r) for w, ranks in LAYOUTS for r in ranks]


def whole_planes(seed=1):
    return np.random.default_rng(seed).integers(1, 1 << 30, (N, K, H, W)).astype(np.uint32)


def test_layout_facts():
    own = shardkit.check_layouts()
    assert len(ALL) == 10
    # the two passes whose value is a function of the frame's row have rotated rows at lb >= 1 to be compared on
    assert shardkit.rotated_rows(H, 0, 3) == 32 and shardkit.rotated_rows(H, 1, 3) == 32 + 5 and shardkit.rotated_rows(H, 2, 3) == 32
    assert shardkit.rotated_rows(H, 1, 5) == 32 and shardkit.rotated_rows(H, 2, 5) == 5
    assert own[3, 1][2] == 6 and own[5, 2][1] == 6
    for (w, r) in ALL:  # the kit's rows are parallel.band_rows's
        s = Shard(w, r)
        assert s.local_rows == parallel.shard_layout(H, r, w)["local_rows"] and s.local_rows % BAND == 0
        assert len(s.frame_rows) == sum(r1 - r0 for (_, _, r0, r1) in s.rows) == int(s.mine.sum())
        for (lb, b, r0, r1) in s.rows:
            assert b == parallel.band_of(lb, r, w) and parallel.rank_of_band(b, w) == r


@pytest.mark.parametrize("world,rank", ALL)
def test_local_owned_padding_partition_the_buffer(world, rank):
    s, a = Shard(world, rank), whole_planes()
    loc = s.local(a)
    assert loc.shape == (N, K, s.local_rows, W) and loc.dtype == a.dtype
    assert np.array_equal(s.owned(loc), a[:, :, s.frame_rows])  # round trip
    assert (s.padding(loc) == SENTINEL).all()
    assert s.owned(loc).shape[2] + s.padding(loc).shape[2] == s.local_rows  # every local row is one or the other
    assert len(np.intersect1d(s.local_at, np.flatnonzero(s.is_pad))) == 0
    f = s.local(a.astype(np.float32))
    assert np.isnan(s.padding(f)).all() and not np.isnan(s.owned(f)).any()
    assert (s.local(a, 7)[:, :, s.is_pad] == 7).all()
    for (lb, _, r0, r1) in s.rows:  # a band lies at its local band
        assert np.array_equal(loc[:, :, lb * BAND: lb * BAND + r1 - r0], a[:, :, r0:r1])
    check_planes(s, loc, a, "untouched")


def test_the_ranks_of_a_world_partition_the_frame():
    for w, _ in LAYOUTS:
        seen = np.zeros(H, np.int64)
        for r in range(w):
            seen += Shard(w, r).mine
        assert (seen == 1).all(), w
    one = Shard(1, 0)
    assert one.local_rows == H and one.mine.all() and not one.is_pad.any()


def raises(*args, **kw):
    with pytest.raises(AssertionError):
        check_planes(*args, **kw)


@pytest.mark.parametrize("world,rank", [(3, 0), (3, 1), (3, 2), (5, 1), (5, 2), (8, 6)])
def test_check_planes_sees_what_it_is_there_for(world, rank):
    s, a = Shard(world, rank), whole_planes()
    good = s.local(a)
    assert check_planes(s, good, a, "good")[1] == good[:, :, s.is_pad].size
    # a wrong word in an owned row: the first and the last owned row
    for row in (s.local_at[0], s.local_at[-1]):
        bad = good.copy()
        bad[1, 2, row, W - 1] ^= 1
        raises(s, bad, a, "wrong row")
    # a write into the padding: the first padding row (the ragged band's tail, or the missing local band) and the last
    pad_rows = np.flatnonzero(s.is_pad)
    assert len(pad_rows) or (world, rank) == (5, 1)  # (rank 1 of 5 owns two full bands of two)
    for row in pad_rows[[0, -1]] if len(pad_rows) else ():
        bad = good.copy()
        bad[0, 0, row, 0] = 0
        raises(s, bad, a, "padding")
    # the padding's own prefill, given as the local array
    pre = np.random.default_rng(3).integers(0, 1 << 31, good.shape).astype(np.uint32)
    mixed = pre.copy()
    mixed[:, :, s.local_at] = good[:, :, s.local_at]
    check_planes(s, mixed, a, "own prefill", before=pre)
    if len(pad_rows):
        mixed[0, 1, pad_rows[0], 5] += 1
        raises(s, mixed, a, "own prefill", before=pre)
    if len(s.rows) >= 2:
        # a band stored at the wrong local band: the first two exchanged
        (l0, _, a0, a1), (l1, _, b0, b1) = s.rows[0], s.rows[1]
        bad = np.full_like(good, SENTINEL)
        bad[:, :, l0 * BAND: l0 * BAND + b1 - b0] = a[:, :, b0:b1]
        bad[:, :, l1 * BAND: l1 * BAND + a1 - a0] = a[:, :, a0:a1]
        for (lb, _, r0, r1) in s.rows[2:]:
            bad[:, :, lb * BAND: lb * BAND + r1 - r0] = a[:, :, r0:r1]
        raises(s, bad, a, "wrong lb")
        # the rows of band lb * world + rank in place of band_of(lb, rank, world)'s: a map without the rotation
        bad = good.copy()
        for (lb, b, r0, r1) in s.rows:
            r = (lb * world + rank) * BAND
            k = min(r1 - r0, H - r)
            if r != r0 and k > 0:
                bad[:, :, lb * BAND: lb * BAND + k] = a[:, :, r: r + k]
        assert not np.array_equal(bad, good) or (world, rank) == (5, 2)  # (band 2 + 5 does not exist)
        if not np.array_equal(bad, good):
            raises(s, bad, a, "no rotation")
    # a value that is a function of the row: the shard-local row in place of the frame's
    y = np.broadcast_to(np.arange(H, dtype=np.uint32)[None, None, :, None], (N, K, H, W))
    by_local = np.broadcast_to(np.arange(s.local_rows, dtype=np.uint32)[None, None, :, None], (N, K, s.local_rows, W)).copy()
    by_local[:, :, s.is_pad] = SENTINEL
    raises(s, by_local, y, "local row")


def test_a_rank_without_a_band():
    s, a = Shard(8, 7), whole_planes()
    loc = s.local(a)
    assert s.rows == [] and s.local_rows == BAND and (loc == SENTINEL).all() and s.owned(loc).shape[2] == 0
    assert check_planes(s, loc, a, "nothing")[1] == loc.size
    loc[1, 0, 31, 69] = 1
    raises(s, loc, a, "a write by the rank without a band")


def test_masked_ids_and_check_rank_sum():
    v = np.random.default_rng(4).integers(1, 50, (N, 4, H, W)).astype(np.uint32)
    for w in shardkit.SUM_WORLDS:
        parts = [shardkit.masked_ids(v, Shard(w, r)) for r in range(w)]
        assert all(np.array_equal(p[:, [0, 2, 3]], v[:, [0, 2, 3]]) for p in parts)
        assert np.array_equal(np.sum([p[:, 1].astype(np.int64) for p in parts], 0), v[:, 1])  # every row is one rank's
        assert np.array_equal(shardkit.masked_ids(v, Shard(w, 0), 9)[:, 1][:, ~Shard(w, 0).mine], np.full((N, H - Shard(w, 0).mine.sum(), W), 9))
    # sums: 20 elements of 400 terms each, dealt to three ranks
    rng = np.random.default_rng(5)
    terms = rng.normal(0, 1, (3, 400, 20)).astype(np.float32).astype(np.float64)
    ref, mag, cnt = terms.sum((0, 1)), np.abs(terms).sum((0, 1)), np.full(20, 1200)
    parts = [terms[r].sum(0).astype(np.float32) for r in range(3)]
    assert check_rank_sum(parts, ref, mag, cnt, "sum") <= 1
    with pytest.raises(AssertionError):
        check_rank_sum(parts[:2], ref, mag, cnt, "a rank lost")
    with pytest.raises(AssertionError):
        check_rank_sum(parts + parts[2:], ref, mag, cnt, "a rank twice")
    with pytest.raises(AssertionError):  # an element nobody adds into must stay 0
        check_rank_sum([np.float32([1e-30])], np.zeros(1), np.zeros(1), np.zeros(1), "untouched")


# ------------------------------------------------------------------------------------------------------ hold_pass, on the background pass
class StubGeo:
    """what hold_pass asks of a geometry, without a device: the rows of every shard"""
    name, H, W = "w70 on the CPU", H, W
    whole = Shard(1, 0)

    def shards(self):
        return [Shard(w, r) for (w, r) in ALL]


def background_case(tmp):
    """the background pass with SRZ_BG_NOBODY by its reference alone (tests/backgroundref.py) on hand-written owner words with holes:
    → (ref, run) for hold_pass, run(fault) answering with the reference's own results rounded to float32 — or with a planted fault"""
    import backgroundref as br
    import cuberef
    import iblref
    tris, C = 20, 3
    ids0 = iblref.rand_ids(np.random.default_rng(5), N, H, W, tris)
    cube = cuberef.make_cube(31, 4, C, frames=N)
    rays = np.stack([br.camera_block(W, H, i, 1.6) for i in range(N)])
    gout = np.random.default_rng(6).normal(0, 2, (N, C, H, W)).astype(np.float32)

    def on(ids, h, fused):
        """the reference on frames of h rows with these ids → (out words [N, C, h, W], gray rows, the cubes' Grads)"""
        accs = [br.Grad(cube.shape[-4:]) for _ in range(N)]
        pre = np.full((C, h, W), SENTINEL, np.uint32)
        out = np.stack([br.forward(tmp, cube[i], tris, ids[i], rays[i], br.NOBODY, fused, pre) for i in range(N)]).view(np.uint32)
        g = gout if h == H else np.zeros((N, C, h, W), np.float32)
        rows = np.stack([br.grad(tmp, cube[i], tris, ids[i], rays[i], g[i], accs[i])[0] for i in range(N)])
        return out, rows, accs

    def ref(tmp_, g, rows, fused):
        ids = ids0.copy()
        ids[:, ~rows] = 1  # a valid owner: those rows leave the pass
        out, gray, accs = on(ids, H, fused)
        return {"out": out}, {"gray": (gray, None, None, 0),
                              "gtex": (np.stack([a.gtex for a in accs]), np.stack([a.gabs for a in accs]), np.stack([a.count for a in accs])[..., None], 0)}

    def run(fault=None):
        def call(tmp_, g, S, fused):
            whole, _ = ref(tmp_, g, np.ones(H, bool), fused)
            _, mine = ref(tmp_, g, S.mine, fused)
            out = S.local(whole["out"])
            sums = {k: np.asarray(r).astype(np.float32) for k, (r, _, _, _) in mine.items()}
            if not S.rows:  # the rank without a band: Shard.acc's prefill stays in the atomic sums
                sums["gtex"] = np.full_like(sums["gtex"], 0.0 if fault == "the empty rank clears" else shardkit.ACC_FILL)
            if fault == "local row" and S.world > 1:  # the rank's rows taken for a frame of local_rows rows: y is the local row
                ids = S.local(ids0[:, None])[:, 0]
                out = on(ids, S.local_rows, fused)[0]
                out[:, :, S.is_pad] = SENTINEL
            if fault == "lost band" and S.world > 1 and len(S.rows) >= 2:  # the sums without the rank's last band
                less = S.mine.copy()
                less[S.rows[-1][2]:S.rows[-1][3]] = False
                sums["gtex"] = ref(tmp_, g, less, fused)[1]["gtex"][0].astype(np.float32)
            if fault == "gray of the whole frame" and S.world > 1:
                sums["gray"] = ref(tmp_, g, np.ones(H, bool), fused)[1]["gray"][0]
            return {"out": out}, sums
        return call
    return ref, run


def test_hold_pass_passes_the_reference_and_sees_planted_faults(tmp_path):
    ref, run = background_case(tmp_path)
    shardkit.hold_pass(tmp_path, StubGeo(), "background", run(), ref, (False, True))
    for fault in ("local row", "lost band", "gray of the whole frame", "the empty rank clears"):
        with pytest.raises(AssertionError):
            shardkit.hold_pass(tmp_path, StubGeo(), "background", run(fault), ref, (False, True))
