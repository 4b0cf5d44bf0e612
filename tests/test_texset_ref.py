"""not-gpu: the texture-set pass's test reference (tests/texsetref.py, a composition of tests/texref.py) pinned on the oracle's
visibility buffers: one slot is texref itself, several slots are np.where over full per-slot results by the batch plane — and the
properties that keep the cases of tests/test_gpu_texture_set.py from passing vacuously, asserted on the reference alone."""
import numpy as np
import pytest

import interpref
import texref
import texsetref
from support import visibility_of
from texsetref import NONE, TG_SLOTS, TILE
from texref import CLAMP, WRAP


def buffers(tmp_path, orc, f):
    vis = visibility_of(tmp_path, orc, f)
    uv = interpref.forward(tmp_path, texref.frame_uv(f), vis.n, vis.words)
    return vis, np.ascontiguousarray(vis.words[1]), uv


def rand_gout(seed, shape):
    return np.random.default_rng([seed, 8]).normal(0, 2, shape).astype(np.float32)


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("mode", [CLAMP, WRAP])
@pytest.mark.parametrize("fused", [True, False])
def test_one_slot_is_texref_itself(tmp_path, orc, mode, fused):
    f = texsetref.three_frame()
    vis, ids, uv = buffers(tmp_path, orc, f)
    tex = texref.make_tex(1, 5, 7, 3)
    pre = np.full((3,) + ids.shape, 0xdeadbeef, np.uint32)
    got = texsetref.forward(tmp_path, f, [tex], [mode], (0, 0, 0), ids, uv, fused, pre)
    assert same_words(got, texref.forward(tmp_path, tex, mode, vis.n, ids, uv, fused, pre))
    gout = rand_gout(3, got.shape)
    acc, ref = [texref.Grad(tex.shape)], texref.Grad(tex.shape)
    pre2 = np.full((2,) + ids.shape, 0xdeadbeef, np.uint32)
    guv = texsetref.grad(tmp_path, f, [tex], [mode], (0, 0, 0), ids, uv, gout, acc, True, fused, pre2)
    assert same_words(guv, texref.grad(tmp_path, tex, mode, vis.n, ids, uv, gout, ref, True, fused, pre2))
    assert np.array_equal(acc[0].gtex, ref.gtex) and np.array_equal(acc[0].gabs, ref.gabs) and np.array_equal(acc[0].count, ref.count)
    assert ref.count.sum() >= 4 * 400


@pytest.mark.parametrize("fused", [True, False])
def test_several_slots_are_where_over_full_results_by_the_batch_plane(tmp_path, orc, fused):
    f = texsetref.holes_frame()
    vis, ids, uv = buffers(tmp_path, orc, f)
    texs = [texref.make_tex(1, 5, 7, 3), texref.make_tex(2, 33, 1, 3), texref.make_tex(3, 64, 64, 3)]
    modes = [CLAMP, WRAP, WRAP]
    fill = np.uint32(0xdeadbeef)
    pre = np.full((3,) + ids.shape, fill, np.uint32)
    got = texsetref.forward(tmp_path, f, texs, modes, texsetref.HOLES_MAP, ids, uv, fused, pre).view(np.uint32)
    b = texsetref.batch_plane(f, ids)
    assert np.array_equal(b >= 0, vis.own) and set(np.unique(b[vis.own])) == {0, 1, 2, 3, 4}
    want = np.where(vis.own, np.uint32(0), np.uint32(0) if fused else fill) * np.ones((3, 1, 1), np.uint32)
    gout = rand_gout(5, got.shape)
    want_uv = np.where(vis.own, np.uint32(0), np.uint32(0) if fused else fill) * np.ones((2, 1, 1), np.uint32)
    accs = [texref.Grad(t.shape) for t in texs]
    pre2 = np.full((2,) + ids.shape, fill, np.uint32)
    guv = texsetref.grad(tmp_path, f, texs, modes, texsetref.HOLES_MAP, ids, uv, gout, accs, True, fused, pre2).view(np.uint32)
    for batch, s in ((0, 1), (1, 0), (3, 2)):
        full = texref.forward(tmp_path, texs[s], modes[s], vis.n, ids, uv).view(np.uint32)
        want = np.where(b == batch, full, want)
        ref = texref.Grad(texs[s].shape)
        full_uv = texref.grad(tmp_path, texs[s], modes[s], vis.n, np.where(b == batch, ids, 0).astype(np.uint32), uv, gout, ref).view(np.uint32)
        want_uv = np.where(b == batch, full_uv, want_uv)
        assert np.array_equal(accs[s].gtex, ref.gtex) and np.array_equal(accs[s].count, ref.count) and ref.count.sum() > 0
    assert np.array_equal(got, want) and np.array_equal(guv, want_uv)
    # a map byte that names no slot is NONE
    again = texsetref.forward(tmp_path, f, texs, modes, texsetref.HOLES_MAP_200, ids, uv, fused, pre).view(np.uint32)
    assert np.array_equal(again, got)


def quad_slots(slots):
    """per aligned quad of four row pixels: the number of different slots (0 .. n_slots - 1) its pixels hold"""
    rows, W = slots.shape
    q = slots.reshape(rows, W // 4, 4)
    n = np.zeros((rows, W // 4), np.int64)
    for s in range(int(slots.max()) + 1):
        if s != NONE:
            n += (q == s).any(2)
    return n


def test_case_three_batches_alternate_within_quads(tmp_path, orc):
    """(a): at least 1 % of the frame's aligned quads hold two different slots, at least one holds three; every slot is sampled"""
    f = texsetref.three_frame()
    vis, ids, uv = buffers(tmp_path, orc, f)
    slots = texsetref.slot_plane(f, ids, texsetref.THREE_MAP, 3)
    n = quad_slots(slots)
    print(f"quads {n.size}: two slots {(n >= 2).sum()}, three {(n >= 3).sum()}")
    assert (n >= 2).sum() >= 0.01 * n.size and (n >= 3).sum() >= 1
    for s in range(3):
        cls = texref.classify(tmp_path, (7, 5), CLAMP, vis.n, np.where(slots == s, ids, 0).astype(np.uint32), uv)
        assert ((cls & texref.SAMPLED) != 0).sum() >= 200, s


@pytest.mark.parametrize("batch_slot", [texsetref.HOLES_MAP, texsetref.HOLES_MAP_200])
def test_case_holes_every_slot_none_and_beyond_the_map(tmp_path, orc, batch_slot):
    """(b): every slot is sampled, and pixels whose byte is NONE and pixels whose batch lies beyond the map both exist"""
    f = texsetref.holes_frame()
    vis, ids, uv = buffers(tmp_path, orc, f)
    slots, b = texsetref.slot_plane(f, ids, batch_slot, 3), texsetref.batch_plane(f, ids)
    for s in range(3):
        cls = texref.classify(tmp_path, (7, 5), CLAMP, vis.n, np.where(slots == s, ids, 0).astype(np.uint32), uv)
        assert ((cls & texref.SAMPLED) != 0).sum() >= 100, s
    assert ((b == 2) & (slots == NONE)).sum() >= 100 and ((b == 4) & (slots == NONE)).sum() >= 100
    assert len(batch_slot) == 4 and (b == 4).any()


def test_case_shared_two_slots_touch_the_same_texel_index_in_one_tile(tmp_path, orc):
    """(c): a table keyed on the texel index alone would merge them"""
    f = texsetref.shared_frame()
    vis, ids, _ = buffers(tmp_path, orc, f)
    tw, th = texsetref.SHARED_TEX
    uv = texsetref.centre_uv(1, 1, 64, 64, tw, th)[0]
    slots = texsetref.slot_plane(f, ids, (0, 1), 2)
    for tile in ((0, 0), (0, 1), (1, 0), (1, 1)):
        t0 = texsetref.touched(tmp_path, f, (th, tw), CLAMP, ids, uv, slots, 0, tile)
        t1 = texsetref.touched(tmp_path, f, (th, tw), WRAP, ids, uv, slots, 1, tile)
        assert len(t0 & t1) >= 10, tile


def test_case_overflow_the_pairs_exceed_the_table_no_single_slot_does(tmp_path, orc):
    """(d): some tile's distinct (slot, texel) pairs exceed TG_SLOTS while no single slot's do"""
    f = texsetref.overflow_frame()
    vis, ids, uv = buffers(tmp_path, orc, f)
    slots = texsetref.slot_plane(f, ids, (0, 1), 2)
    over = 0
    for ty in range(2):
        for tx in range(2):
            n = [len(texsetref.touched(tmp_path, f, (64, 64), CLAMP, ids, uv, slots, s, (ty, tx))) for s in (0, 1)]
            print(f"tile {ty, tx}: distinct texels per slot {n}")
            assert max(n) <= TG_SLOTS
            over += sum(n) > TG_SLOTS
    assert over >= 1
    assert TILE == 32
