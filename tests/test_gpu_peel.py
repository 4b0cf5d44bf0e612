"""-m gpu: depth peeling (srz_frameset_peel_visibility, k_peel) against the oracle-built reference of tests/peelref.py — every
comparison with it bit for bit on the four words, at the pixels the reference keeps: layers 2-4 of every scene, the tie order on
hand-made frames, the layer-1 identity with the visibility render, completeness against the oracle's fragment count, sets (the small
job's clear in the rasteriser, the batch's side clear), the stream feeder after a pool overflow, sharding, hostile previous layers,
and the layers feeding the passes and the gradient chain."""
import numpy as np
import pytest
import torch

import peelref
import srz
import visref
from srz import abi, parallel, visibility
from support import SENTINEL, ccw, ctx, filled, frame, soup, stream, words  # noqa: F401  (ctx: the fixture)

pytestmark = pytest.mark.gpu

NAMES = list(peelref.SCENES)


@pytest.fixture(scope="module")
def shared_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("peelref")


def same_kept(got, exp, keep, what):
    for p in range(4):
        bad = (got[p] != exp[p]) & keep
        assert not bad.any(), f"{what}: plane {p} differs at {int(bad.sum())} kept pixels, first {np.argwhere(bad)[:4].tolist()}: " \
                              f"got {got[p][bad][:4]} want {exp[p][bad][:4]}"


def device_layers(fs, n, flags=abi.FUSED_CLEAR):
    """the first n layers of the set as uint32 words [n][frames, 4, local_rows, W]"""
    ls = visibility.layers(fs, n, flags, stream())
    torch.cuda.synchronize()
    return [words(t) for t in ls]


def owned(w):
    return w[..., 1, :, :] != 0


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("name", NAMES)
def test_layers_2_to_4_equal_the_reference(ctx, shared_tmp, orc, name):
    ref = peelref.reference(shared_tmp, orc, name)
    H, W = ref.left.shape
    fs = ctx.frameset([ref.base.gpu_frame])
    got = device_layers(fs, 4)
    for k in (1, 2, 3):
        lay = ref.layers[min(k, len(ref.layers) - 1)]  # (behind the reference's last layer, all nobody, lies nobody)
        assert k < len(ref.layers) or not lay.own.any()
        same_kept(got[k][0, :, :H], lay.words, lay.keep, f"{name} layer {k + 1}")
    fs.close()


# ------------------------------------------------------------------------------------------------ 2. the tie order, hand-made
WIDE = ((2, 2), (30.5, 4), (6, 28.25))      # a box 29 columns wide: columns 2..25 are V, 26..30 S
NARROW = ((10, 2), (15.5, 20), (11, 30))    # a box 6 columns wide: every column S


def check_order(ctx, tris, what, min_pixels, expect=None):
    """frame 0 holds the triangles `tris` (all of ONE depth as floats compare), frames 1.. one of them each: at every pixel the layers of
    frame 0 name the triangles present there (known, with their classes, from the frames that hold one) in THE ORDER of include/srz.h —
    S by index descending, then V ascending — with that triangle's own words, and nobody behind the last.  expect: the owners of the
    layers at the pixels where every triangle is present (>= min_pixels of them)"""
    n = len(tris)
    fs = ctx.frameset([frame(np.concatenate(tris))] + [frame(t) for t in tris])
    got = device_layers(fs, n + 1)
    alone = got[0][1:]                                                 # [n, 4, H, W]: layer 1 of the one-triangle frames
    present = owned(alone)
    assert not owned(got[1][1:]).any()                                 # (one fragment per pixel there: layer 2 is nobody)
    z = alone[:, 0].view(np.float32)
    assert all((z[i][present[i] & present[j]] == z[j][present[i] & present[j]]).all() for i in range(n) for j in range(n))
    s_class = (alone[:, 1] >> 31) != 0
    tb = peelref.tie_break(np.arange(n, dtype=np.uint32)[:, None, None] + np.zeros_like(alone[:, 1]), s_class).astype(np.int64)
    tb[~present] = 1 << 40
    order = np.argsort(tb, 0)                                          # [n, H, W]: the triangles by place, the absent ones last
    count = present.sum(0)
    ys, xs = np.mgrid[0:64, 0:64]
    for j in range(n + 1):
        there = count > j
        exp = peelref.nobody(64, 64)
        if j < n:
            exp = np.where(there[None], alone[order[j], :, ys, xs].transpose(2, 0, 1), exp)
            exp[1] = np.where(there, (exp[1] & 0x80000000) | (order[j].astype(np.uint32) + 1), 0)  # (alone, every triangle is index 0)
        same_kept(got[j][0], exp, np.ones((64, 64), bool), f"{what} layer {j + 1}")
    full = count == n
    assert int(full.sum()) >= min_pixels, int(full.sum())
    if expect is not None:
        for j, e in enumerate(expect):
            assert ((got[j][0, 1][full] & 0x7fffffff) == e + 1).all(), (what, j)
    fs.close()
    return got


def test_tie_order_of_one_triangle_four_times(ctx):
    v = check_order(ctx, [ccw(*WIDE, z=2.0)] * 4, "four V", 200)
    wide_v = (v[0][0, 1] != 0) & ((v[0][0, 1] >> 31) == 0)
    for j in range(4):  # V ascending, in the 8-wide columns; the same triangle's scalar tail descends
        assert (v[j][0, 1][wide_v] == j + 1).all() and (v[j][0, 1][(v[0][0, 1] >> 31) != 0] == (0x80000000 | (4 - j))).all()
    s = check_order(ctx, [ccw(*NARROW, z=2.0)] * 4, "four S", 40, expect=[3, 2, 1, 0])
    assert ((s[0][0, 1] >> 31) != 0)[s[0][0, 1] != 0].all()


def test_tie_order_mixed_classes_and_signed_zeros(ctx):
    # equal depths from different triangles and classes: z = 0 is the one depth both z expressions give exactly
    mixed = [ccw(*WIDE, z=0.0), ccw(*NARROW, z=0.0), ccw(*WIDE, z=0.0), ccw(*NARROW, z=0.0)]
    check_order(ctx, mixed, "mixed V S V S", 20, expect=[3, 1, 0, 2])
    # +0 and -0 compare equal: the order is the tie order, each layer keeps its own z word
    got = check_order(ctx, [ccw(*WIDE, z=0.0), ccw(*WIDE, z=-0.0)], "+0 then -0", 200)
    v = (got[0][0, 1] != 0) & ((got[0][0, 1] >> 31) == 0)
    assert (got[0][0, 0][v] == 0).all() and (got[1][0, 0][v] == 0x80000000).all()
    got = check_order(ctx, [ccw(*WIDE, z=-0.0), ccw(*WIDE, z=0.0)], "-0 then +0", 200)
    assert (got[0][0, 0][v] == 0x80000000).all() and (got[1][0, 0][v] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. layer 1
@pytest.mark.parametrize("name", NAMES)
def test_peel_of_first_prev_is_the_visibility_render(ctx, shared_tmp, orc, name):
    fs = ctx.frameset([peelref.reference(shared_tmp, orc, name).base.gpu_frame])
    vis = torch.full(fs.out_shape, -1.0, dtype=torch.float32, device="cuda")  # (the rows of the last band below the frame are nobody's to write)
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
    out = torch.full(fs.out_shape, -1.0, dtype=torch.float32, device="cuda")
    visibility.peel(fs, visibility.first_prev(fs), out=out, stream=stream())
    torch.cuda.synchronize()
    assert np.array_equal(words(out), words(vis)), f"{name}: {int((words(out) != words(vis)).sum())} words differ"
    assert owned(words(out)).any()
    fs.close()


def test_flags_ordered_raster_has_no_effect_and_the_clear_is_implied(ctx, shared_tmp, orc):
    fs = ctx.frameset([peelref.reference(shared_tmp, orc, "soup70x45").base.gpu_frame])
    l1 = visibility.layers(fs, 1, stream=stream())[0]
    outs = []
    for flags in (abi.FUSED_CLEAR, abi.FUSED_CLEAR | abi.ORDERED_RASTER, 0):
        out = filled(fs.out_shape).view(torch.float32)
        visibility.peel(fs, l1, out=out, flags=flags, stream=stream())
        outs.append(out)
    torch.cuda.synchronize()
    assert np.array_equal(words(outs[1]), words(outs[0])) and np.array_equal(words(outs[2]), words(outs[0]))
    assert not (words(outs[0])[:, :, :fs.height] == SENTINEL).any() and owned(words(outs[0])[:, :, :fs.height]).any()
    fs.close()


# ------------------------------------------------------------------------------------------------ 4. completeness
@pytest.mark.parametrize("name", NAMES)
def test_peeling_until_empty_visits_every_fragment_once(ctx, shared_tmp, orc, name):
    ref = peelref.reference(shared_tmp, orc, name)
    fs = ctx.frameset([ref.base.gpu_frame])
    lay, total, n_layers = visibility.layers(fs, 1, stream=stream())[0], 0, 0
    while True:
        n_layers += 1
        n_owned = int((lay.view(torch.int32)[:, 1, :fs.height] != 0).sum())  # (rows of the last band below the frame are never written)
        if n_owned == 0:
            break
        assert n_layers <= len(ref.layers), f"{name}: layer {n_layers} still owns {n_owned} pixels, the reference ended at {len(ref.layers)}"
        total += n_owned
        lay = visibility.peel(fs, lay, stream=stream())
    assert n_layers == len(ref.layers)
    assert total == fs.stats()["fragments"], (total, fs.stats())
    fs.close()


# ------------------------------------------------------------------------------------------------ 5. sets
def first_and_second(fs):
    """(peel of first_prev, layer 2) of the set as words"""
    s = stream()
    l1 = visibility.peel(fs, visibility.first_prev(fs), stream=s)
    l2 = visibility.peel(fs, l1, stream=s)
    torch.cuda.synchronize()
    return words(l1), words(l2)


def test_a_set_of_eleven_frames_equals_its_frames_one_by_one(ctx):
    counts = [150, 0, 1, 40, 7, 90, 12, 3, 64, 65, 129]  # (not a multiple of 8 frames; an empty one, one triangle)
    tris = [soup(20 + i, n, 64, 64, peelref.ZS, big=True) if n > 1 else ccw(*WIDE)[:n] for i, n in enumerate(counts)]
    frames = [frame(t) for t in tris]
    fs = ctx.frameset(frames)
    assert fs.n_frames * 4 < 8192  # (the small job: no side clear, k_peel's waves clear the tiles no box reaches)
    l1, l2 = first_and_second(fs)
    assert not owned(l1[1]).any() and owned(l1[2]).any() and not owned(l2[2]).any() and owned(l2[0]).any()
    for i, f in enumerate(frames):
        one = ctx.frameset([f])
        o1, o2 = first_and_second(one)
        assert np.array_equal(l1[i], o1[0]) and np.array_equal(l2[i], o2[0]), f"frame {i} of the set differs from its own one-frame set"
        one.close()
    fs.close()


def test_a_batch_with_the_side_clear_equals_its_frames_one_by_one(ctx):
    size, rng = 1024, np.random.default_rng(77)
    frames = []
    for i in range(9):  # 9 * 1024 tiles > 8192: the clear runs beside k_peel on its own stream
        n = 12 + 2 * i
        t = soup(40 + i, n, 96, 96, peelref.ZS, big=True)
        t["pos"][:, :, :2] += rng.uniform(0, size - 96, (n, 1, 2)).astype(np.float32)
        t["pos"][: n // 3, :, :2] = t["pos"][n // 3: 2 * (n // 3), :, :2] + np.float32(3.25)  # (some on top of others: a layer 2)
        frames.append(frame(t, size, size))
    fs = ctx.frameset(frames)
    l1, l2 = first_and_second(fs)
    vis = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
    torch.cuda.synchronize()
    assert np.array_equal(l1, words(vis)) and owned(l2).any()
    for i in (0, 4, 8):
        one = ctx.frameset([frames[i]])
        o1, o2 = first_and_second(one)
        assert np.array_equal(l1[i], o1[0]) and np.array_equal(l2[i], o2[0]), f"frame {i} of the batch differs from its own one-frame set"
        one.close()
    fs.close()


# ------------------------------------------------------------------------------------------------ 6. the stream feeder
def test_unlisted_bands_are_fed_from_the_stream(ctx, tmp_path, orc):
    """SRZ_OPT_POOL_LAZY (the recipe of tests/test_gpu_vertex_stage.py): 24 screen-filling triangles overflow the first guess of the
    list pool; the set's FIRST call is a peel, whose overflowing bands are fed from the frame's stream; the pool then grows and the
    same call is fed from the lists — both give the oracle's layer 1"""
    n, size = 24, 1024
    t = np.zeros(n, abi.TRI_DTYPE)
    for i in range(n):
        t["pos"][i] = [[-40 + 3 * i, -30, 10 + i % 5], [size + 50 - i, 10 + 2 * i, 12 + (i * 7) % 5], [200 + 5 * i, size + 60, 11 + (i * 3) % 7]]
    t["nrm"] = [0, 0, -1]
    ref = visref.Reference(tmp_path, frame(t, size, size, eye=(0.0, 0.0, -1.0)))
    exp, _, amb, _, own = ref.expected(orc)
    assert amb == 0 and int(own.sum()) > 500000
    ctx.set_option(abi.OPT_POOL_LAZY, 1)
    try:
        fs = ctx.frameset([ref.gpu_frame])
    finally:
        ctx.set_option(abi.OPT_POOL_LAZY, 0)
    counters = []
    for it in range(3):
        out = visibility.peel(fs, visibility.first_prev(fs), stream=stream())
        counters.append(fs.debug_counters())  # (waits for the device)
        same_kept(words(out)[0], exp, np.ones((size, size), bool), f"peel {it} of the lazy set")
    print(counters)
    assert counters[0]["slow_tiles"] > 0 and counters[0]["pool_demand"] > counters[0]["pool_sub_cap"], counters
    assert counters[-1]["slow_tiles"] == 0 and counters[-1]["pool_sub_cap"] >= counters[-1]["pool_demand"], counters
    fs.close()


# ------------------------------------------------------------------------------------------------ 7. sharding
def test_a_shard_peels_its_own_rows(ctx, shared_tmp, orc):
    ref = peelref.reference(shared_tmp, orc, "soup96x80")
    f, h = ref.base.gpu_frame, 80
    fs = ctx.frameset([f])
    full = device_layers(fs, 3)
    c = srz.Context(0, 1, 2)
    try:
        part = c.frameset([f])
        got = device_layers(part, 3)
        rows = parallel.band_rows(h, 1, 2)
        assert rows
        for k in (1, 2):
            for (lb, _, r0, r1) in rows:
                assert np.array_equal(got[k][0, :, lb * 32: lb * 32 + r1 - r0], full[k][0, :, r0:r1]), (k, lb)
            assert owned(got[k]).any()
        part.close()
    finally:
        c.close()
    fs.close()


# ------------------------------------------------------------------------------------------------ 8. a hostile previous layer
def test_any_words_in_prev_give_the_rule_and_stay_inside_the_buffer(ctx, shared_tmp, orc):
    ref = peelref.reference(shared_tmp, orc, "stack12")
    fs = ctx.frameset([ref.base.gpu_frame])
    l1 = device_layers(fs, 1)[0][0]  # [4, 64, 64]
    rng = np.random.default_rng(8)
    prev = l1.copy()
    kind = rng.integers(0, 8, (64, 64))
    ids = prev[1]
    bad_ids = rng.choice(np.uint32([ref.n + 1, ref.n + 2, 0x7fffffff, 0x80000000, 0xffffffff, 0x80000000 | (ref.n + 1), 1 << 22, 0]), (64, 64))
    ids = np.where(kind == 1, bad_ids, ids)                                         # ids out of range
    ids = np.where(kind == 2, ids ^ np.uint32(0x80000000), ids)                      # the S bit flipped
    zw = prev[0]
    zw = np.where(kind == 3, rng.choice(np.uint32([0x7fc00000, 0xffc00000, 0x7f800001, 0xff812345]), (64, 64)), zw)  # NaNs
    zw = np.where(kind == 4, np.uint32(0x7f800000), zw)                              # +inf
    zw = np.where(kind == 5, np.uint32(0xff800000), zw)                              # -inf
    rnd = rng.integers(0, 2 ** 32, (4, 64, 64), dtype=np.uint64).astype(np.uint32)
    rnd[1] = np.where(rng.random((64, 64)) < 0.5, rng.integers(0, 2 * ref.n, (64, 64)).astype(np.uint32) | (rnd[1] & 0x80000000), rnd[1])
    rnd[0] = np.where(rng.random((64, 64)) < 0.5, rng.choice(np.float32([0.5, 1, 2, 3, 4, 5, 6, 7, 8, 9]), (64, 64)).view(np.uint32), rnd[0])
    prev[0], prev[1] = zw, ids
    prev = np.where((kind >= 6)[None], rnd, prev)                                    # random words (depths among the scene's, too)
    prev[2:] = rnd[2:]
    exp, keep = peelref.next_after(ref, prev, ref.n)
    print(f"hostile prev: the rule owns {int((exp[1] != 0).sum())} pixels, ends {int((exp[1] == 0).sum())}")
    assert (exp[1] != 0).sum() > 50 and (exp[1][kind == 1] == 0).all() and (exp[1][kind == 3] == 0).all()
    n_words, guard = 4 * 64 * 64, 4 * 64 * 2  # two rows of every plane's width in front and behind
    buf = filled((guard + n_words + guard,))
    out = buf[guard:guard + n_words]
    d_prev = torch.as_tensor(prev.view(np.int32)).cuda().contiguous()
    fs.peel_visibility(d_prev.data_ptr(), out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
    torch.cuda.synchronize()
    got = words(buf)
    assert (got[:guard] == SENTINEL).all() and (got[guard + n_words:] == SENTINEL).all()
    same_kept(got[guard:guard + n_words].reshape(4, 64, 64), exp, keep, "hostile prev")
    fs.close()


# ------------------------------------------------------------------------------------------------ 9. layers feed the passes
def test_passes_over_layer_2_equal_passes_over_the_reference_layer(ctx, shared_tmp, orc):
    ref = peelref.reference(shared_tmp, orc, "soup96x80")
    H, W = ref.left.shape
    fs = ctx.frameset([ref.base.gpu_frame])
    dev = visibility.layers(fs, 2, stream=stream())[1]
    up = np.zeros((1,) + tuple(fs.out_shape[1:]), np.uint32)
    up[0] = peelref.nobody(fs.out_shape[2], W)
    up[0, :, :H] = ref.layers[1].words
    host = torch.as_tensor(up.view(np.float32)).cuda().contiguous()
    keep = np.zeros(fs.out_shape[2:], bool)
    keep[:H] = ref.layers[1].keep
    attr = torch.as_tensor(np.random.default_rng(3).uniform(-1, 1, (ref.n, 3, 3)).astype(np.float32)).cuda()
    a, b = visibility.interpolate(fs, dev, attr, stream()), visibility.interpolate(fs, host, attr, stream())
    ga, gb = (torch.zeros(fs.gbuffer_shape(abi.GB_ALL), dtype=torch.float32, device="cuda") for _ in range(2))
    for v, g in ((dev, ga), (host, gb)):
        fs.gbuffer(v.data_ptr(), g.data_ptr(), fs.gbuffer_bytes(abi.GB_ALL), abi.GB_ALL, abi.FUSED_CLEAR, stream())
    torch.cuda.synchronize()
    for x, y, what in ((a, b, "interpolate"), (ga, gb, "gbuffer")):
        bad = (words(x)[0] != words(y)[0]) & keep
        assert not bad.any(), f"{what} over layer 2: {int(bad.sum())} words differ"
    assert (words(a)[0] != 0).any() and (words(ga)[0] != 0).any()
    fs.close()


def test_a_loss_on_the_composed_image_reaches_a_hidden_triangle(ctx):
    back = ccw((12, 12), (34, 15), (16, 36), z=5.0)
    front = ccw((2, 2), (62, 6), (8, 62), z=1.0)  # covers `back` completely
    fs = ctx.frameset([frame(np.concatenate([back, front]))])
    first = visibility.decode(visibility.layers(fs, 1, stream=stream())[0])
    assert bool((first.tri == 1).any()) and not bool((first.tri == 0).any())  # layer 1 hides triangle 0

    def grad(n_layers):
        attr = torch.ones((2, 3, 3), dtype=torch.float32, device="cuda", requires_grad=True)
        ls = visibility.layers(fs, n_layers, stream=stream())
        colors = [visibility.interpolate(fs, lay, attr, stream()) for lay in ls]
        alphas = [(visibility.decode(lay).tri >= 0).to(torch.float32).unsqueeze(1) * 0.5 for lay in ls]
        visibility.composite(colors, alphas).sum().backward()
        torch.cuda.synchronize()
        return attr.grad.cpu().numpy()

    g1, g2 = grad(1), grad(2)
    assert (g1[0] == 0).all() and (g1[1] != 0).any()
    assert (g2[0] != 0).all() and np.isfinite(g2).all()
    # every pixel of the hidden triangle passes half of its colour's gradient on, through the half-transparent front one
    n_back = int((visibility.decode(visibility.layers(fs, 2, stream=stream())[1]).tri == 0).sum())
    assert n_back > 100 and abs(float(g2[0].sum()) - 3 * 0.25 * n_back) <= 1e-3 * n_back
    fs.close()
