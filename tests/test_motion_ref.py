"""not-gpu: the motion pass's test reference (tests/motion_ref.c through tests/motionref.py) pinned to the unchanged CPU oracle, to
float64 arithmetic and to its own stated rules.

Owners, classes, alpha, beta and z of a frame come from visref.Reference.expected (the oracle's render, decoded).  x' and y' as float32
are read through the z slot (motionref.rotated): the reference interpolates the three components by one statement."""
import numpy as np
import pytest

import motionref
from srz import abi
from support import frame, frame_positions, hostile_shading_frame, soup, stack, visibility_of

ZS = np.float32([1, 2, 3, 4])
INF = motionref.INF_WORD
FRAMES = {"soup 0": lambda: frame(soup(0, 90, 64, 64, ZS), 64, 64), "stack 200": lambda: stack(200),
          "wide and thin": lambda: hostile_shading_frame(0, "uv-edge", tame=True)}


def grid(shape):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return x.astype(np.float32), y.astype(np.float32)


def f32(words):
    return np.ascontiguousarray(words).view(np.float32)


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_anchor_the_frame_is_its_own_target(tmp_path, orc, name):
    """delta == 0: DEPTH is the oracle's z plane bit for bit, TARGET the pixel's own id and z, at every owned pixel"""
    f = FRAMES[name]()
    v = visibility_of(tmp_path, orc, f)
    words, own = v.words, v.own
    out = motionref.expected(tmp_path, frame_positions(f), words, words)
    assert np.array_equal(out[2][own], words[0][own]), "z' differs from the oracle's z"
    dx, dy = f32(out[0]), f32(out[1])
    worst = max(float(np.abs(dx[own]).max()), float(np.abs(dy[own]).max()))
    print(f"max |flow| at delta 0: {worst:.3g}")
    assert worst < 0.5
    assert np.array_equal(out[3][own], words[1][own]) and np.array_equal(out[4][own], words[0][own])
    assert (out[:, ~own] == 0).all()


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_arithmetic_against_float64(tmp_path, orc, name):
    """a random moved copy of the frame: x', y', z' within 3 * 2^-24 * S, S = |alpha a| + |beta b| + |gamma c|, of the same sum of three
    products in float64 from the float32 alpha, beta, gamma.  V: three roundings (the product gamma c, two fmas), each of a value of
    magnitude <= S.  S: the three products' roundings add up to 2^-24 * S, the first sum's is <= 2^-24 * (|alpha a| + |beta b|), the
    second's <= 2^-24 * S — the same 3 * 2^-24 * S.  dx, dy are the float32 differences x' - x, y' - y bit for bit."""
    f = FRAMES[name]()
    v = visibility_of(tmp_path, orc, f)
    words, own, s_class = v.words, v.own, v.s_class
    rng = np.random.default_rng(7)
    pos = frame_positions(f).reshape(-1, 3, 3)
    moved = (pos + rng.normal(0, 6, pos.shape) + rng.normal(0, 10, (1, 1, 3))).astype(np.float32).reshape(-1, 9)
    out = motionref.expected(tmp_path, moved, words, words)
    al, be = f32(words[2]), f32(words[3])
    one = np.float32(1)
    ga = np.where(s_class, (one - al) - be, one - (al + be)).astype(np.float32)
    idx = np.where(own, (words[1] & 0x7fffffff).astype(np.int64) - 1, 0)
    tri = moved.reshape(-1, 3, 3).astype(np.float64)[idx]  # [H, W, vertex, component]
    x, y = grid(own.shape)
    got = {2: f32(out[2])}
    for c in (0, 1):
        got[c] = f32(motionref.expected(tmp_path, motionref.rotated(moved, c), words, words)[2])
    for c in (0, 1, 2):
        terms = [al.astype(np.float64) * tri[..., 0, c], be.astype(np.float64) * tri[..., 1, c], ga.astype(np.float64) * tri[..., 2, c]]
        exact = terms[0] + terms[1] + terms[2]
        bound = 3 * 2.0 ** -24 * (abs(terms[0]) + abs(terms[1]) + abs(terms[2]))
        err = np.abs(got[c].astype(np.float64) - exact)
        print(f"component {c}: max error / bound = {float((err[own] / bound[own]).max()):.3f}")
        assert (err[own] <= bound[own]).all(), c
    assert np.array_equal(out[0][own], (got[0] - x).view(np.uint32)[own]) and np.array_equal(out[1][own], (got[1] - y).view(np.uint32)[own])


def test_translation_lands_on_the_moved_pixel(tmp_path, orc):
    """the target frame is the frame moved by an integer (k, m) = (5, -3), z + 1 (motionref.translation_frames states why alpha and
    beta, coverage and class are then the same bits at (x + k, y + m)): for EVERY owned pixel rint lands on (x + k, y + m), tid is the
    pixel's own id word, class bit included, tz is the moved frame's z there, and z' = tz bit for bit"""
    k, m, _ = motionref.TRANSLATION
    f0, f1 = motionref.translation_frames()
    v0, v1 = visibility_of(tmp_path, orc, f0), visibility_of(tmp_path, orc, f1)
    w0, own0, amb0, w1, own1, amb1 = v0.words, v0.own, v0.amb, v1.words, v1.own, v1.amb
    assert amb0 == 0 and amb1 == 0  # (the oracle's colours decode to one owner at every pixel of both frames: no pixel is left out)
    out = motionref.expected(tmp_path, frame_positions(f1), w0, w1)
    dx, dy = f32(out[0]), f32(out[1])
    assert (np.abs(dx[own0] - k) < 0.5).all() and (np.abs(dy[own0] - m) < 0.5).all()  # (4.5 and 5.5 are floats: rint(x') == x + k)
    ys, xs = np.nonzero(own0)
    assert np.array_equal(out[3][own0], w0[1][own0]), "tid is not the pixel's own id word"
    assert np.array_equal(out[3][own0], w1[1][ys + m, xs + k]) and np.array_equal(out[4][own0], w1[0][ys + m, xs + k])
    assert np.array_equal(out[2][own0], out[4][own0])  # visible there: the interpolated depth IS the target's z
    assert np.array_equal(own1[ys + m, xs + k], np.ones(len(ys), bool)) and own0.sum() == own1.sum()


def hostile_case(tmp_path, orc):
    f = frame(soup(4, 300, 70, 50, ZS), 70, 50)
    v = visibility_of(tmp_path, orc, f)
    words, own, s_class = v.words, v.own, v.s_class
    pos = motionref.hostile_target_positions(frame_positions(f), 70, 50)
    return f, words, own, s_class, pos


def test_hostile_targets(tmp_path, orc):
    """target positions NaN, +-inf, +-1e30 and at / one ulp around -0.5, W - 0.5, H - 0.5: the rule restated in numpy from x', y' (read
    through the z slot) gives the reference's target words; outside is (0, +inf); the flow is NaN exactly where the sum is; and the
    same source under AddressSanitizer + UBSan (float-cast-overflow) gives the same words without a report: no index is formed from
    a coordinate outside the image"""
    f, words, own, _, pos = hostile_case(tmp_path, orc)
    H, W = own.shape
    out = motionref.expected(tmp_path, pos, words, words)
    xp = f32(motionref.expected(tmp_path, motionref.rotated(pos, 0), words, words)[2])
    yp = f32(motionref.expected(tmp_path, motionref.rotated(pos, 1), words, words)[2])
    with np.errstate(invalid="ignore"):
        tx, ty = np.rint(xp), np.rint(yp)
        inside = own & (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
    outside = own & ~inside
    xi, yi = np.where(inside, tx, 0).astype(np.int64), np.where(inside, ty, 0).astype(np.int64)
    assert np.array_equal(out[3][inside], words[1][yi, xi][inside]) and np.array_equal(out[4][inside], words[0][yi, xi][inside])
    assert (out[3][outside] == 0).all() and (out[4][outside] == INF).all()
    assert np.array_equal(np.isnan(f32(out[0]))[own], np.isnan(xp)[own]) and np.array_equal(np.isnan(f32(out[1]))[own], np.isnan(yp)[own])
    # every kind is there: NaN, +-inf and huge sums, and both sides of each border
    n_nan, n_inf = int((own & (np.isnan(xp) | np.isnan(yp))).sum()), int((own & (np.isinf(xp) | np.isinf(yp))).sum())
    with np.errstate(invalid="ignore"):
        n_huge = int((own & ((np.abs(xp) > 1e29) | (np.abs(yp) > 1e29)) & np.isfinite(xp) & np.isfinite(yp)).sum())
        near = {name: (int((own & (v == lo)).sum()), int((own & (v == hi)).sum()))
                for name, v, lo, hi in (("left", tx, -1, 0), ("right", tx, W - 1, W), ("top", ty, -1, 0), ("bottom", ty, H - 1, H))}
    print(f"inside {int(inside.sum())} outside {int(outside.sum())} nan {n_nan} inf {n_inf} huge {n_huge} borders {near}")
    assert inside.sum() > 200 and outside.sum() > 200 and n_nan > 20 and n_inf > 20 and n_huge > 20
    assert all(a > 0 and b > 0 for a, b in near.values()), near
    san = motionref.expected_sanitized(tmp_path, pos, words, words)
    nan_a, nan_b = np.isnan(f32(out)), np.isnan(f32(san))
    assert np.array_equal(nan_a, nan_b) and np.array_equal(out[~nan_a], san[~nan_a])


def test_nobody_and_out_of_range_ids(tmp_path):
    """id 0, the bare class bit and an index past the triangles are nobody: zeros when fused, untouched otherwise"""
    f = frame(soup(1, 5, 8, 8, ZS), 8, 8)
    words = np.zeros((4, 1, 6), np.uint32)
    words[1, 0] = [0, 0x80000000, 6, 0x7fffffff, 0xffffffff, 1]
    words[2:, 0] = np.float32(0.25).view(np.uint32)
    pre = np.full((5, 1, 6), 0xdeadbeef, np.uint32)
    fused = motionref.expected(tmp_path, frame_positions(f), words, words, fused=True, prefill=pre)
    kept = motionref.expected(tmp_path, frame_positions(f), words, words, fused=False, prefill=pre)
    assert (fused[:, 0, :5] == 0).all() and (kept[:, 0, :5] == 0xdeadbeef).all()
    assert np.array_equal(fused[:, 0, 5], kept[:, 0, 5]) and not (fused[:3, 0, 5] == 0xdeadbeef).any()
    assert (motionref.nobody((1, 6)) == 0).all() and (motionref.nobody((1, 6), False, 7) == 7).all()


def test_plane_order_of_all_7_masks():
    from srz.visibility import motion_planes
    groups = ((abi.MV_FLOW, ["dx", "dy"]), (abi.MV_DEPTH, ["depth"]), (abi.MV_TARGET, ["target_id", "target_z"]))
    assert (abi.MV_FLOW, abi.MV_DEPTH, abi.MV_TARGET, abi.MV_ALL) == (1, 2, 4, 7)
    for what in range(1, 8):
        want = [n for bit, names in groups if what & bit for n in names]
        assert list(motion_planes(what)) == want and len(want) == len(motionref.planes_of(what)), what
    for bad in (0, 8, 15):
        with pytest.raises(ValueError):
            motion_planes(bad)


def test_decode_returns_views():
    import torch
    from srz.visibility import motion_decode
    buf = torch.arange(2 * 5 * 3 * 4, dtype=torch.int32).reshape(2, 5, 3, 4)
    buf[:, 3] = torch.tensor([0, 1, -(1 << 31) | 3, 7])  # nobody / outside; V owner 0; S owner 2; V owner 6
    m = motion_decode(buf, abi.MV_ALL)
    assert m["flow"].shape == (2, 2, 3, 4) and m["depth"].shape == (2, 3, 4) and m["target_z"].shape == (2, 3, 4)
    assert m["target_index"][0, 0].tolist() == [-1, 0, 2, 6] and m["target_s_class"][1, 2].tolist() == [False, False, True, False]
    for key, first in (("flow", 0), ("depth", 2), ("target_z", 4)):
        assert m[key].dtype == torch.float32 and m[key].data_ptr() == buf[:, first:].data_ptr()  # a view: no copy
    part = motion_decode(buf[:, :3], abi.MV_DEPTH | abi.MV_TARGET)
    assert set(part) == {"depth", "target_index", "target_s_class", "target_z"} and part["depth"].data_ptr() == buf.data_ptr()
    with pytest.raises(ValueError):
        motion_decode(buf, abi.MV_FLOW)
