"""not-gpu: the attribute interpolation's test reference (tests/interp_ref.c through tests/interpref.py) pinned on the oracle's
visibility buffers (visref.Reference.expected), for scenes in which both classes occur: to the G-buffer reference's uv planes, to the
buffer's own z plane, and, backward, to numpy restatements in float64."""
import numpy as np
import pytest

import gbufref
import interpref
from support import bits, frame, hostile_shading_frame, soup, visibility_of

ZS = np.float32([1, 2, 3, 4])
FRAMES = {"soup 0": lambda: frame(soup(0, 90, 64, 64, ZS), 64, 64), "soup 3 (quarter-pixel vertices)": lambda: frame(soup(3, 90, 64, 64, ZS), 64, 64),
          "wide and thin": lambda: hostile_shading_frame(0, "uv-edge", tame=True)}


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_uv_as_attributes_is_the_gbuffers_uv(tmp_path, orc, name):
    f = FRAMES[name]()
    v = visibility_of(tmp_path, orc, f)
    words, own, n = v.words, v.own, v.n
    got = interpref.forward(tmp_path, interpref.frame_attr(f, "uv"), n, words)
    want = gbufref.expected(tmp_path, f, {}, words)[3:5]
    assert got.shape == (2, f.height, f.width) and np.array_equal(bits(got), want)
    assert (bits(got)[:, ~own] == 0).all() and (got[:, own] != 0).any()


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_positions_as_attributes_give_the_buffers_depth(tmp_path, orc, name):
    """motion's delta-0 rule: z interpolates like every attribute, so channel 2 of the positions is plane 0 at every owned pixel"""
    f = FRAMES[name]()
    v = visibility_of(tmp_path, orc, f)
    words, own, n = v.words, v.own, v.n
    pre = np.full((3, f.height, f.width), 0xdeadbeef, np.uint32)
    got = bits(interpref.forward(tmp_path, interpref.frame_attr(f, "pos"), n, words, fused=False, prefill=pre))
    assert np.array_equal(got[2][own], words[0][own])
    assert (got[:, ~own] == 0xdeadbeef).all() and (got[:, own] != 0xdeadbeef).all()


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_backward_against_numpy_in_float64(tmp_path, orc, name):
    f = FRAMES[name]()
    v = visibility_of(tmp_path, orc, f)
    words, own, s_class, n = v.words, v.own, v.s_class, v.n
    rng = np.random.default_rng(7)
    H, W = f.height, f.width
    # ---- gbary at one channel: RN(g * RN(a - c)), the product exact in float64 (24 x 24 bits)
    attr1 = rng.normal(0, 3, (n + 2, 3, 1)).astype(np.float32)
    g1 = rng.normal(0, 2, (1, H, W)).astype(np.float32)
    gb = interpref.grad(tmp_path, attr1, n, words, g1)
    tri = (words[1] & 0x7fffffff).astype(np.int64) - 1
    t = np.where(own, tri, 0)
    for plane, corner in ((0, 0), (1, 1)):
        diff = attr1[t, corner, 0] - attr1[t, 2, 0]
        assert diff.dtype == np.float32
        want = (g1[0].astype(np.float64) * diff.astype(np.float64)).astype(np.float32) + np.float32(0)
        assert np.array_equal(bits(gb[plane])[own], bits(want)[own]) and (gb[plane][~own] == 0).all()
    # ---- gattr in double against np.add.at in float64 on the float32 products
    C = 5
    attr = rng.normal(0, 3, (n + 2, 3, C)).astype(np.float32)
    gout = rng.normal(0, 2, (C, H, W)).astype(np.float32)
    gout[:, ~own] = np.nan  # never read
    acc = interpref.Grad(attr.shape)
    interpref.grad(tmp_path, attr, n, words, gout, into=acc, want_bary=False)
    al, be = words[2].view(np.float32), words[3].view(np.float32)
    one = np.float32(1)
    ga = np.where(s_class, (one - al) - be, one - (al + be))
    assert ga.dtype == np.float32
    want, count = np.zeros(attr.shape, np.float64), np.zeros(len(attr), np.int64)
    ys, xs = np.nonzero(own)
    for k, w in enumerate((al, be, ga)):
        for c in range(C):
            prod = w[ys, xs] * gout[c, ys, xs]
            assert prod.dtype == np.float32
            np.add.at(want[:, k, c], tri[ys, xs], prod.astype(np.float64))
    np.add.at(count, tri[ys, xs], 1)
    assert np.isfinite(acc.gattr).all() and np.array_equal(acc.count, count)
    assert np.allclose(acc.gattr, want, rtol=1e-12, atol=1e-12) and (acc.gattr[n:] == 0).all() and (acc.bound() >= 0).all()
    assert (acc.gattr != 0).sum() > 100
