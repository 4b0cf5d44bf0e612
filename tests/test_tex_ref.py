"""not-gpu: the texture pass's test reference (tests/tex_ref.c through tests/texref.py) pinned: hand-computed samples, central
differences of a float64 restatement in numpy, torch's grid_sample as a second opinion, and — on the oracle's visibility buffers of
the very frames tests/test_gpu_texture.py renders — the conditions that keep those tests from passing vacuously."""
import numpy as np
import pytest

import interpref
import texref
from support import bits, visibility_of
from texref import CLAMP, WRAP

ONE = np.ones((1, 1), np.uint32)  # one pixel, owned by triangle 0


def sample(tmp_path, tex, mode, u, v):
    """one owned pixel at (u, v) → (out [C], guv [2] for gout = 1 on every channel, Grad)"""
    tex = np.asarray(tex, np.float32)
    uv = np.float32([[[u]], [[v]]])
    out = texref.forward(tmp_path, tex, mode, 1, ONE, uv)
    acc = texref.Grad(tex.shape)
    guv = texref.grad(tmp_path, tex, mode, 1, ONE, uv, np.ones((tex.shape[2], 1, 1), np.float32), into=acc)
    return out[:, 0, 0], guv[:, 0, 0], acc


T22 = np.float32([[[1.0], [2.0]], [[4.0], [8.0]]])  # [2, 2, 1]: rows y, columns x


# ------------------------------------------------------------------------------------------------------ hand KATs
@pytest.mark.parametrize("mode", [CLAMP, WRAP])
def test_texel_centres_return_the_texels_and_the_midpoint_their_mean(tmp_path, mode):
    for y in (0, 1):
        for x in (0, 1):
            out, _, acc = sample(tmp_path, T22, mode, (x + 0.5) / 2, (y + 0.5) / 2)
            assert out[0] == T22[y, x, 0]
            assert acc.gtex[y, x, 0] == 1.0 and acc.gtex.sum() == 1.0 and acc.count.sum() == 4  # four adds, three of weight 0
    out, guv, acc = sample(tmp_path, T22, mode, 0.5, 0.5)
    assert out[0] == 3.75 and (acc.gtex == 0.25).all() and (acc.count == 1).all()
    # d/du = ((2 - 1) + 0.5 * ((8 - 4) - (2 - 1))) * W = 2.5 * 2, d/dv = (bot - top) * H = (6 - 1.5) * 2
    assert guv[0] == 5.0 and guv[1] == 9.0
    out, guv, _ = sample(tmp_path, T22, mode, 0.375, 0.625)  # fx = 0.25, fy = 0.75: dyadic weights
    top, bot = 1.0 + 0.25 * 1.0, 4.0 + 0.25 * 4.0
    assert out[0] == top + 0.75 * (bot - top) and guv[0] == (1.0 + 0.75 * 3.0) * 2 and guv[1] == (bot - top) * 2


@pytest.mark.parametrize("mode", [CLAMP, WRAP])
def test_one_texel_textures(tmp_path, mode):
    tex = np.float32([[[5.0, -2.0, 0.5]]])
    for u, v in ((0.5, 0.5), (0.0, 1.0), (-3.25, 7.75), (1e6, -1e6), (3e38, -3e38), (0.999, 1e-30)):
        out, guv, acc = sample(tmp_path, tex, mode, u, v)
        assert np.array_equal(out, tex[0, 0]) and (guv == 0).all()
        assert acc.count[0, 0] == 4 and np.allclose(acc.gtex[0, 0], 1.0, rtol=0, atol=2 ** -22)  # the four corners coincide: all add
    wide = np.float32([[[1.0], [3.0], [7.0]]])  # 3 x 1: v never matters
    for v in (0.0, 0.5, 12.5):
        out, guv, _ = sample(tmp_path, wide, mode, 0.5, v)
        assert out[0] == 3.0 and guv[1] == 0.0 and guv[0] == 12.0  # tx = 0 at texel 1: the slope is the one to texel 2, (7 - 3) * W


def test_clamp_at_and_beyond_both_borders(tmp_path):
    for u, x in ((0.25, 0), (0.0, 0), (-0.0, 0), (-5.0, 0), (-3e38, 0), (0.75, 1), (1.0, 1), (9.0, 1), (3e38, 1)):
        out, guv, acc = sample(tmp_path, T22, CLAMP, u, 0.25)
        assert out[0] == T22[0, x, 0], u
        assert guv[0] == 0.0, u  # in_x is false at and beyond the border texels' centres: du is zero
        assert acc.gtex[0, x, 0] == 1.0 and acc.gtex.sum() == 1.0
    out, guv, _ = sample(tmp_path, T22, CLAMP, 0.5, 0.25)  # inside in x; v on the first row's centre: in_y false (fy = 0)
    assert out[0] == 1.5 and guv[0] == 2.0 and guv[1] == 0.0
    out, guv, _ = sample(tmp_path, T22, CLAMP, 0.5, 0.26)
    assert guv[1] != 0.0
    for v, y in ((-1.0, 0), (0.2, 0), (0.8, 1), (4.0, 1)):
        out, guv, _ = sample(tmp_path, T22, CLAMP, 0.25, v)
        assert out[0] == T22[y, 0, 0] and guv[1] == 0.0


def test_the_wrap_seam(tmp_path):
    tex = np.float32([[[1.0], [2.0], [4.0], [8.0]]])  # 4 x 1
    # u slightly below 0 rounds to a fraction of exactly 1: fx = 3.5, between texel 3 and texel 0 (x1 wrapped)
    out, guv, acc = sample(tmp_path, tex, WRAP, -1e-9, 0.5)
    assert out[0] == 4.5 and acc.gtex[0, 3, 0] == 0.5 and acc.gtex[0, 0, 0] == 0.5 and guv[0] == (1.0 - 8.0) * 4
    # u = 1 exactly has fraction 0: fx = -0.5, between texel -1 = 3 (x0 wrapped) and texel 0
    out1, guv1, acc1 = sample(tmp_path, tex, WRAP, 1.0, 0.5)
    assert out1[0] == 4.5 and acc1.gtex[0, 3, 0] == 0.5 and acc1.gtex[0, 0, 0] == 0.5 and guv1[0] == guv[0]
    for u in (0.0, 2.0, -7.0):
        assert sample(tmp_path, tex, WRAP, u, 0.5)[0][0] == 4.5
    # periods: u and u + k sample alike where the sum is exact
    for u in (0.125, 0.375, 0.8125):
        a = sample(tmp_path, tex, WRAP, u, 0.5)
        for k in (1.0, -1.0, 16.0, -4.0):
            b = sample(tmp_path, tex, WRAP, u + k, 0.5)
            assert a[0][0] == b[0][0] and a[1][0] == b[1][0], (u, k)
    assert sample(tmp_path, tex, WRAP, 3e38, -3e38)[0][0] == 4.5  # floorf(u) == u: the fraction is 0
    cls = texref.classify(tmp_path, (1, 4), WRAP, 1, ONE, np.float32([[[-1e-9]], [[0.5]]]))
    assert cls[0, 0] == texref.OWNED | texref.SAMPLED | texref.WRAPPED  # (y1 of a one-row texture wraps too)


@pytest.mark.parametrize("mode", [CLAMP, WRAP])
def test_non_finite_uv_is_not_sampled(tmp_path, mode):
    tex = texref.make_tex(1, 5, 7, 3)
    for u, v in ((np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (0.5, -np.inf), (-np.inf, np.inf), (np.nan, np.nan)):
        uv = np.float32([[[u]], [[v]]])
        pre = np.full((3, 1, 1), 0xdeadbeef, np.uint32)
        out = texref.forward(tmp_path, tex, mode, 1, ONE, uv, fused=False, prefill=pre)
        assert (bits(out) == 0).all()  # written: the pixel has an owner
        acc = texref.Grad(tex.shape)
        guv = texref.grad(tmp_path, tex, mode, 1, ONE, uv, np.ones((3, 1, 1), np.float32), into=acc, fused=False, prefill=np.full((2, 1, 1), 0xdeadbeef, np.uint32))
        assert (bits(guv) == 0).all() and acc.count.sum() == 0 and (acc.gtex == 0).all()
        assert texref.classify(tmp_path, (7, 5), mode, 1, ONE, uv)[0, 0] == texref.OWNED
    out, guv, acc = sample(tmp_path, tex, mode, 3e38, -3e38)  # finite: sampled
    assert np.isfinite(out).all() and acc.count.sum() == 4
    # nobody's pixel: untouched without the fused clear, zero with it
    nobody = np.zeros((1, 1), np.uint32)
    pre = np.full((3, 1, 1), 0xdeadbeef, np.uint32)
    assert (bits(texref.forward(tmp_path, tex, mode, 1, nobody, np.float32([[[0.5]], [[0.5]]]), fused=False, prefill=pre)) == 0xdeadbeef).all()
    assert (bits(texref.forward(tmp_path, tex, mode, 1, nobody, np.float32([[[0.5]], [[0.5]]]), fused=True, prefill=pre)) == 0).all()
    assert (bits(texref.forward(tmp_path, tex, mode, 1, ONE * 2, np.float32([[[0.5]], [[0.5]]]), fused=False, prefill=pre)) == 0xdeadbeef).all()  # id 2 of 1 triangle


# ------------------------------------------------------------------------------------------------------ float64 restatement
def np_sample(tex, mode, u, v):
    """the rule in numpy float64, vectorised over u, v [n] → [n, C]"""
    tex = tex.astype(np.float64)
    H, W, _ = tex.shape

    def axis(c, n):
        if mode == WRAP:
            c = c - np.floor(c)
        f = c * n - 0.5
        if mode == CLAMP:
            f = np.clip(f, 0.0, n - 1.0)
        i0 = np.floor(f)
        t = f - i0
        i0 = i0.astype(np.int64)
        i1 = i0 + 1
        if mode == CLAMP:
            i1 = np.minimum(i1, n - 1)
        else:
            i0, i1 = i0 % n, i1 % n
        return i0, i1, t
    x0, x1, tx = axis(np.asarray(u, np.float64), W)
    y0, y1, ty = axis(np.asarray(v, np.float64), H)
    top = tex[y0, x0] + tx[:, None] * (tex[y0, x1] - tex[y0, x0])
    bot = tex[y1, x0] + tx[:, None] * (tex[y1, x1] - tex[y1, x0])
    return top + ty[:, None] * (bot - top)


@pytest.mark.parametrize("mode", [CLAMP, WRAP])
@pytest.mark.parametrize("w,h", [(5, 7), (2, 2), (33, 1), (64, 64)])
def test_gradients_against_central_differences_in_float64(tmp_path, mode, w, h):
    """guv and gtex of the reference against central differences of np_sample, at points at least 0.05 texels away from a texel
    centre line (where the bilinear surface has its kinks) and, in CLAMP mode, inside the border centres or at least 0.05 beyond"""
    rng = np.random.default_rng([w, h, mode])
    C, n = 3, 400
    tex = texref.make_tex(2, w, h, C)
    lo, hi = (-0.3, 1.3) if mode == CLAMP else (-2.0, 3.0)
    u, v = rng.uniform(lo, hi, 4 * n).astype(np.float32), rng.uniform(lo, hi, 4 * n).astype(np.float32)

    def away(c, size):
        f = c.astype(np.float64) * size - 0.5
        return np.abs(f - np.rint(f)) > 0.05
    keep = away(u, w) & away(v, h)
    u, v = u[keep][:n], v[keep][:n]
    assert len(u) == n
    ids = np.ones((1, n), np.uint32)
    uv = np.stack([u, v])[:, None, :]
    gout = rng.normal(0, 1, (C, 1, n)).astype(np.float32)
    out = texref.forward(tmp_path, tex, mode, 1, ids, uv)[:, 0].T
    want = np_sample(tex, mode, u, v)
    scale = np.abs(tex).max()
    # (the float32 texel coordinate is off by up to an ulp of max(w, h) or of 3 w: that share of a texel difference of up to 2 * scale)
    assert np.abs(out - want).max() <= 8 * 2.0 ** -22 * max(w, h) * scale
    acc = texref.Grad(tex.shape)
    guv = texref.grad(tmp_path, tex, mode, 1, ids, uv, gout, into=acc)[:, 0]
    g = gout[:, 0].T.astype(np.float64)
    eps = 1e-4 / max(w, h)
    du = ((np_sample(tex, mode, u.astype(np.float64) + eps, v) - np_sample(tex, mode, u.astype(np.float64) - eps, v)) * g).sum(1) / (2 * eps)
    dv = ((np_sample(tex, mode, u, v.astype(np.float64) + eps) - np_sample(tex, mode, u, v.astype(np.float64) - eps)) * g).sum(1) / (2 * eps)
    tol = 1e-4 * scale * max(w, h) * C
    assert np.abs(guv[0] - du).max() <= tol and np.abs(guv[1] - dv).max() <= tol, (np.abs(guv[0] - du).max(), np.abs(guv[1] - dv).max(), tol)
    assert (guv != 0).any() or (w == 1 and h == 1)
    # gtex: the loss sum(out * gout) is linear in the texels; its derivative to texel (y, x, c) by a unit bump
    loss = lambda t: (np_sample(t, mode, u, v) * g).sum()  # noqa: E731
    picks = [(int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(0, C))) for _ in range(12)]
    for (y, x, c) in picks:
        bump = tex.astype(np.float64).copy()
        bump[y, x, c] += 1.0
        assert abs((loss(bump) - loss(tex.astype(np.float64))) - acc.gtex[y, x, c]) <= 1e-4 * max(1.0, acc.gabs[y, x, c]), (y, x, c)
    assert acc.count.sum() == 4 * n and (acc.bound() >= 0).all()


# ------------------------------------------------------------------------------------------------------ second opinion
@pytest.mark.parametrize("w,h", [(5, 7), (2, 2), (33, 1), (64, 64), (1, 1)])
def test_second_opinion_grid_sample(tmp_path, w, h):
    """CLAMP mode with uv inside [0, 1] is torch.nn.functional.grid_sample(mode="bilinear", padding_mode="border",
    align_corners=False) at grid = 2 uv - 1, on the CPU.  Neither side is the code under test.  Measured over these five textures
    (values N(0, 3), 3 channels, 4096 points each): the largest |reference - grid_sample| is 1.407e-05 (on the 64 x 64 texture, where
    the roundings of the mapping ((g + 1) * W - 1) / 2 are worth the most texel fractions; 8.6e-06 at 33 x 1, 2.1e-06 at 5 x 7,
    9.5e-07 at 2 x 2, 0 at 1 x 1); the bound is four times that, 5.63e-05: the margin covers grid_sample's extra rounding in its
    coordinate mapping."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng([w, h, 3])
    n, C = 4096, 3
    tex = texref.make_tex(3, w, h, C)
    u, v = rng.uniform(0, 1, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
    u[:8], v[:8] = [0, 1, 0, 1, 0.5, 0.5, 0, 1], [0, 0, 1, 1, 0, 1, 0.5, 0.5]
    out = texref.forward(tmp_path, tex, CLAMP, 1, np.ones((1, n), np.uint32), np.stack([u, v])[:, None, :])[:, 0]
    grid = torch.as_tensor(np.stack([u, v], 1) * np.float32(2) - np.float32(1)).reshape(1, 1, n, 2)
    ref = F.grid_sample(torch.as_tensor(tex).permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0].numpy()
    d = float(np.abs(out - ref).max())
    print(f"grid_sample {w}x{h}: max |reference - grid_sample| = {d:.3e}")
    assert d <= 4 * 1.407e-05


# ------------------------------------------------------------------------------------------------------ the GPU tests' frames
@pytest.mark.parametrize("name", texref.FRAME_CASES)
def test_the_gpu_tests_frames_are_not_vacuous(tmp_path, orc, name):
    """on the oracle's visibility buffer of each frame tests/test_gpu_texture.py renders, with uv = interpolate of the frame's uv (the
    interpolation's reference): at least 200 sampled pixels; in CLAMP mode at least 20 pixels at or beyond the border centres (in_x
    or in_y false); in WRAP mode at least 20 whose x1 or y1 wrapped; in the non-finite case at least 20 pixels that have an owner
    and are not sampled.  The border conditions hold at every texture size but those texref.NO_BORDER lists: at least three sizes
    per frame and mode, and every size in both modes under some frame."""
    f = texref.case_frame(name)
    vis = visibility_of(tmp_path, orc, f)
    uv = interpref.forward(tmp_path, texref.frame_uv(f), vis.n, vis.words)
    for (w, h) in texref.TEX_SIZES:
        for mode in (CLAMP, WRAP):
            cls = texref.classify(tmp_path, (h, w), mode, vis.n, vis.words[1], uv)
            assert np.array_equal((cls & texref.OWNED) != 0, vis.own)
            sampled, outside, wrapped = (int(((cls & b) != 0).sum()) for b in (texref.SAMPLED, texref.OUTSIDE, texref.WRAPPED))
            unsampled = int(vis.own.sum()) - sampled
            print(f"{name} {w}x{h} mode {mode}: owned {int(vis.own.sum())} sampled {sampled} outside {outside} wrapped {wrapped} unsampled {unsampled}")
            assert sampled >= 200
            assert (wrapped == 0) if mode == CLAMP else (outside == 0)
            if (w, h) not in texref.NO_BORDER.get((name, mode), ()):
                assert (outside if mode == CLAMP else wrapped) >= 20
            if name in texref.NON_FINITE_CASES:
                assert unsampled >= 20
            else:
                assert unsampled == 0


def test_every_texture_size_meets_its_border_in_both_modes():
    for mode in (CLAMP, WRAP):
        for name in texref.FRAME_CASES:
            assert len(texref.TEX_SIZES) - len(texref.NO_BORDER.get((name, mode), ())) >= 3
        for size in texref.TEX_SIZES:
            assert any(size not in texref.NO_BORDER.get((name, mode), ()) for name in texref.FRAME_CASES)
