"""-m gpu: srz_cube_prefilter and srz_cube_prefilter_grad against tests/prefilter_ref.c's binary32 build, BIT FOR BIT: dst, den and
gsrc.  Every output starts as support.SENTINEL words, so a word the device did not write shows.  The sizes are the smallest that
take every path: one texel, odd and even sizes, more output than source and the reverse, 9600 source texels (a tail behind every
power-of-two tile), and — by the thresholds of csrc/srz_device.h's prefilter_chunks — a walk cut into rows (every small call), into
faces (16 -> 16 at 9 channels and 6 frames) and not cut at all (64 channels and 86 frames of an 8 x 8 cube)."""
import numpy as np
import pytest
import torch

import prefilterref as P
from support import SENTINEL, ctx, filled, stream, words  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 3), (2, 5), (3, 8), (8, 8), (5, 2), (40, 6), (32, 16)]
# (n_src, n_dst, kind, roughness, cmin, n_ch, frames)
CASES = [(s, d, P.GGX, 0.3, 0.0, 3, 1) for s, d in SIZES]
CASES += [(s, d, P.COSINE, 1.0, 0.0, 3, 1) for s, d in SIZES]
CASES += [(8, 8, P.GGX, r, 0.0, 3, 1) for r in (0.0, 0.0625, 1.0)]
CASES += [(8, 8, P.GGX, 0.3, 0.5, 3, 1), (8, 8, P.COSINE, 1.0, 0.5, 3, 1), (40, 6, P.GGX, 0.0625, 0.5, 3, 1)]
CASES += [(s, d, k, r, c, 3, 1) for s, d, k, r, c in P.EMPTY_CASES]
CASES += [(3, 8, P.GGX, 0.3, 0.0, 1, 1), (8, 8, P.COSINE, 1.0, 0.0, 5, 1), (5, 2, P.GGX, 0.3, 0.0, 5, 2), (8, 8, P.GGX, 0.3, 0.5, 9, 2)]
CASES += [(16, 16, P.GGX, 0.3, 0.0, 9, 6)]                                        # the walk cut into faces, both ways
CASES += [(1, 8, P.GGX, 0.3, 0.0, 64, 86), (8, 1, P.COSINE, 1.0, 0.0, 64, 86)]    # not cut: the forward, the backward


def case_id(c):
    return "{}to{}-{}-r{}-c{}-ch{}-f{}".format(c[0], c[1], "ggx" if c[2] == P.GGX else "cos", *c[3:])


def same_words(got, ref, what):
    """the words are equal; where the reference has a NaN the device has one (its sign and payload are the hardware's own)"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN at other places, {int((np.isnan(got) != nan).sum())} words"
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~nan
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ, first {np.argwhere(bad)[:3].tolist()}: got {got[bad][:3]} want {ref[bad][:3]}"


def device_forward(ctx, cube, n_dst, kind, r, cmin, want_den=True):
    """→ (dst, den or None) as numpy float32, from sentinel-filled buffers"""
    frames, n_src, n_ch = P._dims(cube)
    src = torch.as_tensor(np.ascontiguousarray(cube, np.float32)).cuda()
    dst, den = filled(cube.shape[:-3] + (n_dst, n_dst, n_ch)), filled((6, n_dst, n_dst))
    nbytes = ctx.cube_prefilter_work_bytes(n_src, n_dst, n_ch, frames)
    work = filled((nbytes // 4,))
    ctx.cube_prefilter(src.data_ptr(), n_src, dst.data_ptr(), n_dst, n_ch, frames, kind, r, cmin, den.data_ptr() if want_den else None,
                       work.data_ptr(), nbytes, stream())
    torch.cuda.synchronize()
    assert not (words(dst) == SENTINEL).any(), "a word of dst was not written"
    if want_den:
        assert not (words(den) == SENTINEL).any(), "a word of den was not written"
    else:
        assert (words(den) == SENTINEL).all()
    return words(dst).view(np.float32), (words(den).view(np.float32) if want_den else None)


def device_grad(ctx, gdst, den, n_src, kind, r, cmin):
    frames, n_dst, n_ch = P._dims(gdst)
    g, d = torch.as_tensor(np.ascontiguousarray(gdst, np.float32)).cuda(), torch.as_tensor(np.ascontiguousarray(den, np.float32)).cuda()
    gsrc = filled(gdst.shape[:-3] + (n_src, n_src, n_ch))
    nbytes = ctx.cube_prefilter_work_bytes(n_src, n_dst, n_ch, frames)
    work = filled((nbytes // 4,))
    ctx.cube_prefilter_grad(g.data_ptr(), d.data_ptr(), n_src, n_dst, n_ch, frames, kind, r, cmin, gsrc.data_ptr(), work.data_ptr(), nbytes, stream())
    torch.cuda.synchronize()
    assert not (words(gsrc) == SENTINEL).any(), "a word of gsrc was not written"
    return words(gsrc).view(np.float32)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_forward_and_backward_match_the_reference_bit_for_bit(ctx, tmp_path, case):  # noqa: F811
    n_src, n_dst, kind, r, cmin, n_ch, frames = case
    rng = np.random.default_rng([n_src, n_dst, n_ch, frames])
    shape = ((frames,) if frames > 1 else ()) + (6,)
    cube = rng.uniform(-0.25, 1.0, shape + (n_src, n_src, n_ch)).astype(np.float32)
    gdst = rng.uniform(-1.0, 1.0, shape + (n_dst, n_dst, n_ch)).astype(np.float32)
    ref_dst, ref_den, count = P.forward(tmp_path, cube, n_dst, kind, r, cmin)
    ref_gsrc = P.grad(tmp_path, gdst, ref_den, n_src, kind, r, cmin)
    dst, den = device_forward(ctx, cube, n_dst, kind, r, cmin)
    print(f"{case_id(case)}: {int(count.sum())} pairs taken of {count.size * 6 * n_src * n_src}, {int((count == 0).sum())} empty outputs")
    same_words(den, ref_den, "den")
    same_words(dst, ref_dst, "dst")
    same_words(device_grad(ctx, gdst, ref_den, n_src, kind, r, cmin), ref_gsrc, "gsrc")


@pytest.mark.parametrize("cmin", [0.0, 0.5])
@pytest.mark.parametrize("kind,r", [(P.COSINE, 1.0), (P.GGX, 0.3)])
def test_a_hostile_cube(ctx, tmp_path, kind, r, cmin):  # noqa: F811
    """+inf, -inf, NaN, subnormals and 3e38 at seeded texels (and in the gradient): the reference decides which outputs are finite — a
    skipped pair that was multiplied by zero instead would spread a NaN behind the cutoff — and the device matches its words"""
    rng = np.random.default_rng(11)
    cube, gdst = P.hostile_cube(rng, (6, 8, 8, 3)), P.hostile_cube(rng, (6, 8, 8, 3))
    ref_dst, ref_den, _ = P.forward(tmp_path, cube, 8, kind, r, cmin)
    ref_gsrc = P.grad(tmp_path, gdst, ref_den, 8, kind, r, cmin)
    finite = np.isfinite(ref_dst).all(-1)
    print(f"cmin {cmin}: {int(finite.sum())} of {finite.size} output texels finite, {int(np.isfinite(ref_gsrc).all(-1).sum())} source gradients")
    assert cmin == 0.0 or (finite.any() and not finite.all())  # (the cutoff keeps the hostile texels away from some outputs only)
    dst, den = device_forward(ctx, cube, 8, kind, r, cmin)
    same_words(den, ref_den, "den")
    same_words(dst, ref_dst, "dst")
    same_words(device_grad(ctx, gdst, ref_den, 8, kind, r, cmin), ref_gsrc, "gsrc")


def test_den_is_optional_and_a_call_repeats_its_words(ctx):  # noqa: F811
    rng = np.random.default_rng(12)
    cube = rng.uniform(0, 1, (2, 6, 5, 5, 5)).astype(np.float32)
    gdst = rng.uniform(-1, 1, (2, 6, 8, 8, 5)).astype(np.float32)
    dst, den = device_forward(ctx, cube, 8, P.GGX, 0.3, 0.5)
    dst0, _ = device_forward(ctx, cube, 8, P.GGX, 0.3, 0.5, want_den=False)
    dst1, den1 = device_forward(ctx, cube, 8, P.GGX, 0.3, 0.5)
    assert np.array_equal(dst.view(np.uint32), dst0.view(np.uint32)) and np.array_equal(dst.view(np.uint32), dst1.view(np.uint32))
    assert np.array_equal(den.view(np.uint32), den1.view(np.uint32))
    g0, g1 = device_grad(ctx, gdst, den, 5, P.GGX, 0.3, 0.5), device_grad(ctx, gdst, den, 5, P.GGX, 0.3, 0.5)
    assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
