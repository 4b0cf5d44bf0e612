"""not-gpu: the oracle on hostile SHADING inputs — pinned before tests/test_gpu_shading_edges.py holds the kernels to it.

a. Known answers for the cases where the reference's behaviour is a property of its x86 build (float -> int conversions, the operand
   order of min / max with a NaN); each cites the reference's file and line (Liupeter01/Software-Rasterizer, as tests/test_oracle_kat.py).
b. Every family of support.hostile_shading_frame: the oracle returns 0, its colour planes hold no NaN, every covered colour lies in
   [0, 255], and the family REACHES ITS EDGE on the oracle — a family that does not is a broken generator, and the test says so.
c. The two comparison helpers refuse a NaN on one side only, in any plane.
d. The families under `make -C oracle asan`: the checker reads inside its buffers (and the textures' padded rows) on them."""
import os
import subprocess

import numpy as np
import pytest

from srz import abi
from support import (HOSTILE_EXPONENTS, HOSTILE_FAMILIES, HOSTILE_TEX, HOSTILE_TEX_SHAPES, TEXTURED, ccw, check_approx, compare, dump_frames,
                     frame, hostile_shading_frame, hostile_textures, oracle_with_probes, padded_rows, register_hostile_textures, tolerance_frames)

F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX = (abi.SHADER_TEXTURE, abi.SHADER_PHONG, abi.SHADER_BUMP, abi.SHADER_DISPLACEMENT, abi.SHADER_NORMAL)
SEEDS = (0, 1, 2, 3)
ALWAYS_FINITE = ("uv-edge", "uv-overflow", "exponent", "texture-shape")
ALWAYS_NONFINITE = ("uv-nonfinite", "normal-nonfinite")
BRIGHT = [((20, 20, 0), (1e4, 1e4, 1e4))]  # the ambient term alone (0.005 * 1e4) saturates: a pixel is 255 x (texel != 0)


@pytest.fixture(scope="module")
def horc(orc):
    register_hostile_textures(orc)
    return orc


def kat_tri(uv=0.5, nrm=(0, 0, 1)):
    """x 8..28: columns 8..23 are the 8-wide class (pixel (12, 9)), 24..28 the scalar tail (pixel (25, 9))"""
    t = ccw((8, 8), (28.5, 8), (8, 28.5), nrm=nrm)
    t["uv"][0] = uv
    return t


def rgb(pl, x, y):
    return [float(pl[c][y, x]) for c in (1, 2, 3)]


# ------------------------------------------------------------------------------------------------ a. known answers
def test_nan_uv_in_the_scalar_fetch_is_black(horc):
    """src/TextureLoader.cpp:16-27: glm::clamp keeps a NaN, static_cast<int>(NaN * width) is cvttss2si's 0x80000000 on x86, and
    `x < 0` returns {}: black.  (No byte of the texture is 0 and a tame uv gives 255, so black is the fetch's doing.)"""
    for uv in ([[np.nan, 0.5]] * 3, [[0.5, np.nan]] * 3, [[np.inf, 0.5], [-np.inf, 0.5], [0.5, 0.5]]):
        rc, pl, _ = horc.draw(frame(kat_tri(uv), shader=abi.SHADER_TEXTURE, tex=HOSTILE_TEX, lights=BRIGHT))
        assert rc == 0 and rgb(pl, 25, 9) == [0.0, 0.0, 0.0], uv
    rc, pl, _ = horc.draw(frame(kat_tri(0.5), shader=abi.SHADER_TEXTURE, tex=HOSTILE_TEX, lights=BRIGHT))
    assert rgb(pl, 25, 9) == [255.0, 255.0, 255.0]


def test_uv_one_in_the_scalar_fetch_is_black_and_the_value_below_is_the_last_texel(horc):
    """src/TextureLoader.cpp:20-27: u == 1.0 -> x == m_width -> {}; 1 - 2^-24 -> x == m_width - 1, a texel"""
    rc, pl, _ = horc.draw(frame(kat_tri([[1.0, 0.5]] * 3), shader=abi.SHADER_TEXTURE, tex=HOSTILE_TEX, lights=BRIGHT))
    assert rc == 0 and rgb(pl, 25, 9) == [0.0, 0.0, 0.0]
    rc, pl, _ = horc.draw(frame(kat_tri([[0.5, 7.0]] * 3), shader=abi.SHADER_TEXTURE, tex=HOSTILE_TEX, lights=BRIGHT))
    assert rgb(pl, 25, 9) == [0.0, 0.0, 0.0]  # (clamped to 1.0 first)
    below = float(F32(1.0) - F32(2.0 ** -24))
    rc, pl, _ = horc.draw(frame(kat_tri([[below, below]] * 3), shader=abi.SHADER_TEXTURE, tex=HOSTILE_TEX, lights=BRIGHT))
    assert rgb(pl, 25, 9) == [255.0, 255.0, 255.0]


def test_nan_uv_in_the_wide_fetch_is_the_last_texel(orc):
    """src/Shader.cpp:137-140: u = max_ps(zero, min_ps(u * width, width - 1)); _mm256_min_ps returns its SECOND operand when one is a
    NaN, so a NaN coordinate becomes width - 1 (include/loader/TextureLoader.hpp:56-57 converts that): texel (3, 3), not (0, 0)"""
    tex = np.full((4, 4, 3), 255, np.uint8)
    tex[0, 0], tex[3, 3], tex[0, 3], tex[3, 0] = (255, 0, 255), (0, 255, 255), (255, 255, 0), (0, 0, 255)
    orc.texture_set(13, tex)
    want = {"nan nan": [0.0, 255.0, 255.0], "nan 0": [255.0, 255.0, 0.0], "0 nan": [0.0, 0.0, 255.0], "0 0": [255.0, 0.0, 255.0]}
    for name, uv in (("nan nan", [np.nan, np.nan]), ("nan 0", [np.nan, 0.0]), ("0 nan", [0.0, np.nan]), ("0 0", [0.0, 0.0])):
        rc, pl, _ = orc.draw(frame(kat_tri([uv] * 3), shader=abi.SHADER_TEXTURE, tex=13, lights=BRIGHT))
        assert rc == 0 and rgb(pl, 12, 9) == want[name], name


def test_nan_colour_is_zero_in_both_classes(orc):
    """A light whose x is NaN makes every term of the sum a NaN.  8-wide: src/Shader.cpp:369-373 min_ps(max_ps(colour, zero), one) —
    max_ps returns its second operand, zero.  Scalar tail: src/Tools.cpp:98-103 std::clamp keeps the NaN and glm::uvec3(NaN) is
    cvttss2si's 0x8000000000000000 cut to 32 bits: 0.  The same for the light straight above a scalar pixel (src/Shader.cpp:519-523: the
    distance is 0, the intensity over it inf, times the specular term's 0: NaN)."""
    rc, pl, _ = orc.draw(frame(kat_tri(), shader=abi.SHADER_PHONG, lights=[((np.nan, 9.0, 60.0), (10.0, 20.0, 30.0))]))
    assert rc == 0 and rgb(pl, 12, 9) == [0.0, 0.0, 0.0] and rgb(pl, 25, 9) == [0.0, 0.0, 0.0]
    rc, pl, _ = orc.draw(frame(kat_tri(), shader=abi.SHADER_PHONG, lights=[((25.0, 9.0, 60.0), (10.0, 20.0, 30.0))], eye=(0, 0, 1)))
    assert rgb(pl, 25, 9) == [0.0, 0.0, 0.0] and pl[1][9, 26] > 0.0
    assert not any(np.isnan(c).any() for c in pl[1:])


def test_max_with_a_nan_cosine_keeps_the_ambient_term_in_both_classes(orc):
    """A NaN normal.  Scalar tail: src/Shader.cpp:529,535 std::max(0.f, NaN) = (0 < NaN) ? NaN : 0 = 0 (the other order would keep the
    NaN), so the pixel is ka * I, truncated.  8-wide: src/Tools.cpp:13-24 NormalSIMD::normalized blends the zero vector in where
    `len > 0` is false, include/shader/Shader.hpp:187-201 max_ps(zero, 0) = 0: ka * I again, not truncated."""
    amb = F32(0.005) * F32(100.0)
    for nrm in ((np.nan, 0, 1), (np.nan, np.nan, np.nan)):
        rc, pl, _ = orc.draw(frame(kat_tri(nrm=nrm), shader=abi.SHADER_PHONG, lights=[((40.0, 40.0, 60.0), (100.0, 100.0, 100.0))]))
        assert rc == 0
        assert rgb(pl, 12, 9) == [float(amb * F32(255.0))] * 3
        assert rgb(pl, 25, 9) == [float(np.floor(amb * F32(255.0)))] * 3 == [127.0] * 3


# ------------------------------------------------------------------------------------------------ b. the families reach their edges
def planes_differ(a, b):
    return (a[1] != b[1]) | (a[2] != b[2]) | (a[3] != b[3])


def is_black(pl):
    return (pl[1] == 0) & (pl[2] == 0) & (pl[3] == 0)


def cosines(f):
    """per light, per triangle (at its centroid, with its mean normal): the Blinn-Phong cosine n.h in binary64"""
    t = np.concatenate(f.tris)
    P = t["pos"].astype(np.float64).mean(1)
    n = t["nrm"].astype(np.float64).mean(1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    out = []
    for l in f.lights:
        hv = (l["pos"].astype(np.float64) - P) + (np.array(list(f.c.eye), np.float64) - P)
        out.append((n * hv / np.linalg.norm(hv, axis=1, keepdims=True)).sum(1))
    return out


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("family", HOSTILE_FAMILIES)
def test_family_is_drawn_clean_and_reaches_its_edge(horc, family, seed):
    n_lights = 1 + seed % 4
    f = hostile_shading_frame(seed, family, MIX, n_lights, 150.0)
    again = hostile_shading_frame(seed, family, MIX, n_lights, 150.0)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(f.tris, again.tris)), "the generator is not deterministic"
    assert f.label == ("finite" if family in ALWAYS_FINITE or (family not in ALWAYS_NONFINITE and seed % 2 == 0) else "nonfinite")
    twin = hostile_shading_frame(seed, family, MIX, n_lights, 150.0, tame=True)
    assert twin.label == "finite" and all(np.array_equal(a["pos"], b["pos"]) for a, b in zip(f.tris, twin.tris))
    ref, rst, pre, s_class = oracle_with_probes(horc, f)
    rc, tref, _ = horc.draw(twin)
    assert rc == 0
    cov = np.isfinite(ref[0])
    assert cov.mean() > 0.9 and (s_class & cov).sum() >= 200 and (~s_class & cov).sum() >= 1000, "the geometry lost a pixel class"
    thin = [t for t in np.concatenate(f.tris)[1:] if int(t["pos"][:, 0].max()) - int(t["pos"][:, 0].min()) + 1 < 8]
    assert len(thin) >= 10, "no triangles narrower than 8 pixels"
    for c in ref[1:]:
        assert not np.isnan(c).any(), "NaN in a colour plane"
        assert ((c[cov] >= 0.0) & (c[cov] <= 255.0)).all(), "a colour outside [0, 255]"
    differs = planes_differ(ref, tref)
    black_s = is_black(ref) & s_class & cov & ~is_black(tref)
    print(f"[{family} seed {seed}] {f.label}: covered {int(cov.sum())} S {int((s_class & cov).sum())} differs from the tame twin {int(differs.sum())} "
          f"black S pixels (not black in the twin) {int(black_s.sum())}")
    if family in ("uv-edge", "uv-overflow", "uv-nonfinite", "texture-shape"):
        assert black_s.sum() >= 1, "no scalar-tail pixel went through the fetch's out-of-range case"
        assert (differs & ~s_class).sum() >= 1, "no 8-wide pixel fetched another texel than its twin"
    if family == "uv-nonfinite":
        uv = np.concatenate(f.tris)["uv"]
        per_tri = (~np.isfinite(uv)).any(2).sum(1)
        assert {1, 2, 3} <= set(per_tri.tolist())
    if family == "normal-nonfinite":
        assert any(not np.isfinite(p[cov & s_class]).all() for p in pre[1:]), "no NaN reached the scalar tail's truncation"
    if family in ("normal-nonfinite", "light-edge", "eye-edge", "constants", "exponent"):
        assert differs.sum() > 0.1 * cov.sum(), "the hostile values do not change the picture"
    if family == "exponent":
        for l, c in enumerate(cosines(f)):
            assert (c > 0.9).sum() >= 5 and ((c < 0.1) & (c > 0)).sum() >= 3 and (c <= 0).sum() >= 3, (l, np.sort(c))
    if family == "texture-shape":
        assert {f._batches[b].tex_id for b in range(f.c.n_batches)} == set(HOSTILE_TEX_SHAPES)
        assert {f._batches[b].shader for b in range(f.c.n_batches)} == set(TEXTURED)


@pytest.mark.parametrize("family", HOSTILE_FAMILIES)
def test_the_tolerance_bounds_apply_to_the_frames_the_rule_names(horc, family):
    """support.tolerance_frames marks a frame `bounded` by rule (family and seed); here: exactly those frames are labelled finite AND
    have a finite pre-truncation probe at every covered pixel — a generator change that empties the set fails here, on the CPU"""
    for name, f, bounded in tolerance_frames(family):
        ref, _, pre, _ = oracle_with_probes(horc, f)
        cov = np.isfinite(ref[0])
        finite_pre = all(np.isfinite(q[cov]).all() for q in pre[1:])
        assert bounded == (f.label == "finite" and finite_pre), (name, f.label, finite_pre)


@pytest.mark.parametrize("p", HOSTILE_EXPONENTS, ids=[repr(p) for p in HOSTILE_EXPONENTS])
def test_exponent_family_takes_every_exponent(horc, p):
    """every exponent of the list is drawn clean, and (but for the ones a neighbour's picture equals by arithmetic) changes the picture
    against p = 150: both halves of pow — cosines near 1 and near 0 — are in the frame (test_family_..._reaches_its_edge)"""
    f = hostile_shading_frame(1, "exponent", (abi.SHADER_PHONG, abi.SHADER_TEXTURE), 2, p)
    rc, ref, _ = horc.draw(f)
    rc2, base, _ = horc.draw(hostile_shading_frame(1, "exponent", (abi.SHADER_PHONG, abi.SHADER_TEXTURE), 2, 150.0))
    assert rc == 0 and rc2 == 0
    cov = np.isfinite(ref[0])
    assert all(not np.isnan(c).any() and ((c[cov] >= 0) & (c[cov] <= 255)).all() for c in ref[1:])
    assert planes_differ(ref, base).sum() >= 20, p


def test_a_wrong_row_stride_changes_the_picture(horc):
    """the padded texture (slot 62) read with row_stride = 3 * w is another picture: a stride bug cannot pass the texture-shape family"""
    f = hostile_shading_frame(0, "texture-shape", (abi.SHADER_TEXTURE,), 2, 150.0)
    rc, good, _ = horc.draw(f)
    t, stride = hostile_textures()[62]
    h, w, _ = t.shape
    assert stride > 3 * w
    buf = padded_rows(t, stride)
    assert (buf[:, 3 * w:] == 0xFF).all()
    try:
        assert horc.lib().orc_texture_set(62, buf.ctypes.data, w, h, 3 * w) == 0
        rc2, bad, _ = horc.draw(f)
    finally:
        register_hostile_textures(horc)
    assert rc == 0 and rc2 == 0 and planes_differ(good, bad).sum() >= 20
    assert not planes_differ(good, horc.draw(f)[1]).any()


# ------------------------------------------------------------------------------------------------ c. the helpers
def small_planes():
    z = np.full((4, 4), 5.0, F32)
    return [z, np.full((4, 4), 10.0, F32), np.full((4, 4), 20.0, F32), np.full((4, 4), 30.0, F32)]


@pytest.mark.parametrize("plane", [1, 2, 3])
@pytest.mark.parametrize("side", ["gpu", "oracle"])
def test_compare_refuses_a_nan_on_one_side(plane, side):
    gpu, ref = small_planes(), small_planes()
    assert compare(gpu, ref, "equal") == 0
    (gpu if side == "gpu" else ref)[plane][2, 1] = np.nan
    with pytest.raises(AssertionError):
        compare(gpu, ref, "one NaN")


@pytest.mark.parametrize("plane", [1, 2, 3])
@pytest.mark.parametrize("s_pixel", [False, True], ids=["V", "S"])
@pytest.mark.parametrize("side", ["gpu", "oracle"])
def test_check_approx_refuses_a_nan_on_one_side(plane, s_pixel, side):
    gpu, ref = small_planes(), small_planes()
    s_class = np.zeros((4, 4), bool)
    s_class[2, 1] = s_pixel
    check_approx(gpu, {}, ref, {}, ref, s_class, "equal")
    (gpu if side == "gpu" else ref)[plane][2, 1] = np.nan
    with pytest.raises(AssertionError):
        check_approx(gpu, {}, ref, {}, small_planes(), s_class, "one NaN")


# ------------------------------------------------------------------------------------------------ d. the checker under ASan
def test_oracle_reads_inside_its_buffers_on_the_hostile_families(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "oracle"), "asan"])
    frames = [hostile_shading_frame(seed, family, MIX, 1 + seed % 5, HOSTILE_EXPONENTS[(3 * seed + i) % len(HOSTILE_EXPONENTS)],
                                    flags=abi.FUSED_CLEAR | (abi.UNIFIED if seed == 2 else 0))
              for i, family in enumerate(HOSTILE_FAMILIES) for seed in SEEDS]
    path = tmp_path / "hostile.srzf"
    dump_frames(path, frames)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="2")
    r = subprocess.run([os.path.join(REPO, "oracle", "build", "oracle_asan"), "--file", str(path)], capture_output=True, text=True,
                       timeout=1200, env=env)
    assert r.returncode == 0 and r.stdout.startswith(f"frames={len(frames)} "), r.stdout[-300:] + r.stderr[-4000:]
