"""not-gpu: the G-buffer's test reference (tests/gbuf_ref.c through tests/gbufref.py) pinned to the unchanged CPU oracle.

Owners, classes, alpha and beta of a frame come from visref.Reference.expected (positions only decide them); the reference's normals
and albedo of the frame's OWN attributes then go through the numpy restatements of what the built-in shaders do with them
(gbufref.normal_colour / albedo_colour) and must equal the oracle's colour render bit for bit on every owned pixel: the NORMAL-shaded
frame for the normals, a frame lit so that its colour is its albedo for the albedo (and, through the texel it selects, for uv)."""
import numpy as np
import pytest

import gbufref
from srz import abi
from support import MAX_AMBIGUOUS, bits, frame, hostile_shading_frame, hostile_textures, lit, padded_rows, soup, stack, visibility_of

ZS = np.float32([1, 2, 3, 4])
# the session's oracle is shared with modules that rely on slot 63 being empty (tests/test_oracle_kat.py): its texture goes to slot 50
REMAP = {63: 50}


def textures(orc):
    """support.hostile_textures() into the oracle, each from its padded rows with its row stride → slot -> (h, w, 3) texels"""
    out = {}
    for slot, (t, stride) in hostile_textures().items():
        buf = padded_rows(t, stride)
        assert orc.lib().orc_texture_set(REMAP.get(slot, slot), buf.ctypes.data, t.shape[1], t.shape[0], stride) == 0
        out[REMAP.get(slot, slot)] = t
    return out
NORMAL_FRAMES = {"soup 0": lambda: frame(soup(0, 90, 64, 64, ZS), 64, 64), "soup 2": lambda: frame(soup(2, 90, 64, 64, ZS), 64, 64),
                 "soup 3 (quarter-pixel vertices)": lambda: frame(soup(3, 90, 64, 64, ZS), 64, 64), "stack 200": lambda: stack(200),
                 "wide and thin": lambda: hostile_shading_frame(0, "uv-edge", tame=True)}


def same_colour(got, ref, mask, what):
    for c in range(3):
        bad = mask & (bits(got[c]) != bits(np.ascontiguousarray(ref[c], np.float32)))
        assert not bad.any(), f"{what}: colour plane {c} differs at {int(bad.sum())} pixels, first (y, x) {np.argwhere(bad)[:4].tolist()}: " \
                              f"restated {got[c][bad][:4]} oracle {ref[c][bad][:4]}"


@pytest.mark.parametrize("name", sorted(NORMAL_FRAMES))
def test_normals_are_what_the_normal_shader_sees(tmp_path, orc, name):
    f = NORMAL_FRAMES[name]()
    v = visibility_of(tmp_path, orc, f, max_ambiguous=MAX_AMBIGUOUS)
    words, v_class, s_class = v.words, v.v_class, v.s_class
    nf = lit(f, batches=[(abi.SHADER_NORMAL, -1, t) for t in f.tris])  # the frame's own normals, NORMAL-shaded
    rc, ref, _ = orc.draw(nf, want_stats=False)
    assert rc == 0
    planes = gbufref.expected(tmp_path, nf, {}, words).view(np.float32)
    own = v_class | s_class
    assert not np.isnan(planes[0:5][:, own]).any()
    same_colour(gbufref.normal_colour(planes[0:3], s_class), ref[1:], own, name)
    assert np.array_equal(planes.view(np.uint32)[5][own], _batch_plus_1(nf, words)[own])


def _batch_plus_1(f, words):
    ends = np.cumsum([len(t) for t in f.tris])
    tri = (words[1] & 0x7fffffff).astype(np.int64) - 1
    return np.where(tri >= 0, np.searchsorted(ends, tri, side="right") + 1, 0).astype(np.uint32)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_albedo_and_uv_are_what_the_texture_shader_sees(tmp_path, orc, seed):
    """one TEXTURE batch per texture of support.hostile_textures() (1x1, 1x7, 7x1, 5x7, padded strides), uv over [-0.05, 1.05]"""
    tex = textures(orc)
    f = gbufref.albedo_frame(hostile_shading_frame(seed, "texture-shape", (abi.SHADER_TEXTURE,)), REMAP)
    uv = np.concatenate([t["uv"].ravel() for t in f.tris])
    assert uv.min() < -0.03 and uv.max() > 1.03  # (drawn from [-0.05, 1.05]: both borders are crossed)
    assert {int(f._batches[b].tex_id) for b in range(len(f.tris))} == set(tex) and len(tex) == len(hostile_textures())
    v = visibility_of(tmp_path, orc, f, max_ambiguous=MAX_AMBIGUOUS)
    words, v_class, s_class = v.words, v.v_class, v.s_class
    rc, ref, _ = orc.draw(f, want_stats=False)
    assert rc == 0
    planes = gbufref.expected(tmp_path, f, tex, words).view(np.float32)
    own = v_class | s_class
    assert not np.isnan(planes[:, own][[0, 1, 2, 3, 4, 6, 7, 8]]).any()
    same_colour(gbufref.albedo_colour(planes[6:9], s_class), ref[1:], own, f"albedo seed {seed}")
    # the fetch's corners are all there: black (S, u or v == 1), texel (0, 0)'s bright value, and V pixels never black (no zero byte)
    assert (planes[6][s_class] == 0).any() and (planes[6][v_class] > 0).all()


def test_nobody_and_out_of_range_ids(tmp_path):
    """id 0, the bare class bit and an index past the triangles are nobody: zeros when fused, untouched otherwise"""
    f = frame(soup(1, 5, 8, 8, ZS), 8, 8)
    words = np.zeros((4, 1, 6), np.uint32)
    words[1, 0] = [0, 0x80000000, 6, 0x7fffffff, 0xffffffff, 1]
    words[2:, 0] = np.float32(0.25).view(np.uint32)
    pre = np.full((9, 1, 6), 0xdeadbeef, np.uint32)
    fused = gbufref.expected(tmp_path, f, {}, words, fused=True, prefill=pre)
    kept = gbufref.expected(tmp_path, f, {}, words, fused=False, prefill=pre)
    assert (fused[:, 0, :5] == 0).all() and (kept[:, 0, :5] == 0xdeadbeef).all()
    assert np.array_equal(fused[:, 0, 5], kept[:, 0, 5]) and fused[5, 0, 5] == 1 and (fused[6:, 0, 5] == np.float32(1).view(np.uint32)).all()
