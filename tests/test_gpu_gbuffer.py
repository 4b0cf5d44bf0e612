"""-m gpu: the G-buffer pass (srz_frameset_gbuffer, k_gbuffer).  The visibility buffer is the GPU's own render_visibility (pinned to
the oracle by tests/test_gpu_visibility.py); the expected planes are tests/gbufref.py's applied to that buffer (pinned to the oracle
by tests/test_gbuffer_ref.py).  A value that is NaN on one side must be NaN on the other; every other value matches bit for bit."""
import numpy as np
import pytest
import torch

import gbufref
import scenes
from srz import abi, parallel
from support import (MIX_ALL, SENTINEL, ccw, ctx, frame, hostile_shading_frame, hostile_textures, lit, register_hostile_textures, soup,  # noqa: F401
                     stack, stream, visibility, words)

pytestmark = pytest.mark.gpu

ALL, F = abi.GB_ALL, abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
# a triangle behind everything that covers any frame here (so that the smallest ones have an owner), with attributes of its own
BACKDROP = ccw((-8, -8), (400, -8), (-8, 400), z=80.0, nrm=((0.2, 0.1, 1.0), (-0.3, 0.2, 0.9), (0.1, -0.4, 0.8)), uv=((0.1, 0.2), (0.9, 0.3), (0.4, 0.8)))


@pytest.fixture(scope="module")
def tex(ctx, orc):
    """the hostile textures in the context (and the oracle), and every texture a frame here may name: slot -> (h, w, 3) uint8"""
    register_hostile_textures(orc, ctx)
    t = {slot: a for slot, (a, _) in hostile_textures().items()}
    t[scenes.TEX_SPOT] = np.ascontiguousarray(scenes.spot_texture(), np.uint8)
    return t


def gbuffer(fs, vis, what=ALL, flags=F, fill=0):
    """the pass into a buffer prefilled with the word `fill` → uint32 [n, planes, rows, W]"""
    out = torch.full(fs.gbuffer_shape(what), fill - (1 << 32) if fill >= 1 << 31 else fill, dtype=torch.int32, device="cuda")
    assert fs.gbuffer_bytes(what) == out.numel() * 4
    fs.gbuffer(vis.data_ptr(), out.data_ptr(), fs.gbuffer_bytes(what), what, flags, stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def expect(tmp_path, frames, tex, vis, what=ALL, fused=True, fill=0, shading=None):
    v = words(vis)
    out = []
    for i, f in enumerate(frames):
        pre = np.full((9,) + v.shape[2:], fill, np.uint32)
        e = gbufref.expected(tmp_path, f, tex, v[i], fused, pre, shading[i] if shading else None)
        out.append(e[gbufref.planes_of(what)])
    return np.stack(out)


def check(ctx, tmp_path, tex, frames, what=ALL, flags=F, name=""):
    fs = ctx.frameset(frames)
    vis = visibility(fs, flags)
    got = gbuffer(fs, vis, what, flags & F)  # (the pass takes SRZ_FUSED_CLEAR only; every frame here carries it anyway)
    same(got, expect(tmp_path, frames, tex, vis, what), name)
    fs.close()
    return got, words(vis)


@pytest.mark.parametrize("w,h,n", [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6), (1, 1, 3)])
def test_sizes(ctx, tmp_path, tex, w, h, n):
    """a soup; W and H no multiples of 32; W no multiple of 4 (partial quads, pixel by pixel); one row; one pixel"""
    t = np.concatenate([soup(1, n, w, h, ZS, big=w < 40), BACKDROP])
    f = frame([(abi.SHADER_TEXTURE, 40, t[0::2]), (abi.SHADER_PHONG, -1, t[1::2])], w, h, lights=[[[10, 10, 50], [9, 9, 9]]])
    got, vis = check(ctx, tmp_path, tex, [f], name=f"{w}x{h}")
    assert (vis[0, 1] != 0).any()
    if w >= 50:
        assert (vis[0, 1][:, 48:] != 0).any() and (vis[0, 1][32:] != 0).any()  # the partial tile column and band


def test_every_mask_is_a_slice_of_the_full_buffer(ctx, tmp_path, tex):
    f = hostile_shading_frame(0, "texture-shape", MIX_ALL)
    fs = ctx.frameset([f])
    vis = visibility(fs)
    full = gbuffer(fs, vis, ALL)
    same(full, expect(tmp_path, [f], tex, vis), "all groups")
    for what in range(1, 16):
        part = gbuffer(fs, vis, what)
        assert part.shape[1] == len(gbufref.planes_of(what)) == fs.gbuffer_shape(what)[1]
        assert np.array_equal(part, full[:, gbufref.planes_of(what)]), what
    fs.close()


def test_nine_frames_wrap_the_frame_deal(ctx, tmp_path, tex):
    """workgroup b takes the frames f ≡ b mod 8: the ninth frame is the second of workgroup 0's"""
    frames = [frame([(abi.SHADER_TEXTURE, 40, soup(10 + i, 40 + 5 * i, 64, 64, ZS))], 64, 64) for i in range(9)]
    got, _ = check(ctx, tmp_path, tex, frames, name="nine frames")
    assert len({got[i].tobytes() for i in range(9)}) == 9


def test_unified_is_all_v_class(ctx, tmp_path, tex):
    f = hostile_shading_frame(1, "texture-shape", MIX_ALL, flags=F | abi.UNIFIED)
    _, vis = check(ctx, tmp_path, tex, [f], flags=F | abi.UNIFIED, name="unified")
    assert (vis[0, 1] != 0).any() and not (vis[0, 1] >> 31).any()


def test_every_shader_type_and_its_albedo(ctx, tmp_path, tex):
    f = hostile_shading_frame(2, "uv-edge", MIX_ALL)
    got, vis = check(ctx, tmp_path, tex, [f], name="MIX_ALL")
    ids, batch, kd = vis[0, 1], got[0, 5].astype(np.int64) - 1, got[0, 6:9].view(np.float32)
    s_class = (ids >> 31) != 0
    shader = np.where(batch >= 0, np.asarray(MIX_ALL)[np.clip(batch, 0, 4)], -1)
    ones = (kd == 1.0).all(0)
    for sh in (abi.SHADER_PHONG, abi.SHADER_NORMAL):
        assert (shader == sh).sum() > 50 and ones[shader == sh].all(), sh
    for sh in (abi.SHADER_BUMP, abi.SHADER_DISPLACEMENT):
        v = (shader == sh) & ~s_class
        assert v.sum() > 50 and ones[v].all(), sh
        assert ((shader == sh) & s_class & ~ones).any(), sh  # S-class BUMP / DISPLACEMENT fetch their texel
    assert ((shader == abi.SHADER_TEXTURE) & ~ones).any()


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("family", ["normal-nonfinite", "uv-nonfinite", "uv-overflow", "uv-edge", "texture-shape"])
def test_hostile_families(ctx, tmp_path, tex, family, seed):
    check(ctx, tmp_path, tex, [hostile_shading_frame(seed, family, MIX_ALL)], name=f"{family} {seed}")


def test_zero_length_normal(ctx, tmp_path, tex):
    f0 = hostile_shading_frame(0, "uv-edge", tame=True)
    batches = []
    for b, t in enumerate(f0.tris):
        t2 = t.copy()
        t2["nrm"] = 0.0
        batches.append((int(f0._batches[b].shader), int(f0._batches[b].tex_id), t2))
    got, vis = check(ctx, tmp_path, tex, [lit(f0, batches=batches)], name="zero normals")
    ids, n = vis[0, 1], got[0, 0:3].view(np.float32)
    v, s = (ids != 0) & ((ids >> 31) == 0), (ids >> 31) != 0
    assert v.sum() >= 200 and s.sum() >= 200
    assert (got[0, 0:3][:, v] == 0).all() and np.isnan(n[:, s]).all()


def test_nobody_pixels(ctx, tmp_path, tex):
    t = soup(3, 40, 64, 64, ZS)
    f = frame([(abi.SHADER_TEXTURE, 40, t)], 64, 64, flags=0)
    fs = ctx.frameset([f])
    vis = visibility(fs)
    nobody = words(vis)[0, 1] == 0
    assert nobody.sum() > 500 and (~nobody).sum() > 200
    fused = gbuffer(fs, vis, ALL, F, SENTINEL)
    kept = gbuffer(fs, vis, ALL, 0, SENTINEL)
    same(fused, expect(tmp_path, [f], tex, vis, fused=True, fill=SENTINEL), "fused")
    same(kept, expect(tmp_path, [f], tex, vis, fused=False, fill=SENTINEL), "not fused")
    assert (fused[0][:, nobody] == 0).all() and (kept[0][:, nobody] == SENTINEL).all()
    assert np.array_equal(fused[0][:, ~nobody], kept[0][:, ~nobody]) and (kept[0, 5][~nobody] == 1).all()
    fs.close()


def test_out_of_range_ids_are_nobody(ctx, tmp_path, tex):
    t = soup(1, 120, 96, 80, ZS)
    f = frame([(abi.SHADER_TEXTURE, 40, t)], 96, 80, flags=0)
    fs = ctx.frameset([f])
    v = visibility(fs).cpu().numpy()
    ids = v[0, 1].view(np.uint32)
    ids[0, :16] = len(t) + 1
    ids[1, :16] = 0x7fffffff
    ids[2, :16] = 0xffffffff
    ids[3, :16] = (len(t) + 1) | 0x80000000
    vis = torch.as_tensor(v).cuda()
    for flags in (F, 0):
        got = gbuffer(fs, vis, ALL, flags, SENTINEL)
        same(got, expect(tmp_path, [f], tex, vis, fused=flags == F, fill=SENTINEL), f"flags {flags}")
        assert (got[0, :, :4, :16] == (0 if flags else SENTINEL)).all()
    fs.close()


def test_update_shading_moves_the_albedo_only(ctx, tmp_path, tex):
    t = hostile_shading_frame(3, "texture-shape", (abi.SHADER_TEXTURE,)).tris
    t = [np.concatenate(t[0::2]), np.concatenate(t[1::2])]
    f = frame([(abi.SHADER_TEXTURE, 40, t[0]), (abi.SHADER_TEXTURE, 12, t[1])], lights=[[[10, 10, 50], [9, 9, 9]]])
    fs = ctx.frameset([f])
    vis = visibility(fs)
    before = gbuffer(fs, vis)
    same(before, expect(tmp_path, [f], tex, vis), "before")
    f2 = lit(f, batches=[(abi.SHADER_PHONG, -1, t[0]), (abi.SHADER_TEXTURE, 23, t[1])])
    fs.update_shading([f2])
    after = gbuffer(fs, vis)
    same(after, expect(tmp_path, [f], tex, vis, shading=[[(abi.SHADER_PHONG, -1), (abi.SHADER_TEXTURE, 23)]]), "after")
    assert np.array_equal(before[:, :6], after[:, :6]) and not np.array_equal(before[:, 6:], after[:, 6:])
    b0 = after[0, 5] == 1
    assert b0.sum() > 200 and (after[0, 6:9].view(np.float32)[:, b0] == 1.0).all()
    fs.close()


def test_sceneset_equals_the_frameset_of_its_stream(ctx, tmp_path, tex):
    from srz import scenes as pscenes
    wl = pscenes.spot_bunny_1080p()
    wl.upload_meshes(ctx)
    frames = [wl.frame(3)]
    fs, ss = ctx.frameset(frames), ctx.frameset([wl.scene_frame(3)])
    vis_f, vis_s = visibility(fs), visibility(ss)
    assert torch.equal(vis_f.view(torch.int32), vis_s.view(torch.int32))
    got_f, got_s = gbuffer(fs, vis_f), gbuffer(ss, vis_s)
    same(got_s, got_f, "sceneset against frameset")
    same(got_f, expect(tmp_path, frames, tex, vis_f), "frameset against the reference")
    assert {0, 1, 2} <= set(np.unique(got_s[0, 5]).tolist())  # nobody and both draws
    fs.close(), ss.close()


def test_shard_rows_through_the_band_map(ctx, orc, tmp_path, tex):
    import srz
    w, h = 70, 100
    t = soup(5, 150, w, h, ZS, big=True)
    f = frame([(abi.SHADER_TEXTURE, 40, t[0::2]), (abi.SHADER_NORMAL, -1, t[1::2])], w, h)
    full, _ = check(ctx, tmp_path, tex, [f], name="unsharded")
    c = srz.Context(0, 1, 3)
    register_hostile_textures(orc, c)
    fs = c.frameset([f])
    shard = gbuffer(fs, visibility(fs))
    rows = parallel.band_rows(h, 1, 3)
    assert len(rows) >= 1 and fs.local_rows % 32 == 0
    for (lb, _, r0, r1) in rows:
        assert (full[:, 5, r0:r1] != 0).any()
        same(shard[:, :, lb * 32: lb * 32 + r1 - r0], full[:, :, r0:r1], f"local band {lb}")
    fs.close(), c.close()


def test_misuse(ctx):
    import srz
    L = srz.lib()
    f = frame([(abi.SHADER_TEXTURE, 40, soup(1, 60, 64, 64, ZS))], 64, 64)
    fs = ctx.frameset([f])
    vis = visibility(fs)
    out = torch.full(fs.gbuffer_shape(ALL), 5, dtype=torch.int32, device="cuda")
    nb, h, e = fs.gbuffer_bytes(ALL), ctx.h, abi.SRZ_E_INVALID
    v, o = vis.data_ptr(), out.data_ptr()
    assert fs.gbuffer_bytes(0) == 0 and fs.gbuffer_bytes(16) == 0 and fs.gbuffer_bytes(abi.GB_UV | 32) == 0
    assert nb == 9 * 64 * 64 * 4 and fs.gbuffer_bytes(abi.GB_BATCH) == 64 * 64 * 4
    assert L.srz_frameset_gbuffer(h, fs.h, v, o, nb, 0, F, None) == e                      # what == 0
    assert L.srz_frameset_gbuffer(h, fs.h, v, o, nb, ALL | 16, F, None) == e               # an unknown bit
    assert L.srz_frameset_gbuffer(h, fs.h, v, o, nb - 4, ALL, F, None) == e                # too small
    assert L.srz_frameset_gbuffer(h, fs.h, v, o + 4, nb, abi.GB_UV, F, None) == e          # misaligned output
    assert L.srz_frameset_gbuffer(h, fs.h, v + 4, o, nb, ALL, F, None) == e                # misaligned visibility buffer
    assert L.srz_frameset_gbuffer(h, fs.h, v, v, nb, abi.GB_BATCH, F, None) == e           # the output IS the visibility buffer
    assert L.srz_frameset_gbuffer(h, fs.h, v, v + 3 * 64 * 64 * 4, nb, abi.GB_BATCH, F, None) == e  # ... or lies inside it
    for flag in (abi.UNIFIED, abi.ORDERED_RASTER, abi.NO_Z_READBACK, 16, F | abi.UNIFIED):
        assert L.srz_frameset_gbuffer(h, fs.h, v, o, nb, ALL, flag, None) == e, flag       # a flag other than SRZ_FUSED_CLEAR
    assert L.srz_frameset_gbuffer(h, fs.h, None, o, nb, ALL, F, None) == e
    assert L.srz_frameset_gbuffer(h, fs.h, v, None, nb, ALL, F, None) == e
    assert L.srz_frameset_gbuffer(h, None, v, o, nb, ALL, F, None) == e
    torch.cuda.synchronize()
    assert (out == 5).all()
    fs.close()


def test_a_missing_texture_matters_to_the_albedo_only(ctx, tmp_path, tex):
    import srz
    f = frame([(abi.SHADER_TEXTURE, 55, soup(1, 60, 64, 64, ZS))], 64, 64)  # slot 55: never uploaded
    fs = ctx.frameset([f])
    vis = visibility(fs)
    out = torch.zeros(fs.gbuffer_shape(ALL), dtype=torch.int32, device="cuda")
    rc = srz.lib().srz_frameset_gbuffer(ctx.h, fs.h, vis.data_ptr(), out.data_ptr(), fs.gbuffer_bytes(ALL), ALL, F, None)
    assert rc == abi.SRZ_E_TEXTURE and "55" in srz.lib().srz_last_error(ctx.h).decode()
    with pytest.raises(srz.SrzError) as err:
        fs.gbuffer(vis.data_ptr(), out.data_ptr(), fs.gbuffer_bytes(abi.GB_ALBEDO), abi.GB_ALBEDO, F, stream())
    assert err.value.code == abi.SRZ_E_TEXTURE
    what = abi.GB_NORMAL | abi.GB_UV | abi.GB_BATCH
    same(gbuffer(fs, vis, what), expect(tmp_path, [f], tex, vis, what), "without ALBEDO")
    fs.close()


def test_decode_on_the_device(ctx, tex):
    from srz.visibility import gbuffer_decode
    f = hostile_shading_frame(0, "uv-edge", MIX_ALL, tame=True)
    fs = ctx.frameset([f])
    vis = visibility(fs)
    out = torch.zeros(fs.gbuffer_shape(ALL), dtype=torch.float32, device="cuda")
    fs.gbuffer(vis.data_ptr(), out.data_ptr(), fs.gbuffer_bytes(ALL), ALL, F, stream())
    torch.cuda.synchronize()
    g = gbuffer_decode(out, ALL)
    assert g["normal"].data_ptr() == out.data_ptr() and g["batch"].min().item() >= 0 and g["batch"].max().item() == len(MIX_ALL) - 1
    length = (g["normal"] ** 2).sum(1).sqrt()
    assert ((length - 1).abs() < 1e-5).all()
    fs.close()


# ---- the oracle itself, through the numpy restatements of tests/test_gbuffer_ref.py -------------------------------------------------
def classes(vis):
    ids = vis[0, 1]
    s = (ids >> 31) != 0
    v = (ids != 0) & ~s
    assert v.sum() >= 200 and s.sum() >= 200, (int(v.sum()), int(s.sum()))
    return v, s


def same_colour(got, ref, own, what):
    for c in range(3):
        bad = own & (np.ascontiguousarray(got[c]).view(np.uint32) != np.ascontiguousarray(ref[c], np.float32).view(np.uint32))
        assert not bad.any(), f"{what}: plane {c}: {int(bad.sum())} pixels differ from the oracle's colour"


@pytest.mark.parametrize("name,make", [("soup 0", lambda: frame(soup(0, 90, 64, 64, ZS), 64, 64)), ("stack 200", lambda: stack(200)),
                                       ("wide and thin", lambda: hostile_shading_frame(0, "uv-edge", tame=True))])
def test_oracle_anchor_normals(ctx, orc, name, make):
    f = make()
    nf = lit(f, batches=[(abi.SHADER_NORMAL, -1, t) for t in f.tris])
    fs = ctx.frameset([nf])
    vis = visibility(fs)
    got = gbuffer(fs, vis, abi.GB_NORMAL)
    v, s = classes(words(vis))
    n = got[0].view(np.float32)
    assert not np.isnan(n[:, v | s]).any()
    rc, ref, _ = orc.draw(nf, want_stats=False)
    assert rc == 0
    same_colour(gbufref.normal_colour(n, s), ref[1:], v | s, name)
    fs.close()


@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_anchor_albedo(ctx, orc, tex, seed):
    f = gbufref.albedo_frame(hostile_shading_frame(seed, "texture-shape", (abi.SHADER_TEXTURE,)))
    fs = ctx.frameset([f])
    vis = visibility(fs)
    got = gbuffer(fs, vis, abi.GB_UV | abi.GB_ALBEDO)
    v, s = classes(words(vis))
    kd = got[0, 2:5].view(np.float32)
    assert not np.isnan(got[0].view(np.float32)[:, v | s]).any()
    rc, ref, _ = orc.draw(f, want_stats=False)
    assert rc == 0
    same_colour(gbufref.albedo_colour(kd, s), ref[1:], v | s, f"albedo {seed}")
    fs.close()
