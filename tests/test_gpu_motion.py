"""-m gpu: the motion pass (srz_frameset_motion, k_motion).  The visibility buffer is the GPU's own render_visibility (pinned to the
oracle by tests/test_gpu_visibility.py); the expected planes are tests/motionref.py's applied to that buffer (pinned to the oracle
by tests/test_motion_ref.py).  A value that is NaN on one side must be NaN on the other; every other value matches bit for bit."""
import numpy as np
import pytest
import torch

import motionref
from srz import abi, parallel
from support import SENTINEL, ccw, ctx, frame, frame_positions, hostile_shading_frame, soup, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

ALL, F = abi.MV_ALL, abi.FUSED_CLEAR
ZS = np.float32([1, 2, 3, 4])
INF = motionref.INF_WORD
# a triangle behind everything that covers any frame here (so that the smallest ones have an owner)
BACKDROP = ccw((-8, -8), (400, -8), (-8, 400), z=80.0)


def motion(fs, vis, what=ALL, delta=1, flags=F, fill=0):
    """the pass into a buffer prefilled with the word `fill` → uint32 [n, planes, rows, W]"""
    out = torch.full(fs.motion_shape(what), fill - (1 << 32) if fill >= 1 << 31 else fill, dtype=torch.int32, device="cuda")
    assert fs.motion_bytes(what) == out.numel() * 4
    fs.motion(vis.data_ptr(), out.data_ptr(), fs.motion_bytes(what), what, delta, flags, stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def expect(tmp_path, frames, vis, what=ALL, delta=1, fused=True, fill=0):
    """motionref per frame on the GPU's visibility words; a frame whose target lies outside the set is nobody everywhere"""
    v = vis if isinstance(vis, np.ndarray) else words(vis)
    out = []
    for i in range(len(frames)):
        g = i + delta
        if 0 <= g < len(frames):
            pre = np.full((5,) + v.shape[2:], fill, np.uint32)
            e = motionref.expected(tmp_path, frame_positions(frames[g]), v[i], v[g], fused, pre)
        else:
            e = motionref.nobody(v.shape[2:], fused, fill)
        out.append(e[motionref.planes_of(what)])
    return np.stack(out)


def moved(t, d=(3.3, -2.7, 0.5), seed=5, jitter=1.5):
    """the triangles a little elsewhere: a common shift and a jitter per vertex"""
    t2 = t.copy()
    t2["pos"] = (t["pos"] + np.float32(d) + np.random.default_rng(seed).normal(0, jitter, t["pos"].shape)).astype(np.float32)
    return t2


def with_positions(f, pos):
    """abi.Frame f with the positions [n, 9] instead of its own"""
    batches, k = [], 0
    for b, t in enumerate(f.tris):
        t2 = t.copy()
        t2["pos"] = np.asarray(pos, np.float32).reshape(-1, 3, 3)[k:k + len(t)]
        k += len(t)
        batches.append((int(f._batches[b].shader), int(f._batches[b].tex_id), t2))
    return frame(batches, f.width, f.height, flags=f.c.flags)


def pair(w, h, n, flags=F):
    t = np.concatenate([soup(1, n, w, h, ZS, big=w < 40), BACKDROP])
    return [frame(t, w, h, flags=flags), frame(moved(t), w, h, flags=flags)]


@pytest.mark.parametrize("w,h,n", [(64, 64, 90), (100, 70, 120), (50, 37, 40), (33, 1, 6), (1, 1, 3)])
def test_sizes(ctx, tmp_path, w, h, n):
    """a soup and the soup moved, each with a backdrop; W and H no multiples of 32; W no multiple of 4 (partial quads, pixel by pixel);
    one row; one pixel.  delta = +1 and -1: the frame without a target is all zeros"""
    frames = pair(w, h, n)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    assert (v[:, 1] != 0).any(1).any(1).all()
    if w >= 50:
        assert (v[0, 1][:, 48:] != 0).any() and (v[0, 1][32:] != 0).any()  # the partial tile column and band
    for delta, empty in ((1, 1), (-1, 0)):
        got = motion(fs, vis, ALL, delta, F, SENTINEL)
        same(got, expect(tmp_path, frames, vis, ALL, delta, fill=SENTINEL), f"{w}x{h} delta {delta}")
        assert (got[empty] == 0).all() and (got[1 - empty, 2] != 0).any()
    fs.close()


def test_every_mask_is_a_slice_of_the_full_buffer(ctx, tmp_path):
    frames = pair(100, 70, 120)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    full = motion(fs, vis, ALL)
    same(full, expect(tmp_path, frames, vis), "all groups")
    for what in range(1, 8):
        part = motion(fs, vis, what)
        assert part.shape[1] == len(motionref.planes_of(what)) == fs.motion_shape(what)[1]
        assert np.array_equal(part, full[:, motionref.planes_of(what)]), what
    fs.close()


def test_nine_frames_wrap_the_frame_deal(ctx, tmp_path):
    """workgroup b takes the frames f ≡ b mod 8: the ninth frame is the second of workgroup 0's; delta = 3 leaves the last three
    frames without a target, delta = -8 all but the last"""
    t = np.concatenate([soup(11, 60, 64, 64, ZS), BACKDROP])
    frames = [frame(moved(t, (1.5 * i, -1.0 * i, 0.25 * i), seed=i, jitter=0.5), 64, 64) for i in range(9)]
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    for delta, live in ((3, range(0, 6)), (-8, range(8, 9))):
        got = motion(fs, vis, ALL, delta, F, SENTINEL)
        same(got, expect(tmp_path, frames, vis, ALL, delta, fill=SENTINEL), f"delta {delta}")
        for i in range(9):
            assert (got[i] != 0).any() == (i in live), (delta, i)
        assert len({got[i].tobytes() for i in live}) == len(live)
    fs.close()


@pytest.mark.parametrize("unified", [False, True])
def test_the_frame_is_its_own_target(ctx, tmp_path, unified):
    """delta == 0: DEPTH is plane 0 of the buffer and TARGET the pixel's own id and z, at every owned pixel"""
    flags = F | (abi.UNIFIED if unified else 0)
    frames = [frame(np.concatenate([soup(0, 90, 64, 64, ZS), BACKDROP]), 64, 64, flags=flags),
              hostile_shading_frame(0, "uv-edge", tame=True, flags=flags)]
    fs = ctx.frameset(frames)
    vis = visibility(fs, flags)
    v = words(vis)
    got = motion(fs, vis, ALL, 0)
    same(got, expect(tmp_path, frames, vis, ALL, 0), "delta 0")
    own, s_class = v[:, 1] != 0, (v[:, 1] >> 31) != 0
    assert own.sum() > 4000 and (s_class.any() != unified)
    assert np.array_equal(got[:, 2][own], v[:, 0][own]) and np.array_equal(got[:, 3][own], v[:, 1][own]) and np.array_equal(got[:, 4][own], v[:, 0][own])
    flow = got[:, 0:2].view(np.float32)
    assert (np.abs(flow[:, 0][own]) < 0.5).all() and (np.abs(flow[:, 1][own]) < 0.5).all()
    assert not (got[:, 3] >> 31).any() or not unified
    fs.close()


def test_translation_lands_on_the_moved_pixel(ctx, tmp_path):
    """tests/test_motion_ref.py's translation frames on the GPU's own buffers: every owned pixel lands on (x + k, y + m) and finds its
    own id word there, class bit included"""
    k, m, _ = motionref.TRANSLATION
    frames = list(motionref.translation_frames())
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    got = motion(fs, vis, ALL, 1)
    same(got, expect(tmp_path, frames, vis), "translation")
    own = v[0, 1] != 0
    s_class = own & ((v[0, 1] >> 31) != 0)
    assert (own & ~s_class).sum() >= 200 and s_class.sum() >= 200
    dx, dy = got[0, 0].view(np.float32), got[0, 1].view(np.float32)
    assert (np.abs(dx[own] - k) < 0.5).all() and (np.abs(dy[own] - m) < 0.5).all()
    ys, xs = np.nonzero(own)
    assert np.array_equal(got[0, 3][own], v[0, 1][own]), "tid is not the pixel's own id word"
    assert np.array_equal(got[0, 3][own], v[1, 1][ys + m, xs + k]) and np.array_equal(got[0, 4][own], v[1, 0][ys + m, xs + k])
    assert np.array_equal(got[0, 2][own], got[0, 4][own])
    fs.close()


def test_hostile_targets(ctx, tmp_path):
    """tests/test_motion_ref.py's hostile target positions (NaN, +-inf, +-1e30, the borders of the nearest-sample range): the planes
    are the reference's bit for bit, and nothing outside the image was read as a target"""
    f = frame(soup(4, 300, 70, 50, ZS), 70, 50)
    frames = [f, with_positions(f, motionref.hostile_target_positions(frame_positions(f), 70, 50))]
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    got = motion(fs, vis, ALL, 1)
    same(got, expect(tmp_path, frames, vis), "hostile targets")
    own = words(vis)[0, 1] != 0
    flow = got[0, 0:2].view(np.float32)
    outside = own & (got[0, 3] == 0) & (got[0, 4] == INF)
    assert np.isnan(flow[:, own]).any() and np.isinf(flow[:, own]).any() and outside.sum() > 200 and (own & ~outside).sum() > 200
    fs.close()


def test_nobody_pixels_and_out_of_range_ids(ctx, tmp_path):
    """frames that do not clear: fused (the call's flag) gives zeros at nobody's pixels and at ids outside the frame's triangles, not
    fused keeps the prefill there; owned pixels are the same words in both runs"""
    t = soup(3, 40, 96, 80, ZS)
    frames = [frame(t, 96, 80, flags=0), frame(moved(t), 96, 80, flags=0)]
    fs = ctx.frameset(frames)
    v = visibility(fs).cpu().numpy()
    ids = v[0, 1].view(np.uint32)
    ids[0, :16] = len(t) + 1
    ids[1, :16] = 0x7fffffff
    ids[2, :16] = 0xffffffff
    ids[3, :16] = (len(t) + 1) | 0x80000000
    vis = torch.as_tensor(v).cuda()
    nobody = (ids == 0) | (((ids & 0x7fffffff) - 1) >= len(t))
    assert nobody[:4, :16].all() and nobody.sum() > 500 and (~nobody).sum() > 200
    fused = motion(fs, vis, ALL, 1, F, SENTINEL)
    kept = motion(fs, vis, ALL, 1, 0, SENTINEL)
    same(fused, expect(tmp_path, frames, vis, fused=True, fill=SENTINEL), "fused")
    same(kept, expect(tmp_path, frames, vis, fused=False, fill=SENTINEL), "not fused")
    assert (fused[0][:, nobody] == 0).all() and (kept[0][:, nobody] == SENTINEL).all()
    assert np.array_equal(fused[0][:, ~nobody], kept[0][:, ~nobody])
    assert (fused[1] == 0).all() and (kept[1] == SENTINEL).all()  # the frame without a target
    fs.close()


def test_sceneset_equals_the_frameset_of_its_stream(ctx, tmp_path):
    from srz import scenes as pscenes
    wl = pscenes.spot_bunny_1080p()
    wl.upload_meshes(ctx)
    frames = [wl.frame(3), wl.frame(4)]
    fs, ss = ctx.frameset(frames), ctx.frameset([wl.scene_frame(3), wl.scene_frame(4)])
    vis_f, vis_s = visibility(fs), visibility(ss)
    assert torch.equal(vis_f.view(torch.int32), vis_s.view(torch.int32))
    got_f, got_s = motion(fs, vis_f), motion(ss, vis_s)
    same(got_s, got_f, "sceneset against frameset")
    same(got_f, expect(tmp_path, frames, vis_f), "frameset against the reference")
    assert (got_s[0, 3] != 0).sum() > 10000 and (got_s[0, 0] != 0).any()
    fs.close(), ss.close()


def test_shard_rows_through_the_band_map(ctx, tmp_path):
    import srz
    w, h = 70, 100
    t = soup(5, 150, w, h, ZS, big=True)
    frames = [frame(t, w, h), frame(moved(t), w, h)]
    what = abi.MV_FLOW | abi.MV_DEPTH
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    full = motion(fs, vis, what)
    same(full, expect(tmp_path, frames, vis, what), "unsharded")
    fs.close()
    c = srz.Context(0, 1, 3)
    fs = c.frameset(frames)
    svis = visibility(fs)
    shard = motion(fs, svis, what)
    rows = parallel.band_rows(h, 1, 3)
    assert len(rows) >= 1 and fs.local_rows % 32 == 0
    for (lb, _, r0, r1) in rows:
        assert (full[0, 2, r0:r1] != 0).any()
        same(shard[:, :, lb * 32: lb * 32 + r1 - r0], full[:, :, r0:r1], f"local band {lb}")
    out = torch.full(fs.motion_shape(ALL), 5, dtype=torch.int32, device="cuda")
    for bad in (abi.MV_TARGET, ALL):
        rc = srz.lib().srz_frameset_motion(c.h, fs.h, svis.data_ptr(), out.data_ptr(), fs.motion_bytes(bad), bad, 1, F, None)
        assert rc == abi.SRZ_E_INVALID, bad
    torch.cuda.synchronize()
    assert (out == 5).all()
    fs.close(), c.close()


def test_misuse(ctx, tmp_path):
    import srz
    L = srz.lib()
    t = soup(1, 60, 64, 64, ZS)
    a, b, short = frame(t, 64, 64), frame(moved(t), 64, 64), frame(t[:50], 64, 64)
    fs = ctx.frameset([a, short, b])
    vis = visibility(fs)
    out = torch.full(fs.motion_shape(ALL), 5, dtype=torch.int32, device="cuda")
    nb, h, e = fs.motion_bytes(ALL), ctx.h, abi.SRZ_E_INVALID
    v, o = vis.data_ptr(), out.data_ptr()
    assert fs.motion_bytes(0) == 0 and fs.motion_bytes(8) == 0 and fs.motion_bytes(abi.MV_DEPTH | 32) == 0
    assert nb == 3 * 5 * 64 * 64 * 4 and fs.motion_bytes(abi.MV_DEPTH) == 3 * 64 * 64 * 4
    D = abi.MV_DEPTH
    assert L.srz_frameset_motion(h, fs.h, v, o, nb, 0, 2, F, None) == e                       # what == 0
    assert L.srz_frameset_motion(h, fs.h, v, o, nb, ALL | 8, 2, F, None) == e                 # an unknown bit
    assert L.srz_frameset_motion(h, fs.h, v, o, nb - 4, ALL, 2, F, None) == e                 # too small
    assert L.srz_frameset_motion(h, fs.h, v, o + 4, nb, D, 2, F, None) == e                   # misaligned output
    assert L.srz_frameset_motion(h, fs.h, v + 4, o, nb, ALL, 2, F, None) == e                 # misaligned visibility buffer
    assert L.srz_frameset_motion(h, fs.h, v, v, nb, D, 2, F, None) == e                       # the output IS the visibility buffer
    assert L.srz_frameset_motion(h, fs.h, v, v + 3 * 64 * 64 * 4, nb, D, 2, F, None) == e     # ... or lies inside it
    for flag in (abi.UNIFIED, abi.ORDERED_RASTER, abi.NO_Z_READBACK, 16, F | abi.UNIFIED):
        assert L.srz_frameset_motion(h, fs.h, v, o, nb, ALL, 2, flag, None) == e, flag        # a flag other than SRZ_FUSED_CLEAR
    for delta in (1, -1):                                                                     # 60 against 50 triangles, in range
        assert L.srz_frameset_motion(h, fs.h, v, o, nb, ALL, delta, F, None) == e, delta
        assert "triangle count" in L.srz_last_error(h).decode()
    assert L.srz_frameset_motion(h, fs.h, None, o, nb, ALL, 2, F, None) == e
    assert L.srz_frameset_motion(h, fs.h, v, None, nb, ALL, 2, F, None) == e
    assert L.srz_frameset_motion(h, None, v, o, nb, ALL, 2, F, None) == e
    torch.cuda.synchronize()
    assert (out == 5).all()
    # the same counts with the differing pair out of range: delta = 2 pairs frame 0 with frame 2 only
    frames = [a, short, b]
    got = motion(fs, vis, ALL, 2)
    want = expect(tmp_path, frames, vis, ALL, 2)
    same(got, want, "delta 2")
    assert (got[0, 3] != 0).any() and (got[1:] == 0).all()
    for delta in (3, -3, 2 ** 31 - 1, -2 ** 31):  # no pair at all: accepted, nobody everywhere
        assert (motion(fs, vis, ALL, delta, F, SENTINEL) == 0).all(), delta
    fs.close()


def test_decode_on_the_device(ctx):
    from srz.visibility import decode, motion_decode
    frames = pair(64, 64, 90)
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    out = torch.zeros(fs.motion_shape(ALL), dtype=torch.float32, device="cuda")
    fs.motion(vis.data_ptr(), out.data_ptr(), fs.motion_bytes(ALL), ALL, 1, F, stream())
    torch.cuda.synchronize()
    m = motion_decode(out, ALL)
    assert m["flow"].data_ptr() == out.data_ptr() and m["flow"].shape == (2, 2, 64, 64) and m["depth"].shape == (2, 64, 64)
    tri = decode(vis).tri
    visible = (m["target_index"][0] == tri[0]) & (tri[0] >= 0)
    assert visible.sum().item() > 1000 and m["target_index"].max().item() < 91 and m["target_index"][1].max().item() == -1
    assert torch.isfinite(m["target_z"][0][visible]).all() and (m["target_s_class"][0] & (m["target_index"][0] < 0)).sum().item() == 0
    fs.close()
