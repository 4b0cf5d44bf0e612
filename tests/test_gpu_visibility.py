"""-m gpu: the visibility buffer (srz_frameset_render_visibility, k_visibility) against the oracle-built reference of
tests/visref.py: ids (owner + 1 | S class), z, alpha and beta bit for bit, on every id width of k_raster's owner slots and on the
ordered rasteriser; accumulate mode; scenesets; sharding and both exchanges; no interference with the colour render."""
import numpy as np
import pytest
import torch

import scenes
import visref
from srz import abi, parallel
from support import ctx, frame, render, same, soup, stack, words  # noqa: F401  (ctx: the fixture)

pytestmark = pytest.mark.gpu


def check(ctx, tmp_path, orc, frames, flags=abi.FUSED_CLEAR, prefill=None, what=""):
    """every frame's visibility buffer equals the reference; returns the frameset (its debug counters) and the words"""
    refs = [visref.Reference(tmp_path, f) for f in frames]
    fs, out = render(ctx, [r.gpu_frame for r in refs], flags, prefill, vis=True)
    got = words(out)
    for i, r in enumerate(refs):
        init = None if prefill is None else tuple(prefill[i, p, :r.H] for p in range(4))
        exp, _, amb, _, _ = r.expected(orc, init)
        assert amb == 0, f"{what}: {amb} pixels decode ambiguously"
        same(got[i, :, :r.H], exp, f"{what} frame {i} (planes z, id, alpha, beta)")
    return fs, got


@pytest.mark.parametrize("shader", [abi.SHADER_TEXTURE, abi.SHADER_PHONG, abi.SHADER_NORMAL])
def test_spot_ids_z_alpha_beta(ctx, tmp_path, orc, shader):
    frames = [scenes.config2(a, size=512, shader=shader) for a in (0, 4, 13, 27)]
    _, vis = check(ctx, tmp_path, orc, frames, what=f"spot512 shader {shader}")
    # plane 0 is the colour render's plane 0 bit for bit
    refs = [visref.Reference(tmp_path, f) for f in frames]
    col = words(render(ctx, [r.gpu_frame for r in refs])[1])
    assert np.array_equal(col[:, 0], vis[:, 0])
    assert (vis[:, 1] & 0x80000000).any() and ((vis[:, 1] != 0) & ((vis[:, 1] & 0x80000000) == 0)).any()  # both classes


def test_config3_and_config5(ctx, tmp_path, orc):
    check(ctx, tmp_path, orc, [scenes.config3(2)], what="config3 1080p")
    fs, _ = check(ctx, tmp_path, orc, [scenes.config5(3, size=1024)], what="config5 x8 at 1024")


@pytest.mark.parametrize("seed", range(6))
def test_soups_with_ties_and_unified(ctx, tmp_path, orc, seed):
    zs = np.array([1.0, 2.0, 2.0, 3.0, 0.5], np.float32)
    t = soup(seed, 150, 96, 80, zs, big=seed % 3 == 1)
    check(ctx, tmp_path, orc, [frame(t, 96, 80)], what=f"soup {seed}")
    check(ctx, tmp_path, orc, [frame(t, 96, 80, flags=abi.FUSED_CLEAR | abi.UNIFIED)], what=f"soup {seed} unified")


@pytest.mark.parametrize("n", [100, 300, 700])
def test_every_id_width(ctx, tmp_path, orc, n):
    """<= 127 list entries: 8-bit positions; 128..512: 16-bit; > 512 triangles over one tile: 32-bit indices"""
    check(ctx, tmp_path, orc, [stack(n), stack(n, jitter=1)], what=f"{n} over one tile")


@pytest.mark.parametrize("seed", range(3))
def test_ordered_rasteriser_paths(ctx, tmp_path, orc, seed):
    """±0 and NaN depths (k_raster hands those tiles to k_raster_slow) and SRZ_ORDERED_RASTER everywhere"""
    zs = np.array([0.0, -0.0, 1e-30, -1e-30, 1.0], np.float32)
    t = soup(seed, 60, 96, 80, zs)
    fs, _ = check(ctx, tmp_path, orc, [frame(t, 96, 80)], what=f"zero-z {seed}")
    assert fs.debug_counters()["slow_tiles"] > 0
    t2 = soup(seed + 10, 80, 96, 80, np.array([1.0, 2.0, np.nan], np.float32))
    fs, _ = check(ctx, tmp_path, orc, [frame(t2, 96, 80)], what=f"nan-z {seed}")
    fs, _ = check(ctx, tmp_path, orc, [frame(soup(seed + 20, 120, 96, 80, np.float32([1, 2, 3])), 96, 80,
                                              flags=abi.FUSED_CLEAR | abi.ORDERED_RASTER)], what=f"ordered {seed}")
    assert fs.debug_counters()["slow_tiles"] > 0


def test_accumulate_mode_keeps_what_survives(ctx, tmp_path, orc):
    rng = np.random.default_rng(5)
    frames = [frame(soup(s, 120, 96, 80, np.float32([1, 2, 3])), 96, 80, flags=0) for s in (1, 2)]
    pre = rng.integers(0, 2 ** 32, (2, 4, 80, 96), dtype=np.uint64).astype(np.uint32).view(np.float32)
    pre[:, 0] = rng.uniform(0.5, 4.0, (2, 80, 96)).astype(np.float32)
    pre[:, 1:] = np.where(np.isnan(pre[:, 1:]), np.float32(7), pre[:, 1:])  # (NaN payloads are kept by copies, but not by every compare)
    check(ctx, tmp_path, orc, frames, flags=0, prefill=pre, what="accumulate")


def test_width_not_a_multiple_of_4_or_32(ctx, tmp_path, orc):
    """50 x 37: two tile columns and two bands, the second of each partial, and no aligned quad in the frame (W % 4 != 0) — every quad
    is read back and written pixel by pixel, up to the frame's edge in the last one of a row.  With SRZ_FUSED_CLEAR, and in accumulate
    mode over a prefilled buffer, whose words stay where nobody owns the pixel"""
    w, h = 50, 37
    t = soup(1, 36, w, h, np.float32([1, 2, 3]))
    _, fused = check(ctx, tmp_path, orc, [frame(t, w, h)], what="50x37 fused")
    ids = fused[0, 1, :h]
    assert (ids[:, 48:] != 0).any() and (ids[32:] != 0).any() and (ids[32:, 32:] != 0).any()  # the partial column, band, corner
    rng = np.random.default_rng(9)
    pre = rng.integers(0, 2 ** 32, (1, 4, h, w), dtype=np.uint64).astype(np.uint32).view(np.float32)
    pre[:, 0] = rng.uniform(0.5, 4.0, (1, h, w)).astype(np.float32)
    pre[:, 1:] = np.where(np.isnan(pre[:, 1:]), np.float32(7), pre[:, 1:])
    _, acc = check(ctx, tmp_path, orc, [frame(t, w, h, flags=0)], flags=0, prefill=pre, what="50x37 accumulate")
    nobody = ids == 0  # (nobody with the clear's depth behind it: nobody in front of the prefill's either)
    assert nobody.any() and np.array_equal(acc[0, :, :h][:, nobody], pre.view(np.uint32)[0][:, nobody])


def test_sceneset_ids_are_draw_offset_plus_face(ctx):
    """the vertex-stage path gives the buffer of a frameset of the host-built stream (spot + bunny: two draws)"""
    from srz import scenes as pscenes
    from srz import visibility
    wl = pscenes.spot_bunny_1080p()
    wl.upload_meshes(ctx)
    idx = (0, 11)
    ws = words(render(ctx, [wl.scene_frame(i) for i in idx], vis=True)[1])
    frames = [wl.frame(i) for i in idx]
    wf = words(render(ctx, frames, vis=True)[1])
    assert np.array_equal(ws, wf)
    n0 = len(frames[0].tris[0])
    v = visibility.decode(torch.as_tensor(ws.view(np.float32)))
    d = visibility.batch_of([len(t) for t in frames[0].tris], v.tri)
    assert (d == 0).any() and (d == 1).any()
    assert (v.tri[d == 1] >= n0).all() and (v.tri[d == 0] < n0).all()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_shards_and_both_exchanges(ctx, tmp_path, world):
    import srz
    w, h = 200, 270
    frames = [abi.Frame(w, h, scenes.EYE, scenes.LIGHTS, [(abi.SHADER_TEXTURE, scenes.TEX_SPOT,
                        scenes.mesh_stream(scenes.SPOT_OBJ, w, h, float(10 * a), (0, 0, 0), 0.3))], abi.FUSED_CLEAR) for a in (3, 9)]
    full = words(render(ctx, frames, vis=True)[1])
    s = torch.cuda.current_stream().cuda_stream
    ctxs, sets, g, msgs = [], [], [], []
    for r in range(world):
        c = srz.Context(0, r, world)
        fs = c.frameset(frames)
        gb = torch.zeros((world,) + fs.out_shape, dtype=torch.float32, device="cuda")
        fs.render_visibility(gb[r].data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
        cap = fs.sparse_capacity()
        m = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        fs.sparse_pack(gb[r].data_ptr(), m.data_ptr(), cap, abi.EXCHANGE_PLANES, s)
        ctxs.append(c), sets.append(fs), g.append(gb), msgs.append(m)
    torch.cuda.synchronize()
    shard = [g[r][r].cpu().numpy().view(np.uint32) for r in range(world)]
    for r in range(world):  # every rank's shard holds the unsharded buffer's rows
        for (lb, _, r0, r1) in parallel.band_rows(h, r, world):
            assert np.array_equal(shard[r][:, :, lb * 32: lb * 32 + r1 - r0], full[:, :, r0:r1]), (world, r, lb)
    dense = torch.stack([g[r][r] for r in range(world)])  # = the in-place all-gather's result
    fullg = torch.zeros((len(frames), 4, sets[0].local_rows * world, w), dtype=torch.float32, device="cuda")
    sets[0].deinterleave(dense.data_ptr(), fullg.data_ptr(), abi.EXCHANGE_PLANES, s)
    torch.cuda.synchronize()
    assert np.array_equal(fullg[:, :, :h].cpu().numpy().view(np.uint32), full[:, :, :h])
    recv = torch.stack(msgs).contiguous()
    cap = msgs[0].numel()
    for r in range(world):
        sets[r].sparse_unpack(recv.data_ptr(), cap, g[r].data_ptr(), abi.EXCHANGE_PLANES, s)
    torch.cuda.synchronize()
    for r in range(world):
        for q in range(world):
            for (lb, _, r0, r1) in parallel.band_rows(h, q, world):
                a = g[r][q][:, :, lb * 32: lb * 32 + r1 - r0].cpu().numpy().view(np.uint32)
                assert np.array_equal(a, full[:, :, r0:r1]), (world, r, q, lb)
    for fs, c in zip(sets, ctxs):
        fs.close(), c.close()


def test_no_interference_with_the_colour_render(ctx):
    import srz
    frames = [scenes.config2(i % 36, size=1024) for i in range(16)]  # a batch-sized set: the side clear and its grid measurement
    s = torch.cuda.current_stream().cuda_stream

    def run(mixed):
        c = srz.Context(0)
        c.texture_upload(scenes.TEX_SPOT, scenes.spot_texture())
        fs = c.frameset(frames)
        col = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
        vis = torch.zeros_like(col)
        outs, seq = [], []
        for k in range(26):
            fs.render(col.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
            if k in (0, 25):
                outs.append(col.clone())
            d = fs.debug_counters()
            seq.append((d["clear_tuned"], d["clear_wgs"]))
            if mixed:
                fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
        torch.cuda.synchronize()
        fs.close(), c.close()
        return outs, seq, vis

    o1, s1, _ = run(False)
    o2, s2, vis = run(True)
    for a, b in zip(o1, o2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the grid measurement of the mixed set ran as a colour-only set's does: it decided, on one of the candidates, and once decided it
    # stays (which candidate wins is a timing, not a property of the renders)
    for sq in (s1, s2):
        tuned = [t for t, _ in sq]
        assert tuned == sorted(tuned) and tuned[-1] == 1 and sq[-1][1] in (96, 128, 256), sq
    # the tolerance mode of the shaders does not touch the visibility buffer
    c = srz.Context(0)
    c.set_option(abi.OPT_APPROX_SHADE, 1)
    fs = c.frameset(frames)
    vis2 = torch.zeros_like(vis)
    fs.render_visibility(vis2.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    torch.cuda.synchronize()
    assert torch.equal(vis.view(torch.int32), vis2.view(torch.int32))
    fs.close(), c.close()
