"""-m gpu: shading a visibility buffer (srz_frameset_shade_visibility, k_shade_vis) and relighting a set (srz_frameset_update_shading):
shade(render_visibility(F)) is the colour render of F bit for bit — every shading build, every owner-id width, the ordered rasteriser,
SRZ_UNIFIED, the tolerance mode, shards —; relit sets equal their colour render and the oracle; accumulate mode, in place, misuse."""
import ctypes

import numpy as np
import pytest
import torch

import scenes
from srz import abi
from support import ccw, compare, ctx, frame, lit, run, same, soup, stack, stream, words  # noqa: F401  (ctx: the fixture)

pytestmark = pytest.mark.gpu


def check(ctx, frames, flags=abi.FUSED_CLEAR, what=""):
    fs = ctx.frameset(frames)
    col, out, vis = run(fs, flags)
    same(col.swapaxes(0, 1), out.swapaxes(0, 1), what)
    assert (words(vis)[:, 1] != 0).any(), f"{what}: nothing drawn"
    fs.close()
    return col


@pytest.mark.parametrize("shader", [abi.SHADER_TEXTURE, abi.SHADER_PHONG, abi.SHADER_NORMAL, abi.SHADER_BUMP, abi.SHADER_DISPLACEMENT])
def test_config2_every_shader(ctx, shader):
    check(ctx, [scenes.config2(a, size=512, shader=shader) for a in (0, 13)], what=f"shader {shader}")


LIGHTS5 = np.array([[[0.9, 0.9, -0.9], [100, 100, 100]], [[0.0, 0.8, 0.9], [50, 50, 50]], [[-0.7, 0.2, 0.5], [30, 60, 90]],
                    [[0.3, -0.8, 0.7], [70, 70, 70]], [[0.1, 0.1, 1.5], [20, 25, 30]]], np.float32)


@pytest.mark.parametrize("n_lights", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("grey", [True, False])
def test_every_light_count_grey_or_not(ctx, n_lights, grey):
    L = LIGHTS5[:n_lights].copy()
    if grey:
        L[:, 1] = L[:, 1, :1]
    frames = [lit(scenes.config2(a, size=512, shader=sh), L) for a, sh in ((3, abi.SHADER_TEXTURE), (7, abi.SHADER_PHONG))]
    check(ctx, frames, what=f"{n_lights} lights grey={grey}")


@pytest.mark.parametrize("p", [150.0, 32.0, 7.5, 5000.0])
def test_exponents(ctx, p):
    """150 and 32: the integer chains; 7.5: pow_fast (GENPOW); 5000: outside both fast domains (generic)"""
    frames = [lit(scenes.config2(a, size=512, shader=sh), p=p) for a, sh in ((5, abi.SHADER_TEXTURE), (9, abi.SHADER_PHONG))]
    check(ctx, frames, what=f"p={p}")


def test_config3_config5_and_readme_scene(ctx):
    import srz
    check(ctx, [scenes.config3(2)], what="config3")
    check(ctx, [scenes.config5(3, size=1024)], what="config5 1024")
    c = srz.Context(0)
    c.texture_upload(scenes.TEX_SPOT, scenes.spot_texture())
    c.texture_upload(scenes.TEX_CRATE, scenes.crate_texture())
    check(c, [scenes.readme_scene(i, size=512) for i in (0, 5)], what="readme spot + crate")
    c.close()


@pytest.mark.parametrize("seed", range(4))
def test_soups_unified_and_ordered(ctx, seed):
    zs = np.array([1.0, 2.0, 2.0, 3.0, 0.5], np.float32)
    t = soup(seed, 150, 96, 80, zs, big=seed % 3 == 1)
    check(ctx, [frame(t, 96, 80)], what=f"soup {seed}")
    check(ctx, [frame(t, 96, 80, flags=abi.FUSED_CLEAR | abi.UNIFIED)], what=f"soup {seed} unified")
    check(ctx, [frame(t, 96, 80, flags=abi.FUSED_CLEAR | abi.ORDERED_RASTER)], what=f"soup {seed} ordered")
    t0 = soup(seed, 60, 96, 80, np.array([0.0, -0.0, 1e-30, 1.0], np.float32))
    check(ctx, [frame(t0, 96, 80)], what=f"zero-z soup {seed}")


@pytest.mark.parametrize("n", [100, 300, 700])
def test_every_id_width(ctx, n):
    check(ctx, [stack(n), stack(n, jitter=1)], what=f"{n} over one tile")


def test_tolerance_mode_against_its_own_colour_render():
    import srz
    c = srz.Context(0)
    c.set_option(abi.OPT_APPROX_SHADE, 1)
    c.texture_upload(scenes.TEX_SPOT, scenes.spot_texture())
    frames = [scenes.config2(a, size=512, shader=sh) for a, sh in ((1, abi.SHADER_TEXTURE), (2, abi.SHADER_PHONG), (3, abi.SHADER_BUMP))]
    frames.append(lit(scenes.config2(4, size=512), LIGHTS5[:3], p=7.5))
    check(c, frames, what="approx")
    c.close()


def test_relight_after_update_shading(ctx, orc):
    frames = [scenes.config2(a, size=512, shader=sh) for a, sh in ((2, abi.SHADER_TEXTURE), (8, abi.SHADER_PHONG))]
    fs = ctx.frameset(frames)
    vis = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    s = stream()
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    f0, f1 = frames
    new = [lit(f0, LIGHTS5[2:4], ka=(0.1, 0.05, 0.02), ks=(0.9, 0.8, 0.7), p=32.0),  # (same light counts: 2)
           lit(f1, LIGHTS5[3:5], p=64.0, batches=[(abi.SHADER_NORMAL, -1, f1.tris[0])])]
    with pytest.raises(Exception):  # (the structure must stay: another light count)
        fs.update_shading([lit(f0, LIGHTS5[:3]), f1])
    fs.update_shading(new)
    out = torch.zeros_like(vis)
    col = torch.zeros_like(vis)
    fs.shade_visibility(vis.data_ptr(), out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    fs.render(col.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    torch.cuda.synchronize()
    assert np.array_equal(words(out), words(col))
    for i, f in enumerate(new):
        rc, ref, _ = orc.draw(f)
        assert rc == 0
        compare(out[i].cpu().numpy(), ref, f"relit frame {i}")
    fs.close()


def test_sceneset_relit_through_sceneset_update(ctx, orc):
    import srz
    from srz import scenes as pscenes
    wl = pscenes.spot_bunny_1080p()
    wl.upload_meshes(ctx)
    sfs = [wl.scene_frame(i) for i in (0, 11)]
    fs = ctx.frameset(sfs)
    vis = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    s = stream()
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    torch.cuda.synchronize()
    for sf in sfs:  # new lights and exponent, same matrices
        L = np.ascontiguousarray(LIGHTS5[1:1 + sf.c.n_lights].reshape(-1, 6)).view(abi.LIGHT_DTYPE).reshape(-1)
        sf.lights = L
        sf.c.lights = L.ctypes.data
        sf.c.p = 40.0
    ctx._check(srz.lib().srz_sceneset_update(ctx.h, fs.h, abi.scene_frames_array(sfs), len(sfs)))
    out, col = torch.zeros_like(vis), torch.zeros_like(vis)
    fs.shade_visibility(vis.data_ptr(), out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    fs.render(col.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    torch.cuda.synchronize()
    assert np.array_equal(words(out), words(col))
    # the oracle on the host-built stream of the same frames with the new lights (the vertex stage's stream is that stream bit for bit:
    # tests/test_gpu_visibility.py::test_sceneset_ids_are_draw_offset_plus_face)
    for i, (k, sf) in enumerate(zip((0, 11), sfs)):
        f = lit(wl.frame(k), LIGHTS5[1:1 + sf.c.n_lights], p=40.0)
        rc, ref, _ = orc.draw(f)
        assert rc == 0
        compare(out[i].cpu().numpy(), ref, f"relit scene frame {k}")
    # update_shading is for framesets: a sceneset is refused, its buffers untouched
    plain = abi.frames_array([wl.frame(0), wl.frame(11)])
    assert srz.lib().srz_frameset_update_shading(ctx.h, fs.h, plain, 2) == abi.SRZ_E_INVALID
    assert "srz_sceneset_update" in srz.lib().srz_last_error(ctx.h).decode()
    out2 = torch.zeros_like(vis)
    fs.shade_visibility(vis.data_ptr(), out2.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    torch.cuda.synchronize()
    assert np.array_equal(words(out2), words(col))
    fs.close()


@pytest.mark.parametrize("shader", [abi.SHADER_PHONG, abi.SHADER_TEXTURE, abi.SHADER_NORMAL])
@pytest.mark.parametrize("build", ["fast2", "generic5", "generic_p5000"])
def test_operands_outside_the_fast_math_range(ctx, shader, build):
    """test_gpu_parity's zero / huge / tiny normals, a light straight above a pixel and one at the eye: the FAST build (2 lights) hands the
    tiles to the generic build's redo list, the generic build (5 lights, or p = 5000) re-shades them at once — both with IEEE math, bit
    for bit as the colour render"""
    tris = np.concatenate([
        ccw((4, 4), (30.5, 4), (4, 30.5), nrm=(0, 0, 0)),
        ccw((34, 4), (60.5, 4), (34, 30.5), nrm=(1e30, -1e30, 1e30)),
        ccw((4, 34), (30.5, 34), (4, 60.5), nrm=(1e-30, 1e-30, -1e-30)),
        ccw((34, 34), (47.5, 34), (34, 47.5), nrm=(0.3, -0.2, -1)),
        ccw((50, 50), (55, 50), (50, 55), nrm=(0, 0, -1), uv=((0.1, 0.1), (0.9, 0.2), (0.4, 0.8)))])
    lights = [[(40.0, 40.0, 60.0), (500, 500, 500)], [(0.0, 0.0, 1.0), (300, 200, 100)]]
    if build == "generic5":
        lights += [[(-0.7, 0.2, 0.5), (30, 60, 90)], [(0.3, -0.8, 0.7), (70, 70, 70)], [(0.1, 0.1, 1.5), (20, 25, 30)]]
    kw = {"p": 5000.0} if build == "generic_p5000" else {}
    tex = scenes.TEX_SPOT if shader == abi.SHADER_TEXTURE else -1
    for flags in (abi.FUSED_CLEAR, abi.FUSED_CLEAR | abi.UNIFIED):
        f = frame(tris, shader=shader, lights=lights, tex=tex, flags=flags, **kw)
        ctx.draw(f, want_stats=True)  # (the counting run's generic k_shade counts the tiles that took the IEEE pass)
        assert ctx.debug_counters()[11] >= 1, "no tile left FastMath's range: the test does not reach the fallback"
        fs = ctx.frameset([f, f])
        col, out, _ = run(fs)
        assert np.array_equal(col, out), (build, shader, flags)
        if build == "fast2":  # (the shade's own hand-back: redo_count is the shade's after it)
            assert fs.debug_counters()["redo_tiles"] >= 1
        fs.close()


def test_accumulate_mode_and_layering(ctx):
    rng = np.random.default_rng(3)
    frames = [frame(soup(sd, 120, 96, 80, np.float32([1, 2, 3])), 96, 80, flags=0, shader=abi.SHADER_NORMAL) for sd in (1, 2)]
    fs = ctx.frameset(frames)
    s = stream()
    # a non-fused shade leaves the "nobody" pixels of a poisoned output untouched
    vis = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    poison = torch.full_like(vis, -7.25)
    fs.shade_visibility(vis.data_ptr(), poison.data_ptr(), fs.out_bytes, 0, s)
    torch.cuda.synchronize()
    nobody = words(vis)[:, 1] == 0
    assert nobody.any() and (poison.cpu().numpy()[:, :, :80][np.broadcast_to(nobody[:, None, :80], (2, 4, 80, 96))] == -7.25).all()
    # layering: colour render onto B == shade (non-fused, onto B) of the visibility render onto (B.z, 0, 0, 0)
    B = rng.uniform(0, 255, fs.out_shape).astype(np.float32)
    B[:, 0] = rng.uniform(0.5, 4.0, (2, fs.local_rows, 96)).astype(np.float32)
    col = torch.as_tensor(B).cuda()
    fs.render(col.data_ptr(), fs.out_bytes, 0, s)
    vb = np.zeros_like(B)
    vb[:, 0] = B[:, 0]
    vis2 = torch.as_tensor(vb).cuda()
    fs.render_visibility(vis2.data_ptr(), fs.out_bytes, 0, s)
    out = torch.as_tensor(B).cuda()
    fs.shade_visibility(vis2.data_ptr(), out.data_ptr(), fs.out_bytes, 0, s)
    torch.cuda.synchronize()
    assert np.array_equal(words(out), words(col))
    fs.close()


def test_in_place(ctx):
    frames = [scenes.config2(a, size=512) for a in (4, 21)]
    fs = ctx.frameset(frames)
    s = stream()
    col = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    buf = torch.zeros_like(col)
    fs.render(col.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    fs.render_visibility(buf.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    fs.shade_visibility(buf.data_ptr(), buf.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    torch.cuda.synchronize()
    assert np.array_equal(words(buf), words(col))
    fs.close()


def test_width_not_a_multiple_of_4_or_32(ctx):
    """50 x 37: a partial second tile column and band, no aligned quad in the frame (the ids, z, α, β and the colour of every quad go
    pixel by pixel, the last quad of a row ends at the frame's edge) — fused, accumulate and in place against the colour render"""
    w, h = 50, 37
    t = soup(1, 36, w, h, np.float32([1, 2, 3]))
    col = check(ctx, [frame(t, w, h)], what="50x37 fused")
    s = stream()
    # accumulate (as test_accumulate_mode_and_layering; the frame's own flags without SRZ_FUSED_CLEAR too, they are OR-ed in): colour
    # render onto B == shade onto B of the visibility render onto (B.z, 0, 0, 0), and B's words stay where nobody owns the pixel
    fs = ctx.frameset([frame(t, w, h, flags=0)])
    rng = np.random.default_rng(4)
    B = rng.uniform(0, 255, fs.out_shape).astype(np.float32)
    B[:, 0] = rng.uniform(0.5, 4.0, B[:, 0].shape).astype(np.float32)
    vb = np.zeros_like(B)
    vb[:, 0] = B[:, 0]
    acc, vis, out = torch.as_tensor(B).cuda(), torch.as_tensor(vb).cuda(), torch.as_tensor(B).cuda()
    fs.render(acc.data_ptr(), fs.out_bytes, 0, s)
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, 0, s)
    fs.shade_visibility(vis.data_ptr(), out.data_ptr(), fs.out_bytes, 0, s)
    torch.cuda.synchronize()
    nobody = words(vis)[:, 1] == 0
    assert nobody.any() and (~nobody).any() and (~nobody)[:, :, 48:].any()
    assert np.array_equal(words(out), words(acc))
    keep = np.broadcast_to(nobody[:, None], B.shape)
    assert np.array_equal(words(out)[keep], B.view(np.uint32)[keep])
    assert not np.array_equal(words(out)[:, 1:], B.view(np.uint32)[:, 1:])  # (and the owned ones were shaded)
    fs.close()
    fs = ctx.frameset([frame(t, w, h)])  # in place (fused)
    buf = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render_visibility(buf.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    fs.shade_visibility(buf.data_ptr(), buf.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    torch.cuda.synchronize()
    assert np.array_equal(words(buf), col)
    fs.close()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_shards(ctx, world):
    import srz
    w, h = 200, 270
    frames = [abi.Frame(w, h, scenes.EYE, scenes.LIGHTS, [(abi.SHADER_TEXTURE, scenes.TEX_SPOT,
                        scenes.mesh_stream(scenes.SPOT_OBJ, w, h, float(10 * a), (0, 0, 0), 0.3))], abi.FUSED_CLEAR) for a in (3, 9)]
    for r in range(world):
        c = srz.Context(0, r, world)
        c.texture_upload(scenes.TEX_SPOT, scenes.spot_texture())
        fs = c.frameset(frames)
        col, out, _ = run(fs)
        assert np.array_equal(col, out), (world, r)
        fs.close(), c.close()


def test_out_of_range_ids_are_nobody(ctx):
    t0 = soup(1, 120, 96, 80, np.float32([1, 2, 3]))
    t1 = soup(2, 120, 96, 80, np.float32([1, 2, 3]))
    fs = ctx.frameset([frame(t0, 96, 80, flags=0), frame(t1, 96, 80, flags=0)])
    s = stream()
    vis = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    torch.cuda.synchronize()
    v = vis.cpu().numpy()
    ids = v[0, 1].view(np.uint32)
    n0 = len(t0)
    ids[0, :16] = np.arange(n0 + 1, n0 + 17, dtype=np.uint32)  # indices of frame 1's triangles, seen from frame 0
    ids[1, :16] = np.arange(n0 + 1, n0 + 17, dtype=np.uint32) | 0x80000000
    v[0, 0, :2, :16] = 1.5
    vis = torch.as_tensor(v).cuda()
    out = torch.full_like(vis, 9.0)
    fs.shade_visibility(vis.data_ptr(), out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    o = torch.full_like(vis, 9.0)
    fs.shade_visibility(vis.data_ptr(), o.data_ptr(), fs.out_bytes, 0, s)
    torch.cuda.synchronize()
    got, got0 = out.cpu().numpy(), o.cpu().numpy()
    assert (got[0, 0, :2, :16] == np.inf).all() and (got[0, 1:, :2, :16] == 0).all()
    assert (got0[0, :, :2, :16] == 9.0).all()
    # in place with SRZ_FUSED_CLEAR the out-of-range words become the clear values too; the owned pixels equal the separate shade's
    fs.shade_visibility(vis.data_ptr(), vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    torch.cuda.synchronize()
    ip = vis.cpu().numpy()
    assert (ip[0, 0, :2, :16] == np.inf).all() and (ip[0, 1:, :2, :16] == 0).all()
    assert np.array_equal(ip.view(np.uint32), got.view(np.uint32))


def test_misuse_is_an_error_and_leaves_the_output(ctx):
    import srz
    L = srz.lib()
    fs = ctx.frameset([scenes.config2(1, size=256)])
    n = fs.out_bytes // 4
    big = torch.zeros(3 * n + 64, dtype=torch.float32, device="cuda")
    vis, out = big[:n], big[n + 16: 2 * n + 16]
    s = stream()
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    out.fill_(5.0)
    torch.cuda.synchronize()
    h, e = ctx.h, abi.SRZ_E_INVALID
    assert L.srz_frameset_shade_visibility(h, fs.h, None, out.data_ptr(), fs.out_bytes, 1, None) == e
    assert L.srz_frameset_shade_visibility(h, fs.h, vis.data_ptr(), None, fs.out_bytes, 1, None) == e
    assert L.srz_frameset_shade_visibility(h, None, vis.data_ptr(), out.data_ptr(), fs.out_bytes, 1, None) == e
    assert L.srz_frameset_shade_visibility(h, fs.h, vis.data_ptr(), out.data_ptr(), fs.out_bytes - 4, 1, None) == e
    assert L.srz_frameset_shade_visibility(h, fs.h, vis.data_ptr(), out.data_ptr() + 4, fs.out_bytes, 1, None) == e
    assert L.srz_frameset_shade_visibility(h, fs.h, vis.data_ptr() + 4, out.data_ptr(), fs.out_bytes, 1, None) == e
    assert L.srz_frameset_shade_visibility(h, fs.h, vis.data_ptr(), vis.data_ptr() + 64, fs.out_bytes, 1, None) == e
    assert L.srz_frameset_shade_visibility(h, fs.h, vis.data_ptr() + 64, vis.data_ptr(), fs.out_bytes, 1, None) == e
    f = scenes.config2(1, size=256)
    bad_light = [lit(f, LIGHTS5[:3])]
    assert L.srz_frameset_update_shading(h, fs.h, abi.frames_array(bad_light), 1) == e
    t = f.tris[0][:-1]
    assert L.srz_frameset_update_shading(h, fs.h, abi.frames_array([lit(f, batches=[(abi.SHADER_TEXTURE, scenes.TEX_SPOT, t)])]), 1) == e
    assert L.srz_frameset_update_shading(h, fs.h, abi.frames_array([f, f]), 2) == e
    torch.cuda.synchronize()
    assert (out == 5.0).all()
    fs.close()


def test_no_interference_with_the_clear_grid_measurement(ctx):
    import srz
    frames = [scenes.config2(i % 36, size=1024) for i in range(16)]
    s = stream()

    def go(mixed):
        c = srz.Context(0)
        c.texture_upload(scenes.TEX_SPOT, scenes.spot_texture())
        fs = c.frameset(frames)
        col = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
        vis, sh = torch.zeros_like(col), torch.zeros_like(col)
        outs, seq = [], []
        if mixed:
            fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
        for k in range(26):
            fs.render(col.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
            if k in (0, 25):
                outs.append(col.clone())
            d = fs.debug_counters()
            seq.append((d["clear_tuned"], d["clear_wgs"]))
            if mixed:
                fs.shade_visibility(vis.data_ptr(), sh.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
        torch.cuda.synchronize()
        fs.close(), c.close()
        return outs, seq, sh

    o1, s1, _ = go(False)
    o2, s2, sh = go(True)
    for a, b in zip(o1, o2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(sh.view(torch.int32), o2[-1].view(torch.int32))
    for sq in (s1, s2):
        tuned = [t for t, _ in sq]
        assert tuned == sorted(tuned) and tuned[-1] == 1 and sq[-1][1] in (96, 128, 256), sq
