"""-m gpu: the TOLERANCE MODE of the fragment shaders (SRZ_OPT_APPROX_SHADE, opt-in) against the CPU oracle.

The reference's own x86 path shades with approximate instructions (_mm256_rcp_ps: include/shader/Shader.hpp:131, src/Tools.cpp:19,
include/loader/TextureLoader.hpp:99, src/Rasterizer.cpp:111; SVML _mm256_pow_ps: include/shader/Shader.hpp:195), so north_star
asks for "a stated per-channel float tolerance, z-buffer bit-exact".  The default mode is exact (test_gpu_parity.py: bit-identical
colours); this mode trades that for speed and must stay inside the tolerance SURVEY.md §8c states:

  * z plane, coverage, counters: BIT-IDENTICAL (k_raster does not change);
  * pixels of the 8-wide ("V") columns:  |colour - oracle| <= 0.5 on the 0..255 scale, every channel;
  * pixels of the scalar-tail ("S") columns (whose colours are truncated to integers): EQUAL, except where the oracle's value in front
    of the truncation lies within 1e-3 of an integer — there the truncation may land on the neighbouring integer (|Δ| = 1);
  * the resolved 8-bit image >= 99.9 % identical.
Exceptions are counted and printed, never hidden.  The oracle tells the class and the pre-truncation value of a pixel through
its test probe (oracle.debug_s)."""
import numpy as np
import pytest

import scenes
from srz import abi
from support import actx, bits, check_approx, oracle_with_probes, random_frame, same  # noqa: F401  (actx: the fixture)

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("name,build", [
    ("config2 TEXTURE", lambda: scenes.config2(7)),
    ("config2 PHONG", lambda: scenes.config2(3, shader=abi.SHADER_PHONG)),
    ("config2 NORMAL", lambda: scenes.config2(11, shader=abi.SHADER_NORMAL)),
    ("config3", lambda: scenes.config3(3)),
    ("config4", lambda: scenes.config4(2)),
    ("config5", lambda: scenes.config5(1)),
])
def test_tolerance_mode_within_the_stated_tolerance(actx, orc, name, build):
    f = build()
    ref, rst, pre, s_class = oracle_with_probes(orc, f)
    gpu, gst = actx.draw(f, want_stats=True)
    worst_v, _ = check_approx(gpu, gst, ref, rst, pre, s_class, name)
    same8 = (orc.resolve8(gpu) == orc.resolve8(ref)).all(axis=2)
    frac = float(same8.mean())
    print(f"[approx {name}] resolved 8-bit image identical on {frac:.6f} of the pixels")
    assert frac >= 0.999


@pytest.mark.parametrize("p", [0.0, 1.0, 7.5, 32.0, 150.0, 1000.5])
def test_tolerance_mode_exponents(actx, orc, p):
    """any finite exponent >= 0 goes through exp2(p log2 x) in this mode (the exact mode has three forms)"""
    f0 = scenes.config2(5, size=512)
    f = abi.Frame(512, 512, scenes.EYE, scenes.LIGHTS, [(abi.SHADER_TEXTURE, scenes.TEX_SPOT, f0.tris[0])], abi.FUSED_CLEAR, p=p)
    ref, rst, pre, s_class = oracle_with_probes(orc, f)
    gpu, gst = actx.draw(f, want_stats=True)
    check_approx(gpu, gst, ref, rst, pre, s_class, f"p={p}")


@pytest.mark.parametrize("n_lights", [1, 3, 4])
def test_tolerance_mode_light_counts(actx, orc, n_lights):
    lights = np.array([[[0.9, 0.9, -0.9], [100, 100, 100]], [[0.0, 0.8, 0.9], [50, 50, 50]], [[-0.7, 0.2, 0.5], [30, 60, 90]],
                       [[0.3, -0.9, 0.4], [80, 20, 40]]], np.float32)[:n_lights]
    f0 = scenes.config2(9, size=512)
    f = abi.Frame(512, 512, scenes.EYE, lights, [(abi.SHADER_TEXTURE, scenes.TEX_SPOT, f0.tris[0])], abi.FUSED_CLEAR)
    ref, rst, pre, s_class = oracle_with_probes(orc, f)
    gpu, gst = actx.draw(f, want_stats=True)
    check_approx(gpu, gst, ref, rst, pre, s_class, f"{n_lights} lights")


def test_frames_the_tolerance_builds_do_not_cover_stay_exact(actx, orc):
    """0 or more than 4 lights, BUMP / DISPLACEMENT batches: the exact builds shade them, bit-identically, with the option on"""
    f0 = scenes.config2(4, size=256)
    five = np.tile(scenes.LIGHTS, (3, 1, 1))[:5]
    for name, f in (("5 lights", abi.Frame(256, 256, scenes.EYE, five, [(abi.SHADER_TEXTURE, scenes.TEX_SPOT, f0.tris[0])], abi.FUSED_CLEAR)),
                    ("BUMP", abi.Frame(256, 256, scenes.EYE, scenes.LIGHTS, [(abi.SHADER_BUMP, scenes.TEX_SPOT, f0.tris[0])], abi.FUSED_CLEAR))):
        rc, ref, rst = orc.draw(f)
        gpu, gst = actx.draw(f, want_stats=True)
        assert rc == 0 and gst == rst
        for g, r in zip(gpu, ref):
            assert np.array_equal(bits(g), bits(r)), name


def test_option_is_per_frameset_and_the_default_stays_exact(orc):
    """a frameset keeps the mode it was created in; a ctx that never set the option is bit-identical to the oracle"""
    import torch
    import srz
    c = srz.Context(0)
    c.texture_upload(scenes.TEX_SPOT, scenes.spot_texture())
    f = scenes.config2(2, size=512, shader=abi.SHADER_PHONG)
    rc, ref, _ = orc.draw(f)
    exact_set = c.frameset([f])
    c.set_option(abi.OPT_APPROX_SHADE, 1)
    approx_set = c.frameset([f])
    c.set_option(abi.OPT_APPROX_SHADE, 0)
    outs = []
    for fs in (exact_set, approx_set):
        out = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
        fs.render(out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy()[0])
    assert np.array_equal(bits(outs[0]), bits(np.stack(ref)))                       # exact set: the oracle, bit for bit
    assert np.array_equal(bits(outs[1][0]), bits(ref[0]))                           # approx set: z bit-identical ...
    assert not np.array_equal(bits(outs[1][1:]), bits(np.stack(ref[1:])))           # ... colours in another arithmetic
    assert float(np.abs(outs[1][1:] - np.stack(ref[1:])).max()) <= 1.0
    gpu, _ = c.draw(f)                                                              # the ctx's own draw follows the option: off again
    assert np.array_equal(bits(np.stack(gpu)), bits(np.stack(ref)))
    exact_set.close(), approx_set.close(), c.close()


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("SRZ_FUZZ_SEEDS", "8"))))
def test_tolerance_mode_on_random_frames(orc, seed):
    """the fuzz frames of support.random_frame (random soups, every shader, 0-3 lights placed INSIDE the image, exponents 150 / 8 / 2.5,
    degenerate normals, uvs beyond [0, 1]) through a frameset in the tolerance mode: z, coverage and counters bit-identical, colours
    within the stated tolerance; frames the tolerance builds do not cover (no light, BUMP / DISPLACEMENT batches) bit-identical"""
    import torch
    import srz
    rng = np.random.default_rng(5000 + seed)
    w, h = [(64, 64), (200, 120), (97, 131), (256, 96), (33, 290), (128, 128), (320, 200), (70, 70)][seed % 8]
    flags = abi.FUSED_CLEAR | (abi.UNIFIED if seed % 3 == 2 else 0)
    frames = [random_frame(rng, w, h, int(rng.integers(1, 400)), flags) for _ in range(int(rng.integers(2, 8)))]
    ctx = srz.Context(0)
    ctx.texture_upload(0, scenes.spot_texture())
    ctx.set_option(abi.OPT_APPROX_SHADE, 1)
    fs = ctx.frameset(frames)
    out = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render(out.data_ptr(), fs.out_bytes, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, f in enumerate(frames):
        ref, rst, pre, s_class = oracle_with_probes(orc, f)
        covered = len(f.lights) >= 1 and all(int(f._batches[b].shader) in (abi.SHADER_NORMAL, abi.SHADER_TEXTURE, abi.SHADER_PHONG) for b in range(f.c.n_batches))
        if covered:
            check_approx(tuple(got[i]), rst, ref, rst, pre, s_class, f"fuzz seed {seed} frame {i}")
        else:
            same(got[i], ref, f"seed {seed} frame {i}")
    fs.close(), ctx.close()
