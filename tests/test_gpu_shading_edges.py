"""-m gpu: hostile SHADING inputs (support.hostile_shading_frame: tame geometry; uv, normals, lights, eye, ka / ks / kh / kn, the
exponent and the textures' shapes at their edges) against the CPU oracle, BIT FOR BIT on all four planes (support.same: the oracle's
planes hold no NaN — tests/test_oracle_shading_edges.py pins that and that every family reaches its edge), counters equal, through:

a. srz_draw, order-independent / SRZ_ORDERED_RASTER / SRZ_UNIFIED; every exponent of HOSTILE_EXPONENTS with 1..5 lights;
b. a frameset with one frame per BUILD KIND of k_shade (1..4 lights x integer exponent / non-integer exponent / a BUMP + DISPLACEMENT
   batch, and generic frames: 0 and 5 lights, an exponent outside the FAST ranges), the kinds mask asserted as
   tests/test_gpu_shade_kinds.py does, so every build meets every family; the same set through render_visibility + shade_visibility,
   and re-lit by update_shading with another family's lights and constants.  The tiles the FAST builds hand to the generic one
   (debug_counters' redo_tiles) are printed per family and per kind, after the colour render and after shade_visibility; a set whose
   inputs are all finite must keep some for itself, and in the families whose hostile values cannot reach a checked operand every
   kind must (KEEPS_EVERY_KIND);
c. a sceneset (the device vertex stage) for the normal and uv families, normal_m's last row making w = 0 for some normals;
d. the tolerance mode: z, counters and uncovered pixels bit-identical, colours NaN-free in [0, 255] for every family; the stated value
   bounds (support.check_approx, unchanged) where the frame is labelled finite AND the oracle's pre-truncation probe is finite at every
   covered pixel (checked on the CPU).  Of the frames below that is: every frame of uv-edge, uv-overflow, exponent and texture-shape and
   the even seeds of light-edge, eye-edge and constants; never uv-nonfinite and normal-nonfinite, nor the odd seeds of the three mixed
   families (labelled by their inputs): support.tolerance_frames states the rule, tests/test_oracle_shading_edges.py asserts it on
   the CPU, test_tolerance_mode again and prints the frames it leaves unbounded.
The frames are 64 x 64 (4 tiles), a few dozen triangles: the oracle side costs milliseconds."""
import numpy as np
import pytest
import torch

from srz import abi
from support import (HOSTILE_EXPONENTS, HOSTILE_FAMILIES, MIX_ALL, MIX_PLAIN, bits, check_approx, hostile_shading_frame, lit, make_ctx,
                     oracle_with_probes, register_hostile_textures, run, run_both, same, stream, tolerance_frames, words, xform_div_w)

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZE = 64
TILES = (SIZE // 32) ** 2
MIX_BUMPY = (abi.SHADER_TEXTURE, abi.SHADER_PHONG, abi.SHADER_BUMP, abi.SHADER_DISPLACEMENT)
# exponents by the class classify_frames puts them in (csrc/srz_api.hip): integer 0..256 / non-integer in (0, 4096] / everything else
P_INT, P_FRAC, P_OTHER = (150.0, 32.0, 0.0, 1.0, 2.0, 255.0, 256.0), (7.5, 0.5, 4095.5), (5000.0, 257.0, 4096.0, 4097.0, -1.0, 1e30, np.inf, np.nan)


@pytest.fixture(scope="module")
def hctx(orc):
    """a context (and the session's oracle) with the hostile textures beside the spot texture"""
    g = make_ctx()
    c = next(g)
    register_hostile_textures(orc, c)
    yield c
    c.close()


@pytest.fixture()
def hactx(orc):
    """a fresh context in the tolerance mode with the hostile textures"""
    g = make_ctx(approx=True)
    c = next(g)
    register_hostile_textures(orc, c)
    yield c
    c.close()


def oracle(orc, f):
    rc, ref, _ = orc.draw(f)
    assert rc == 0
    return ref


def lights_of(f):
    """frame f's lights as the [n, 2, 3] array lit() and abi.SceneFrame take"""
    return np.stack([f.lights["pos"], f.lights["intensity"]], 1)


def exponent_of(family, form, i):
    """the cell's exponent: the plain one of its class; the exponent family walks the class's edges"""
    ps = {"int": P_INT, "frac": P_FRAC, "other": P_OTHER}[form]
    return ps[i % len(ps)] if family == "exponent" else ps[i % 2 if form == "int" else 0]


# ------------------------------------------------------------------------------------------------ a. srz_draw
@pytest.mark.parametrize("family", HOSTILE_FAMILIES)
def test_draw_paths(hctx, orc, family):
    for seed in (0, 1, 2, 3):
        for extra in (0, abi.ORDERED_RASTER, abi.UNIFIED):
            p = (P_INT + P_FRAC + P_OTHER)[(5 * seed + extra) % 18] if family == "exponent" else (150.0, 7.5, 5000.0)[seed % 3]
            f = hostile_shading_frame(seed, family, MIX_ALL, 1 + (seed + extra) % 5, p, SIZE, SIZE, flags=abi.FUSED_CLEAR | extra)
            what = f"{family} seed {seed} flags+={extra} p={p}"
            gpu, ref = run_both(hctx, orc, f, what=what)
            same(gpu, ref, what)


@pytest.mark.parametrize("p", HOSTILE_EXPONENTS, ids=[repr(p) for p in HOSTILE_EXPONENTS])
def test_every_exponent(hctx, orc, p):
    """every exponent of the list (NaN, inf, the values at and past the FAST ranges' edges included) with 1..5 lights, cosines near 0
    and near 1 in every frame (the exponent family), through srz_draw and as the exponent a live set is re-lit to"""
    frames = [hostile_shading_frame(n, "exponent", MIX_ALL if n % 2 else MIX_PLAIN, n, p, SIZE, SIZE) for n in (1, 2, 3, 4, 5)]
    for f in frames:
        what = f"exponent p={p!r} {f.c.n_lights} lights"
        gpu, ref = run_both(hctx, orc, f, what=what)
        same(gpu, ref, what)
    fs = hctx.frameset([lit(f, p=150.0) for f in frames])
    fs.update_shading(frames)
    hctx.sync()
    col, out, _ = run(fs)
    for i, f in enumerate(frames):
        same(col.view(np.float32)[i], oracle(orc, f), f"set re-lit to p={p!r}: frame {i}")
    same(out.swapaxes(0, 1), col.swapaxes(0, 1), f"set re-lit to p={p!r}: shade_visibility against the colour render")
    fs.close()


# ------------------------------------------------------------------------------------------------ b. every build kind
def kind_cells():
    """(lights, exponent class, shader mix) of the set's frames: kinds 0..3, 8..11, 4..7, then three generic frames"""
    cells = [(n, form, mix) for form, mix in (("int", MIX_PLAIN), ("frac", MIX_PLAIN), ("int", MIX_BUMPY)) for n in (1, 2, 3, 4)]
    return cells + [(0, "int", MIX_PLAIN), (5, "int", MIX_BUMPY), (2, "other", MIX_PLAIN)]


def kind_frames(family, parity):
    return [hostile_shading_frame(2 * i + parity, family, mix, n, exponent_of(family, form, i), SIZE, SIZE)
            for i, (n, form, mix) in enumerate(kind_cells())]


KIND_OF_CELL = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7)  # the build kind of the set's first twelve frames (kind_cells' order)
# Families whose hostile values cannot reach an operand the FAST builds check (the tracked reciprocals / square roots / divisions take
# positions, normals, lights and the eye, never uv or a texel; the exponents of these frames are plain): EVERY kind must keep a tile
# of its own frame.  For the other families a single finite value (a light or a constant of 1e30, a light on a pixel) legitimately
# sends every tile of its frame to the generic build, so only the set as a whole is bounded, as the figures printed per kind show.
KEEPS_EVERY_KIND = ("uv-edge", "uv-overflow", "texture-shape")


def handed_over(ctx, f):
    """(redo_tiles after the colour render, after shade_visibility) of frame f as a set of its own"""
    fs = ctx.frameset([f])
    col = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    vis, out = torch.zeros_like(col), torch.zeros_like(col)
    fs.render(col.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
    r_col = fs.debug_counters()["redo_tiles"]
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
    fs.shade_visibility(vis.data_ptr(), out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
    r_vis = fs.debug_counters()["redo_tiles"]
    fs.close()
    return r_col, r_vis


@pytest.mark.parametrize("parity", [0, 1], ids=["even-seeds", "odd-seeds"])
@pytest.mark.parametrize("family", HOSTILE_FAMILIES)
def test_every_build_kind(hctx, orc, family, parity):
    frames = kind_frames(family, parity)
    fs = hctx.frameset(frames)
    assert fs.shade_kinds() == (0xfff, True), f"{family}: kinds {fs.shade_kinds()}"
    col, out, vis = run(fs)
    redo = fs.debug_counters()["redo_tiles"]
    fast_tiles = 12 * TILES
    labels = sorted({f.label for f in frames[:12]})  # (of the frames the FAST builds shade)
    per_kind = [handed_over(hctx, f) for f in frames[:12]]  # (frame i of the set is the frame of kind KIND_OF_CELL[i])
    print(f"[{family} {'odd' if parity else 'even'} seeds] kinds mask={fs.shade_kinds()[0]:#05x} generic={fs.shade_kinds()[1]} labels={labels} "
          f"tiles handed to the generic build: {redo} of {fast_tiles} tiles of FAST frames (the set, after shade_visibility); per kind, of "
          f"{TILES} tiles each, (colour render, shade_visibility): " + " ".join(f"{k}:{r}" for k, r in zip(KIND_OF_CELL, per_kind)))
    for i, f in enumerate(frames):
        same(col.view(np.float32)[i], oracle(orc, f), f"{family} kinds frame {i} ({f.c.n_lights} lights, p={f.c.p}, {f.label})")
    same(out.swapaxes(0, 1), col.swapaxes(0, 1), f"{family}: shade_visibility against the colour render")
    assert (words(vis)[:, 1] != 0).any()
    if labels == ["finite"]:
        assert redo < fast_tiles, f"{family}: every tile of the FAST builds went to the generic build: they were not tested"
    if family in KEEPS_EVERY_KIND:
        for k, (r_col, r_vis) in zip(KIND_OF_CELL, per_kind):
            assert r_col < TILES and r_vis < TILES, f"{family}: the FAST build of kind {k} handed every tile over: it was not tested"
    # re-lit with another family's lights, constants and exponent: the OLD visibility buffer shades to the oracle's new picture
    other = "constants" if family == "light-edge" else "light-edge"
    donors = kind_frames(other, 1 - parity)
    relit = [lit(f, lights_of(d), ka=tuple(d.c.ka), ks=tuple(d.c.ks), p=d.c.p, kh=d.c.kh, kn=d.c.kn) for f, d in zip(frames, donors)]
    fs.update_shading(relit)
    hctx.sync()
    col2, out2 = torch.zeros_like(vis), torch.zeros_like(vis)
    fs.render(col2.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
    fs.shade_visibility(vis.data_ptr(), out2.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
    torch.cuda.synchronize()
    for i, f in enumerate(relit):
        same(words(out2).view(np.float32)[i], oracle(orc, f), f"{family} re-lit by {other}: shade_visibility frame {i}")
    same(words(col2).swapaxes(0, 1), words(out2).swapaxes(0, 1), f"{family} re-lit by {other}: the colour render")
    fs.close()


# ------------------------------------------------------------------------------------------------ c. the device vertex stage
@pytest.mark.parametrize("family", ["normal-nonfinite", "uv-nonfinite", "uv-edge", "uv-overflow"])
def test_sceneset_vertex_stage(hctx, orc, family):
    """meshes whose vertices carry the hostile attributes; ndc_mvp is the identity (the positions pass unchanged), normal_m is the
    identity with the last row (0, 0, 1, -1): w = nz - 1, zero for the normals that are exactly (0, 0, 1) — to_vec3 divides by it"""
    ident = np.eye(4, dtype=F32).reshape(16)
    nm = ident.copy()
    nm[2 * 4 + 3], nm[3 * 4 + 3] = 1.0, -1.0
    sframes, hframes, slot = [], [], 0
    for seed in (0, 1):
        f = hostile_shading_frame(seed, family, MIX_PLAIN, 2 + seed, (150.0, 7.5)[seed], SIZE, SIZE)
        draws, batches = [], []
        for b, t in enumerate(f.tris):
            v = np.zeros((3 * len(t), 8), F32)
            v[:, 0:3], v[:, 3:6], v[:, 6:8] = t["pos"].reshape(-1, 3), t["nrm"].reshape(-1, 3), t["uv"].reshape(-1, 2)
            v[::5, 3:6] = (0.0, 0.0, 1.0)  # w = 0 for these
            hctx.mesh_upload(slot, v, np.arange(3 * len(t), dtype=np.uint32).reshape(-1, 3))
            sh, tex = f._batches[b].shader, f._batches[b].tex_id
            draws.append((slot, sh, tex, ident, nm))
            ht = t.copy()
            ht["pos"] = xform_div_w(ident, v[:, 0:3]).reshape(-1, 3, 3)
            ht["nrm"] = xform_div_w(nm, v[:, 3:6]).reshape(-1, 3, 3)
            assert np.array_equal(bits(ht["pos"]), bits(t["pos"])) and np.isnan(ht["nrm"][0, 0, 0]) and np.isinf(ht["nrm"][0, 0, 2])
            batches.append((sh, tex, ht))
            slot += 1
        c = f.c
        args = dict(ka=tuple(c.ka), ks=tuple(c.ks), p=c.p, kh=c.kh, kn=c.kn)
        sframes.append(abi.SceneFrame(SIZE, SIZE, tuple(c.eye), lights_of(f), draws, 1.0, 0.0, abi.FUSED_CLEAR, **args))
        hframes.append(abi.Frame(SIZE, SIZE, tuple(c.eye), f.lights, batches, abi.FUSED_CLEAR, **args))
    outs = []
    for fr in (hframes, sframes):
        fs = hctx.frameset(fr)
        col, out, _ = run(fs)
        same(out.swapaxes(0, 1), col.swapaxes(0, 1), f"{family}: shade_visibility against the colour render")
        outs.append(col.view(np.float32))
        fs.close()
    same(outs[1].swapaxes(0, 1), outs[0].swapaxes(0, 1), f"{family}: the sceneset against the frameset of the numpy vertex stage")
    for i, f in enumerate(hframes):
        same(outs[1][i], oracle(orc, f), f"{family}: sceneset frame {i} against the oracle")


# ------------------------------------------------------------------------------------------------ d. the tolerance mode
@pytest.mark.parametrize("family", HOSTILE_FAMILIES)
def test_tolerance_mode(hactx, orc, family):
    n_bounded = 0
    for name, f, bounded in tolerance_frames(family, SIZE):
        ref, rst, pre, s_class = oracle_with_probes(orc, f)
        gpu, gst = hactx.draw(f, want_stats=True)
        assert gst == rst, (name, gst, rst)
        assert np.array_equal(bits(gpu[0]), bits(ref[0])), f"{name}: z plane"
        cov = np.isfinite(ref[0])
        for ch in (1, 2, 3):
            assert np.array_equal(bits(gpu[ch][~cov]), bits(ref[ch][~cov])), f"{name}: uncovered pixels"
            assert not np.isnan(gpu[ch]).any(), f"{name}: NaN in colour plane {ch}"
            assert ((gpu[ch][cov] >= 0.0) & (gpu[ch][cov] <= 255.0)).all(), f"{name}: colour outside [0, 255]"
        finite_pre = all(np.isfinite(q[cov]).all() for q in pre[1:])
        assert bounded == (f.label == "finite" and finite_pre), (name, f.label, finite_pre)
        if bounded:
            check_approx(gpu, gst, ref, rst, pre, s_class, name)
            n_bounded += 1
        else:
            print(f"[approx {name}] unbounded: label {f.label}, pre-truncation probe finite: {finite_pre}")
        if "all" in name.split():
            same(gpu, ref, f"{name}: a frame with a BUMP batch keeps the exact build")
    print(f"[approx {family}] value bounds asserted on {n_bounded} of 8 frames")
