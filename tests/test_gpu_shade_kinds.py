"""Every build kind of k_shade / k_shade_vis against the CPU oracle, with the proof of which build ran (FrameSet.shade_kinds()).

The exact mode has thirteen separately compiled builds per kernel (csrc/srz_device.h: kinds 0..3 = 1..4 lights with an integer exponent,
4..7 = the same with a BUMP / DISPLACEMENT batch, 8..11 = 1..4 lights with pow_fast, 12 = generic), each with a grey and a coloured
path; the tolerance mode has four more.  classify_frames picks the kind on the host.  Here every kind shades a frame through both
entry points (the colour render, and render_visibility + shade_visibility), every frame is compared WITH THE ORACLE through
support.compare() (bit-identical z, |Δcolour| <= 1e-3 on <= 1e-5 of the covered pixels; the count of colour words that are
not bit-identical is printed), and the kinds a set reports are compared with the rule written out below.  The tests without the gpu
mark check on the CPU that the inputs can tell a wrong build from a right one: the pictures are not saturated, dropping the last
light or swapping the last two intensities changes them, the exponents of the boundary cases give finite planes, and the frames of
the hand-back case have pixels inside pow_fast's flagged interval."""
import math

import numpy as np
import pytest
import torch

import scenes
from srz import abi
from support import changed, check_approx, compare, ctx, lit, oracle_with_probes, run, same, stream, words  # noqa: F401  (ctx: the fixture)

gpu = pytest.mark.gpu

SIZE = 256
GENERIC = 12
SHADERS = {"NORMAL": abi.SHADER_NORMAL, "TEXTURE": abi.SHADER_TEXTURE, "PHONG": abi.SHADER_PHONG, "BUMP": abi.SHADER_BUMP,
           "DISPLACEMENT": abi.SHADER_DISPLACEMENT}
BUMPY = (abi.SHADER_BUMP, abi.SHADER_DISPLACEMENT)

# ---- the rule (csrc/srz_device.h "k_shade builds", csrc/srz_api.hip "Which frames the FAST builds of k_shade can shade"), written out:
# 1..4 lights and an integer exponent 0..256 -> kind lights - 1, + 4 with a BUMP / DISPLACEMENT batch; 1..4 lights and a non-integer
# exponent in (0, 4096] -> kind 8 + lights - 1, but generic with a BUMP / DISPLACEMENT batch; everything else generic.
FORM_OF_P = {150.0: "int", 32.0: "int", 7.5: "frac", 5000.0: "other"}  # (150: the fixed chain, 32: the scalar integer loop)
FIRST_KIND = {("int", False): 0, ("int", True): 4, ("frac", False): 8}  # (form, bumpy) -> the kind of ONE light; absent: generic


def kind_of(n_lights, form, bumpy):
    if not 1 <= n_lights <= 4 or (form, bumpy) not in FIRST_KIND:
        return GENERIC
    return FIRST_KIND[(form, bumpy)] + n_lights - 1


def kinds_of(cells):
    """(mask, any_generic) of a set whose frames are the (n_lights, form, bumpy) of cells"""
    ks = [kind_of(*c) for c in cells]
    return sum({1 << k for k in ks if k != GENERIC}), GENERIC in ks


# ---- the lights.  The shaders take a light's position in the space of the fragment's (x, y, z) = (pixel column, pixel row, depth):
# the spot of config 2 at 256^2 covers x 60..167, y 52..197, z 84..90, the eye sits at (0, 0, 0.9), and the visible normals point
# to +z.  Five lights outside the image on different sides, at depths beyond the mesh (so that the diffuse and the specular term of
# every light are alive: the README's two lights, at z = -0.9 and 0.9, leave most pixels with the ambient term alone), with distinct
# intensities small enough that four of them do not saturate a channel (the attenuation is 1 / the distance in x and y, about
# 1 / 150: ambient + diffuse of one light is about 0.01 * intensity).
LIGHT_POS = np.array([[0.9, 0.9, 400.0], [300.0, 20.0, 350.0], [-40.0, 300.0, 500.0], [280.0, 290.0, 300.0], [128.0, -60.0, 450.0]], np.float32)
LIGHT_GREY = np.array([22.0, 13.0, 17.0, 9.0, 11.0], np.float32)
TINT = np.array([0.5, 1.0, 1.5], np.float32)  # the coloured variant of a light: its grey intensity times this


def lights(n, grey, size=SIZE):
    """n of the five lights; coloured: the LAST one has unequal channels (the grey test of classify_frames has to reach it)"""
    L = np.zeros((n, 2, 3), np.float32)
    L[:, 0] = LIGHT_POS[:n] * np.array([size / SIZE, size / SIZE, 1.0], np.float32)
    L[:, 1] = LIGHT_GREY[:n, None]
    if not grey and n:
        L[-1, 1] *= TINT
    return L


def base(a, shader, size=SIZE):
    return scenes.config2(a, size=size, shader=shader)


def matrix_cells():
    return [(n, p) for n in (1, 2, 3, 4) for p in (150.0, 32.0, 7.5, 5000.0)]


def matrix_frames(shader, grey):
    return [lit(base(3 + 2 * i, shader), lights(n, grey), p=p) for i, (n, p) in enumerate(matrix_cells())]


def planes(w):
    """[frames, 4, H, W] uint32 words as float32 planes"""
    return w.view(np.float32)


def oracle(orc, f):
    rc, ref, _ = orc.draw(f)
    assert rc == 0
    return ref


SEEN = {"render": [0, False], "shade_visibility": [0, False]}  # the union of the kinds every passed set has reported, per entry point


def both_ways_against_the_oracle(ctx, orc, frames, expect, what, count=True):
    """the set reports `expect`; its colour render and the shade of its visibility render are the same words; every frame is the
    oracle's.  Returns the number of colour words that are not bit-identical to the oracle's."""
    fs = ctx.frameset(frames)
    assert fs.shade_kinds() == expect, f"{what}: kinds {fs.shade_kinds()} expected {expect}"
    col, out, vis = run(fs)
    n_diff = 0
    for i, f in enumerate(frames):
        n_diff += compare(planes(col)[i], oracle(orc, f), f"{what} frame {i} ({f.c.n_lights} lights, p={f.c.p})")
    if count:
        SEEN["render"][0] |= expect[0]
        SEEN["render"][1] |= expect[1]
    same(out.swapaxes(0, 1), col.swapaxes(0, 1), f"{what}: shade_visibility against the colour render")
    assert (words(vis)[:, 1] != 0).any(), f"{what}: nothing drawn"
    if count:
        SEEN["shade_visibility"][0] |= expect[0]
        SEEN["shade_visibility"][1] |= expect[1]
    fs.close()
    print(f"[{what}] kinds mask={expect[0]:#05x} generic={expect[1]} colour_words_not_bit_identical={n_diff}")
    return n_diff


# ------------------------------------------------------------------------------------------------ a. the kind matrix
@pytest.mark.parametrize("shader", ["TEXTURE", "PHONG", "BUMP", "DISPLACEMENT"])
@pytest.mark.parametrize("grey", [True, False], ids=["grey", "coloured"])
def test_matrix_inputs_tell_a_wrong_light_from_a_right_one(orc, shader, grey):
    """(CPU) the oracle's picture of every lit cell is not saturated, loses > 20 % of its pixels' colours when the last light is dropped
    and > 20 % when the last light takes its neighbour's intensity: a build that drops or swaps a light cannot pass compare().
    (NORMAL ignores the lights; its cells pin the build's normal path and the work lists.)"""
    for i, (n, p) in enumerate(matrix_cells()):
        L = lights(n, grey)
        f = lit(base(3 + 2 * i, SHADERS[shader]), L, p=p)
        ref = oracle(orc, f)
        cov = np.isfinite(ref[0])
        if SHADERS[shader] in BUMPY:  # (the 8-wide columns of these two are the reference's empty stubs: white)
            cov = cov & ~((ref[1] == 255.0) & (ref[2] == 255.0) & (ref[3] == 255.0))
        inside = cov & np.logical_and.reduce([(c > 0.0) & (c < 255.0) for c in ref[1:]])
        assert inside.sum() > 0.5 * cov.sum(), (shader, n, p, int(inside.sum()), int(cov.sum()))
        other = L.copy()
        other[-1, 1] = (LIGHT_GREY[n] if grey else LIGHT_GREY[n] * TINT[::-1])  # (the next light's intensity / the tint reversed)
        assert changed(ref, oracle(orc, lit(f, other))) > 0.2, (shader, n, p)
        assert changed(ref, oracle(orc, lit(f, L[:-1]))) > 0.2, (shader, n, p)


@gpu
@pytest.mark.parametrize("shader", list(SHADERS))
@pytest.mark.parametrize("grey", [True, False], ids=["grey", "coloured"])
def test_kind_matrix(ctx, orc, shader, grey):
    """1..4 lights x {150, 32, 7.5, 5000} in ONE set per (shader, colour): 16 frames of up to 9 kinds, so every render also walks
    several work lists and launches several builds.  BUMP / DISPLACEMENT with p = 7.5 is generic by design."""
    sh = SHADERS[shader]
    bumpy = sh in BUMPY
    cells = [(n, FORM_OF_P[p], bumpy) for n, p in matrix_cells()]
    expect = kinds_of(cells)
    if bumpy:
        assert expect == (0xf0, True) and all(kind_of(n, "frac", True) == GENERIC for n in (1, 2, 3, 4))
    else:
        assert expect == (0xf0f, True)
    both_ways_against_the_oracle(ctx, orc, matrix_frames(sh, grey), expect, f"matrix {shader} {'grey' if grey else 'coloured'}")


@gpu
def test_matrix_reached_every_kind_through_both_entry_points():
    """completeness is a condition: the sets of test_kind_matrix that passed have reported all of kinds 0..11 and the generic build,
    for the colour render and for shade_visibility (run after test_kind_matrix, in the same process)"""
    print({k: (hex(m), g) for k, (m, g) in SEEN.items()})
    for entry, (mask, generic) in SEEN.items():
        assert mask == 0xfff and generic, f"{entry}: kinds seen {mask:#05x}, generic {generic}"


# ------------------------------------------------------------------------------------------------ b. FD_GREY edges
def grey_edge_frames():
    frames, names = [], []
    for n in (2, 4):
        for a, sh in ((5, abi.SHADER_PHONG), (8, abi.SHADER_TEXTURE)):
            f, g = base(a, sh), lights(n, True)
            last = lights(n, False)
            neg = g.copy()
            neg[-1, 1] = np.array([0.0, -0.0, 0.0], np.float32)
            black = g.copy()
            black[:, 1] = 0.0
            for name, fr in (("ka", lit(f, g, ka=(0.005, 0.005, 0.02))), ("ks", lit(f, g, ks=(0.7937, 0.7937, 0.4))),
                             ("last light", lit(f, last)), ("-0.0", lit(f, neg)), ("black", lit(f, black))):
                frames.append(fr), names.append(f"{name}, {n} lights, shader {sh}")
    return frames, names


def test_grey_edges_are_what_they_say():
    frames, names = grey_edge_frames()
    for f, name in zip(frames, names):
        I = np.stack([f.lights["intensity"][i] for i in range(len(f.lights))]).view(np.uint32)
        ka, ks = np.float32(list(f.c.ka)).view(np.uint32), np.float32(list(f.c.ks)).view(np.uint32)
        grey = [len(set(ka.tolist())) == 1, len(set(ks.tolist())) == 1] + [len(set(r.tolist())) == 1 for r in I]
        if name.startswith("black"):
            assert all(grey) and not I.any()
        else:  # exactly one of ka, ks, the lights is not grey: ka, ks, or the LAST light
            assert grey.count(False) == 1 and grey.index(False) == {"ka": 0, "ks": 1}.get(name.split(",")[0], len(grey) - 1), name
        if name.startswith("-0.0"):
            assert I[-1].tolist() == [0, 0x80000000, 0] and (f.lights["intensity"][-1] == 0).all()


@gpu
def test_grey_edges(ctx, orc):
    """one channel of ka / of ks / of the last light only / a -0.0 beside +0.0 (equal as numbers, not as bits) breaks FD_GREY; all lights
    black keeps it: 2 and 4 lights, PHONG and TEXTURE, one set"""
    frames, _ = grey_edge_frames()
    both_ways_against_the_oracle(ctx, orc, frames, (1 << 1 | 1 << 3, False), "FD_GREY edges", count=False)


# ------------------------------------------------------------------------------------------------ c. exponent boundaries
BOUNDARY = [(0.0, "int"), (-0.0, "int"), (1.0, "int"), (255.0, "int"), (256.0, "int"), (257.0, "other"),
            (0.001, "frac"), (255.5, "frac"), (4095.5, "frac"), (4096.5, "other"),
            (-2.0, "other"), (math.inf, "other"), (math.nan, "other")]
BOUNDARY_IDS = [repr(p) for p, _ in BOUNDARY]


@pytest.mark.parametrize("p,form", BOUNDARY, ids=BOUNDARY_IDS)
def test_oracle_takes_every_boundary_exponent(orc, p, form):
    """(CPU) the oracle draws each of them (rc 0) and its final clamp leaves finite colours, so compare()'s arithmetic can express
    every cell; the exponent reaches the frame as the binary32 it names (the sign of -0.0 included)"""
    for n in (2, 4):
        f = lit(base(6, abi.SHADER_PHONG), lights(n, False), p=p)
        assert np.float32(f.c.p).view(np.uint32) == np.float32(p).view(np.uint32) or (math.isnan(p) and math.isnan(f.c.p))
        ref = oracle(orc, f)
        assert all(np.isfinite(c).all() for c in ref[1:]), (p, n)
        assert np.isfinite(ref[0]).sum() > 5000


@gpu
@pytest.mark.parametrize("p,form", BOUNDARY, ids=BOUNDARY_IDS)
def test_exponent_boundaries(ctx, orc, p, form):
    """the edges of classify_frames' three exponent classes, PHONG, 2 and 4 lights, single-frame sets"""
    for n in (2, 4):
        k = kind_of(n, form, False)
        expect = (0, True) if k == GENERIC else (1 << k, False)
        both_ways_against_the_oracle(ctx, orc, [lit(base(6, abi.SHADER_PHONG), lights(n, False), p=p)], expect,
                                     f"p={p!r} {n} lights", count=False)


# ------------------------------------------------------------------------------------------------ d. GENPOW's hand-back
P_RING = 1000.7  # pow_fast flags results in [2^-151, 2^-120): cosines in [2^(-151/p), 2^(-120/p)) = about [0.9007, 0.9202)


def ring_frames(n):
    return [lit(base(a, abi.SHADER_PHONG), lights(n, True), p=P_RING) for a in (4, 22)]


def ring_pixels(orc, f):
    """per light: the covered pixels whose Blinn-Phong cosine n.h lies well inside the flagged interval.  n: the oracle's NORMAL
    render of the same triangles ((n + 1) / 2 * 255, truncated to integers in the scalar columns: an error below 0.01 in the cosine,
    hence the margin); the fragment's position is (column, row, z)"""
    ref = oracle(orc, lit(f, batches=[(abi.SHADER_NORMAL, -1, f.tris[0])]))
    cov = np.isfinite(ref[0])
    n = np.stack([c.astype(np.float64) / 255.0 * 2.0 - 1.0 for c in ref[1:]], -1)
    n /= np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-30)
    ys, xs = np.mgrid[0:f.height, 0:f.width]
    P = np.stack([xs.astype(np.float64), ys.astype(np.float64), np.where(cov, ref[0], 0.0).astype(np.float64)], -1)
    eye = np.array(list(f.c.eye), np.float64)
    lo, hi = 2.0 ** (-151.0 / P_RING) + 0.004, 2.0 ** (-120.0 / P_RING) - 0.004
    counts = []
    for l in f.lights:
        h = (l["pos"].astype(np.float64) - P) + (eye - P)
        h /= np.linalg.norm(h, axis=-1, keepdims=True)
        c = (n * h).sum(-1)
        counts.append(int((cov & (c > lo) & (c < hi)).sum()))
    return counts


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_ring_frames_have_pixels_inside_the_flagged_interval(orc, n):
    """(CPU) before relying on the ring: some frame of the case has it around the highlight of EVERY one of its lights, the last included"""
    counts = [ring_pixels(orc, f) for f in ring_frames(n)]
    print(f"[ring] {n} lights: pixels with n.h inside the flagged interval, per frame and light: {counts}")
    for l in range(n):
        assert max(c[l] for c in counts) >= 32, (n, l, counts)


@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_genpow_hands_flagged_tiles_back_at_every_light_count(ctx, orc, n):
    """kinds 8..11: a flagged power sends the tile to the generic build's redo list, from k_shade and from k_shade_vis; the result is
    the oracle's"""
    frames = ring_frames(n)
    fs = ctx.frameset(frames)
    assert fs.shade_kinds() == (1 << (8 + n - 1), False)
    col = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    vis, out = torch.zeros_like(col), torch.zeros_like(col)
    s = stream()
    fs.render(col.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    redo_render = fs.debug_counters()["redo_tiles"]
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    fs.shade_visibility(vis.data_ptr(), out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    redo_shade = fs.debug_counters()["redo_tiles"]
    torch.cuda.synchronize()
    print(f"[hand-back] {n} lights: redo_tiles after the colour render {redo_render}, after shade_visibility {redo_shade}")
    assert redo_render >= 1, "no tile was handed back by the colour render: the test does not reach pow_fast's flag"
    assert redo_shade >= 1, "no tile was handed back by shade_visibility: the test does not reach pow_fast's flag"
    assert np.array_equal(words(col), words(out))
    for i, f in enumerate(frames):
        compare(col[i].cpu().numpy(), oracle(orc, f), f"hand-back {n} lights frame {i}")
    fs.close()


# ------------------------------------------------------------------------------------------------ e. kind transitions on a live set
def walk():
    """the five shadings of the walk for 4 lights: (name, p, grey, intensity scale, bump the first frame, kind of an un-bumped frame)"""
    return [("kind 3", 150.0, False, 1.0, False, 3), ("kind 11", 7.5, False, 0.8, False, 11), ("generic", 5000.0, False, 1.2, False, GENERIC),
            ("kind 7", 32.0, False, 0.9, True, 3), ("kind 3 grey", 150.0, True, 1.1, False, 3)]


def walk_lights(grey, scale, size=SIZE):
    L = lights(4, grey, size)
    L[:, 1] *= np.float32(scale)
    return L


def walk_expect(kind, bump):
    mask = (1 << kind if kind != GENERIC else 0) | (1 << 7 if bump else 0)
    return mask, kind == GENERIC


@gpu
def test_kind_transitions_through_update_shading(ctx, orc):
    """one live set of two frames (4 lights, PHONG and TEXTURE) walked generic -> 3 -> 11 -> generic -> 7 (+ 3) -> 3 grey: after each
    update the set reports the new kinds, renders the oracle's picture of the NEW frames, and shades the visibility buffer rendered
    before the first update to the same words"""
    f0, f1 = base(7, abi.SHADER_PHONG), base(12, abi.SHADER_TEXTURE)
    fs = ctx.frameset([lit(f0, walk_lights(True, 1.0), p=5000.0), lit(f1, walk_lights(True, 1.0), p=5000.0)])
    assert fs.shade_kinds() == (0, True)
    s = stream()
    vis = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    torch.cuda.synchronize()
    for name, p, grey, scale, bump, kind in walk():
        L = walk_lights(grey, scale)
        new = [lit(f0, L, p=p, batches=[(abi.SHADER_BUMP if bump else abi.SHADER_PHONG, scenes.TEX_SPOT, f0.tris[0])]), lit(f1, L, p=p)]
        fs.update_shading(new)
        ctx.sync()
        assert fs.shade_kinds() == walk_expect(kind, bump), (name, fs.shade_kinds())
        col, out = torch.zeros_like(vis), torch.zeros_like(vis)
        fs.render(col.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
        fs.shade_visibility(vis.data_ptr(), out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
        torch.cuda.synchronize()
        for i, f in enumerate(new):
            compare(col[i].cpu().numpy(), oracle(orc, f), f"walk step {name} frame {i}")
        assert np.array_equal(words(out), words(col)), name
    fs.close()


@gpu
def test_kind_transitions_through_the_cached_set_of_draw(orc):
    """the same five shadings in a row through srz_draw, whose one-frame set is reused while the structure stays (the BUMP step changes
    a batch's shader, so that step and the one after it rebuild the set)"""
    import srz
    c = srz.Context(0)
    c.texture_upload(scenes.TEX_SPOT, scenes.spot_texture())
    for a, sh in ((7, abi.SHADER_PHONG), (12, abi.SHADER_TEXTURE)):
        f0 = base(a, sh)
        for name, p, grey, scale, bump, _ in walk():
            f = lit(f0, walk_lights(grey, scale), p=p, batches=[(abi.SHADER_BUMP if bump else sh, scenes.TEX_SPOT, f0.tris[0])])
            got, _ = c.draw(f)
            compare(np.stack(got), oracle(orc, f), f"draw walk shader {sh} step {name}")
    c.close()


@gpu
def test_kind_transitions_through_sceneset_update(ctx, orc):
    """the walk on a sceneset of four lights (the device's vertex stage feeds both entry points), re-lit by srz_sceneset_update; the
    oracle draws the host-built stream of the same frames (the vertex stage's stream is that stream bit for bit:
    tests/test_gpu_visibility.py::test_sceneset_ids_are_draw_offset_plus_face)"""
    import srz
    from srz import scenes as pscenes
    size = 512
    four = [tuple(map(tuple, l)) for l in lights(4, True, size).tolist()]
    wl = pscenes.spot_texture_1024(size=size, name="spot_texture_512_4lights", lights=four, p=5000.0)
    wl.upload_meshes(ctx)
    idx = (2, 15)
    sfs = [wl.scene_frame(i) for i in idx]
    hfs = [wl.frame(i) for i in idx]
    assert all(sf.c.n_lights == 4 for sf in sfs)
    fs = ctx.frameset(sfs)
    assert fs.shade_kinds() == (0, True)
    s = stream()
    vis = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
    torch.cuda.synchronize()
    for name, p, grey, scale, bump, kind in walk():
        L = walk_lights(grey, scale, size)
        sh = abi.SHADER_BUMP if bump else abi.SHADER_TEXTURE
        for sf in sfs:
            sf.lights = np.ascontiguousarray(L.reshape(-1, 6)).view(abi.LIGHT_DTYPE).reshape(-1)
            sf.c.lights = sf.lights.ctypes.data
            sf.c.p = p
        sfs[0]._draws[0].shader = sh
        ctx._check(srz.lib().srz_sceneset_update(ctx.h, fs.h, abi.scene_frames_array(sfs), len(sfs)))
        ctx.sync()
        assert fs.shade_kinds() == walk_expect(kind, bump), (name, fs.shade_kinds())
        col, out = torch.zeros_like(vis), torch.zeros_like(vis)
        fs.render(col.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
        fs.shade_visibility(vis.data_ptr(), out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)
        torch.cuda.synchronize()
        for i, hf in enumerate(hfs):
            f = lit(hf, L, p=p, batches=[(sh if i == 0 else abi.SHADER_TEXTURE, scenes.TEX_SPOT, hf.tris[0])])
            compare(col[i].cpu().numpy(), oracle(orc, f), f"sceneset walk step {name} frame {idx[i]}")
        assert np.array_equal(words(out), words(col)), name
    fs.close()


# ------------------------------------------------------------------------------------------------ f. the tolerance mode
@gpu
def test_tolerance_mode_uses_the_plain_kinds_only(orc):
    """SRZ_OPT_APPROX_SHADE: 1..4 lights with p = 150 or 7.5 go to kinds 0..3 (its four builds), never to 8..11; a BUMP frame, five
    lights and no light keep the exact generic build — checked with support.check_approx, its tolerance unchanged"""
    import srz
    c = srz.Context(0)
    c.set_option(abi.OPT_APPROX_SHADE, 1)
    c.texture_upload(scenes.TEX_SPOT, scenes.spot_texture())
    fast = [lit(base(2 + i, (abi.SHADER_TEXTURE, abi.SHADER_PHONG)[i % 2]), lights(n, i % 3 == 0), p=p)
            for i, (n, p) in enumerate((n, p) for n in (1, 2, 3, 4) for p in (150.0, 7.5))]
    exact = [lit(base(9, abi.SHADER_BUMP), lights(2, True)), lit(base(10, abi.SHADER_TEXTURE), lights(5, False)),
             lit(base(11, abi.SHADER_PHONG), lights(0, True))]
    for n in (1, 2, 3, 4):
        for p in (150.0, 7.5):
            one = c.frameset([lit(base(1, abi.SHADER_PHONG), lights(n, True), p=p)])
            assert one.shade_kinds() == (1 << (n - 1), False), (n, p, one.shade_kinds())
            one.close()
    for frames, expect, what in ((fast, (0xf, False), "fast"), (exact, (0, True), "exact"), (fast + exact, (0xf, True), "mixed")):
        fs = c.frameset(frames)
        assert fs.shade_kinds() == expect, (what, fs.shade_kinds())
        out = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
        fs.render(out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for i, f in enumerate(frames):
            ref, rst, pre, s_class = oracle_with_probes(orc, f)
            check_approx(tuple(got[i]), rst, ref, rst, pre, s_class, f"approx {what} frame {i}")
            if f in exact:
                assert np.array_equal(got[i].view(np.uint32), np.stack(ref).view(np.uint32)), (what, i)
        fs.close()
    c.close()
