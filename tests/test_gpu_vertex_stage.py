"""-m gpu: the device vertex stage (k_vertex = Scene::loadTriangleStream on the GPU): meshes resident
in HBM + per-frame matrices must give the same framebuffer, bit for bit, as host-built post-MVP streams and the oracle.

Beyond the workloads' own matrices (the first test), every frame below is built both ways by support.scene_pair: an abi.SceneFrame of
mesh slots and matrices, and an abi.Frame of the numpy vertex stage's triangles (tests/test_vertex_stage_ref.py pins that restatement
to the oracle's orc_vertex_stage on the CPU).  The sceneset's planes are compared with the frameset of the numpy triangles on the GPU
and with the oracle's draw of that Frame, bit for bit (support.same); there is no tolerance in this module.  A sceneset rendered
WITHOUT stats goes k_vertex(bbox_out) -> k_chunks -> bucket_group(P = nullptr); srz_draw_scene WITH stats (and srz_frameset_stats)
runs the counting pass k_vertex(nullptr) -> k_setup<true> first."""
import numpy as np
import pytest
import torch

from srz import abi
from srz import scenes as pscenes
from support import (big_tris, bits, col_major, ctx, place, render, same, scene_pair, sceneset_update, stream,  # noqa: F401  (ctx: the fixture)
                     unshared_mesh)

pytestmark = pytest.mark.gpu

F32 = np.float32
IDENT = np.eye(4, dtype=F32).reshape(16)
ZS, ZO = 49.95, 50.05  # (znear 0.1, zfar 100: the workloads' pair)


@pytest.mark.parametrize("make", [pscenes.spot_texture_1024, pscenes.spot_bunny_1080p])
def test_sceneset_equals_frameset_and_oracle(orc, make):
    import srz
    wl = make()
    ctx = srz.Context(0)
    idx = (0, 7, 19)
    frames = [wl.frame(i) for i in idx]
    wl.upload_textures(ctx)
    wl.upload_meshes(ctx)
    sframes = [wl.scene_frame(i) for i in idx]
    for slot, tex in enumerate(wl.texture_arrays):
        orc.texture_set(slot, tex)
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for fr in (frames, sframes):
        fs = ctx.frameset(fr)
        out = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
        fs.render(out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
        st = fs.stats()
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    for k, f in enumerate(frames):
        rc, ref, _ = orc.draw(f)
        assert np.array_equal(bits(outs[1][k]), bits(np.stack(ref)))
    # single-frame entry point with host planes
    planes, st1 = ctx.draw(sframes[1], want_stats=True)
    rc, ref, rst = orc.draw(frames[1])
    assert st1 == rst
    for a, b in zip(planes, ref):
        assert np.array_equal(bits(a), bits(b))
    ctx.close()


def test_mesh_upload_argument_checks():
    import srz
    ctx = srz.Context(0)
    v = np.zeros((3, 8), np.float32)
    with pytest.raises(srz.SrzError):
        ctx.mesh_upload(0, v, np.array([[0, 1, 3]], np.uint32))      # index out of range
    with pytest.raises(srz.SrzError):
        ctx.mesh_upload(999, v, np.array([[0, 1, 2]], np.uint32))    # slot out of range
    wl = pscenes.spot_texture_1024()
    with pytest.raises(srz.SrzError):
        ctx.frameset([wl.scene_frame(0)])                            # mesh slot 0 never uploaded
    ctx.close()


# ------------------------------------------------------------------------------------------------ shared steps
def oracle(orc, f):
    rc, ref, st = orc.draw(f)
    assert rc == 0
    return ref, st


def set_planes(c, frames, flags=abi.FUSED_CLEAR):
    """(the set, its colour render as [n, 4, rows, W] float32 on the host)"""
    fs, out = render(c, frames, flags)
    return fs, out.cpu().numpy()


def check_sets(c, orc, sframes, hframes, what, flags=abi.FUSED_CLEAR, refs=None, stats=False):
    """the sceneset against the frameset of the numpy triangles and against the oracle, every frame, bit for bit; stats: both sets'
    srz_frameset_stats equal the oracle's counters summed over the frames"""
    refs = refs or [oracle(orc, f) for f in hframes]
    fs_h, got_h = set_planes(c, hframes, flags)
    fs_s, got_s = set_planes(c, sframes, flags)
    for i, (ref, _) in enumerate(refs):
        same(got_s[i], got_h[i], f"{what}: frame {i}: the sceneset against the frameset of the numpy vertex stage")
        same(got_s[i], ref, f"{what}: frame {i}: the sceneset against the oracle")
    if stats:
        total = {k: sum(st[k] for _, st in refs) for k in refs[0][1]}
        assert fs_h.stats() == total, (what, "frameset", fs_h.stats(), total)
        assert fs_s.stats() == total, (what, "sceneset", fs_s.stats(), total)
    fs_h.close()
    return fs_s, got_s


def check_draw(c, orc, sframe, hframe, what, ref=None):
    """srz_draw_scene with stats (k_vertex without boxes, k_setup<true>, then the colour render's k_vertex + k_chunks) = the oracle"""
    ref, rst = ref or oracle(orc, hframe)
    gpu, gst = c.draw(sframe, want_stats=True)
    assert gst == rst, (what, gst, rst)
    same(gpu, ref, f"{what}: srz_draw_scene against the oracle")
    return rst


# ------------------------------------------------------------------------------------------------ a. projective positions
A_W, A_H, A_SEED = 96, 80, 0
A_LIGHTS = [((20.0, 10.0, 120.0), (900.0, 800.0, 700.0)), ((90.0, 70.0, 60.0), (300.0, 500.0, 400.0))]


def projective_mesh(seed, n_verts=300, n_faces=900):
    """shared vertices, random faces (some repeat a vertex); z in [-0.5, 2.5): w = a z + b with b = -a / 2 is negative for a third of
    them, and exactly zero for every eleventh (z = 0.5)"""
    rng = np.random.default_rng(seed)
    v = np.zeros((n_verts, 8), F32)
    v[:, 0:2], v[:, 2] = rng.uniform(-1, 1, (n_verts, 2)), rng.uniform(-0.5, 2.5, n_verts)
    v[::11, 2] = 0.5
    v[:, 3:6], v[:, 6:8] = rng.normal(size=(n_verts, 3)), rng.uniform(0, 1, (n_verts, 2))
    faces = rng.integers(0, n_verts, (n_faces, 3)).astype(np.uint32)
    faces[::60, 2] = faces[::60, 0]
    return v, faces


def projective(w, h, k, a, cx=0.0, cy=0.0):
    """viewport(k w / 2, k h / 2 about the centre + (cx, cy)) composed with a projection whose last row is (0, 0, a, -a / 2)"""
    P = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0.1], [0, 0, a, -a / 2]], np.float64)
    V = np.array([[k * w / 2, 0, 0, w / 2 + cx], [0, k * h / 2, 0, h / 2 + cy], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    return col_major(V @ P)


def projective_frames(flags=abi.FUSED_CLEAR, c=None):
    """two frames of one mesh drawn twice (NORMAL, then PHONG) under four different projective matrices and general normal matrices
    with a fourth row of their own -> [(SceneFrame, Frame)] and the mesh"""
    v, faces = projective_mesh(A_SEED)
    rng = np.random.default_rng(A_SEED + 1000)
    pairs = []
    for i, mats in enumerate((((0.45, 1.0, 0, 0), (0.3, 2.0, 7, -5)), ((0.6, 2.0, -9, 4), (0.4, 1.0, 3, 3)))):
        draws = []
        for (k, a, cx, cy), sh in zip(mats, (abi.SHADER_NORMAL, abi.SHADER_PHONG)):
            nm = rng.uniform(-1, 1, 16).astype(F32)
            nm[15] = 3.0
            draws.append((v, faces, sh, -1, projective(A_W, A_H, k, a, cx, cy), nm))
        pairs.append(scene_pair(draws, A_W, A_H, (30.0, 20.0, 150.0), A_LIGHTS, ZS, ZO, flags, ctx=c if i == 0 else None, slots=[0, 0],
                                p=(150.0, 7.5)[i]))
    return pairs, v


def test_projective_positions_and_shared_vertices(ctx, orc):
    """k_vertex under real projective matrices: w < 0 for a third of the vertices (mirrored, the reference does not clip), w == 0 for
    every eleventh (inf / NaN positions setup_triangle must drop), z * 49.95 + 50.05, shared vertices and faces that repeat one,
    normals through a general matrix.  Three ways: a two-frame sceneset without stats (k_vertex with boxes -> k_chunks, sorted groups);
    srz_draw_scene with stats (k_vertex without boxes -> k_setup<true>, then the render); both again with SRZ_ORDERED_RASTER."""
    pairs, v = projective_frames(c=ctx)
    w = v[:, 2] - F32(0.5)
    assert int((w == 0).sum()) == 28 and 80 <= int((w < 0).sum()) <= 120
    refs = [oracle(orc, f) for _, f in pairs]
    for i, (_, st) in enumerate(refs):  # the frames are not empty (checked on the oracle alone)
        assert st["n_tris"] == 1800 and st["n_tris"] - st["n_culled"] >= 450 and st["visible"] >= 1000, (i, st)
    check_sets(ctx, orc, [s for s, _ in pairs], [f for _, f in pairs], "projective", refs=refs, stats=True)[0].close()
    for i, (sf, f) in enumerate(pairs):
        check_draw(ctx, orc, sf, f, f"projective frame {i}", ref=refs[i])
    ordered, _ = projective_frames(abi.FUSED_CLEAR | abi.ORDERED_RASTER)
    orefs = [oracle(orc, f) for _, f in ordered]
    check_sets(ctx, orc, [s for s, _ in ordered], [f for _, f in ordered], "projective, ordered", flags=abi.FUSED_CLEAR | abi.ORDERED_RASTER,
               refs=orefs)[0].close()
    for i, (sf, f) in enumerate(ordered):
        assert check_draw(ctx, orc, sf, f, f"projective frame {i}, ordered", ref=orefs[i]) == refs[i][1]


# ------------------------------------------------------------------------------------------------ b. face counts and the draw mix
B_W, B_H = 160, 96
# (faces, x, y, pixels per quad) of each draw's region, in draw order (not sorted); faces = 0: the empty mesh, faces = 12: ONE slot
# drawn twice with different matrices.  ceil(sqrt(faces / 2)) quads a side: 1025 -> 23 x 2 px, 513 -> 17 x 2, 512 / 511 -> 16 x 2,
# 257 / 256 / 255 -> 12 x 2, 65 / 64 / 63 -> 6 x 4: no two regions share a pixel.  (Every region starts 0.3 / 0.4 pixels off the grid: a
# quad's edges pass no pixel centre)
B_DRAWS = ((257, 0, 48, 2), (1, 151, 2, 8), (1025, 0, 0, 2), (64, 104, 48, 4), (511, 118, 0, 2), (63, 130, 48, 4), (513, 48, 0, 2),
           (0, 0, 0, 1), (256, 26, 48, 2), (65, 78, 48, 4), (512, 84, 0, 2), (255, 52, 48, 2), (12, 50, 37, 3), (12, 100, 37, 3))


def quad_mesh(n_faces, seed):
    """n_faces triangles of a g x g grid of quads over the unit square (g = ceil(sqrt(n_faces / 2))), a normal of its own per face
    (three vertices per face, stored shuffled), depths of its own per face, wound to survive the cull for an eye at +z -> (verts8,
    faces, g)"""
    g = max(1, int(np.ceil(np.sqrt(n_faces / 2.0))))
    rng = np.random.default_rng(seed)
    t = np.zeros(n_faces, abi.TRI_DTYPE)
    k = np.arange(n_faces)
    qx, qy, half = (k // 2) % g, (k // 2) // g, k % 2
    x0, y0, x1, y1 = qx / g, qy / g, (qx + 1) / g, (qy + 1) / g
    a = np.where(half[:, None] == 0, np.stack([x0, y0], 1), np.stack([x1, y1], 1))
    b = np.where(half[:, None] == 0, np.stack([x0, y1], 1), np.stack([x1, y0], 1))
    c = np.where(half[:, None] == 0, np.stack([x1, y0], 1), np.stack([x0, y1], 1))
    t["pos"][:, 0, :2], t["pos"][:, 1, :2], t["pos"][:, 2, :2] = a, b, c
    t["pos"][:, :, 2] = rng.uniform(0.1, 0.9, (n_faces, 1))
    nn = rng.normal(size=(n_faces, 1, 3))
    t["nrm"] = nn / np.linalg.norm(nn, axis=2, keepdims=True)
    t["uv"] = rng.uniform(0, 1, (n_faces, 3, 2))
    v, faces = unshared_mesh(t, 1.0, 1.0, seed + 1)
    return v, faces, g


def draw_mix(c=None, with_empty=True):
    meshes, draws, slots = {}, [], []
    for i, (n, x, y, q) in enumerate(B_DRAWS):
        if n == 0 and not with_empty:
            continue
        if n not in meshes:
            meshes[n] = (len(meshes),) + quad_mesh(n, 40 + n) if n else (len(meshes), np.zeros((1, 8), F32), np.zeros((0, 3), np.uint32), 1)
        slot, v, faces, g = meshes[n]
        side = g * q + (0.25 if i % 2 else 0.0)  # (a quarter pixel on every other draw: edges off the pixel grid)
        nm = IDENT.copy()
        nm[15] = 2.0 + i
        draws.append((v, faces, abi.SHADER_NORMAL, -1, place(side, side * (2.5 if n == 1 else 1.0), x + 0.3, y + 0.4, sz=40.0, oz=5.0 + i), nm))
        slots.append(slot)
    return scene_pair(draws, B_W, B_H, (0.0, 0.0, 1.0), [], 1.0, 0.0, ctx=c, slots=slots)


def outcome(fn):
    import srz
    try:
        return "ok", fn()
    except srz.SrzError as e:
        return "SrzError", e


def test_face_count_edges_and_draw_mix(ctx, orc):
    """one frame of 14 draws, 1 .. 1025 faces each at the edges of k_vertex's 256-face blocks and the 64-triangle chunks, not sorted
    by size (grid.x follows the 1025: the other draws leave whole blocks idle), every draw over pixels of its own; one slot drawn twice
    with different matrices; a mesh of no faces between two others, which must do whatever a Frame with an empty batch there does.
    Without stats: k_vertex with boxes -> k_chunks (sorted groups); fs.stats() and srz_draw_scene: k_vertex without boxes ->
    k_setup<true>."""
    sf, f = draw_mix(ctx)
    how_h, fs_h = outcome(lambda: ctx.frameset([f]))
    how_s, fs_s = outcome(lambda: ctx.frameset([sf]))
    assert how_h == how_s, (how_h, fs_h, how_s, fs_s)
    if how_h == "ok":
        fs_h.close(), fs_s.close()
    else:  # (both refuse the empty draw: the rest of the mix without it)
        sf, f = draw_mix(ctx, with_empty=False)
    ref, rst = oracle(orc, f)
    n_faces = sum(n for n, _, _, _ in B_DRAWS)
    assert rst["n_tris"] == n_faces and rst["n_culled"] == 0 and rst["visible"] >= 6000, rst  # every face is kept
    check_sets(ctx, orc, [sf], [f], "draw mix", refs=[(ref, rst)], stats=True)[0].close()
    check_draw(ctx, orc, sf, f, "draw mix", ref=(ref, rst))


# ------------------------------------------------------------------------------------------------ c. the grid-stride loop
C_W, C_H, C_SMALL, C_LAST = 128, 96, 262144, 300


def sphere_points(n):
    """n well separated unit vectors (a Fibonacci lattice: neighbours are about 3.5 / sqrt(n) apart)"""
    k = np.arange(n) + 0.5
    z, phi = 1.0 - 2.0 * k / n, k * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def stride_mesh():
    """262 144 triangles of one to three pixels at depths 60 .. 90 all over the frame, then 300 triangles at depths 5 .. 6 tiling
    x 96 .. 126, y 3 .. 93 (10 x 15 quads of 3 x 6 pixels), each with a normal of its own -> (verts8, faces, the 300 normals)"""
    rng = np.random.default_rng(12)
    n = C_SMALL + C_LAST
    t = np.zeros(n, abi.TRI_DTYPE)
    c = rng.uniform([0, 0], [C_W, C_H], (C_SMALL, 2))
    r = rng.uniform(0.6, 1.6, (C_SMALL, 1))
    t["pos"][:C_SMALL, 0, :2] = c + r * [-1.0, -0.8]
    t["pos"][:C_SMALL, 1, :2] = c + r * [0.1, 1.0]
    t["pos"][:C_SMALL, 2, :2] = c + r * [1.0, -0.6]
    t["pos"][:C_SMALL, :, 2] = rng.uniform(60, 90, (C_SMALL, 1))
    nn = rng.normal(size=(C_SMALL, 1, 3))
    t["nrm"][:C_SMALL] = nn / np.linalg.norm(nn, axis=2, keepdims=True)
    k = np.arange(C_LAST)
    qx, qy, half = (k // 2) % 10, (k // 2) // 10, (k % 2)[:, None]
    x0, y0 = 96.4 + 3 * qx, 3.3 + 6 * qy
    x1, y1 = x0 + 3, y0 + 6
    t["pos"][C_SMALL:, 0, :2] = np.where(half == 0, np.stack([x0, y0], 1), np.stack([x1, y1], 1))
    t["pos"][C_SMALL:, 1, :2] = np.where(half == 0, np.stack([x0, y1], 1), np.stack([x1, y0], 1))
    t["pos"][C_SMALL:, 2, :2] = np.where(half == 0, np.stack([x1, y0], 1), np.stack([x0, y1], 1))
    t["pos"][C_SMALL:, :, 2] = rng.uniform(5, 6, (C_LAST, 1))
    normals = sphere_points(C_LAST)
    t["nrm"][C_SMALL:] = normals[:, None, :]
    v, faces = unshared_mesh(t, C_W, C_H, 13)
    return v, faces, normals


def test_grid_stride_loop(ctx, orc):
    """one draw of 262 144 + 300 faces: launch_vertex caps grid.x at 1024 blocks of 256, so the last 300 faces are the second trip of
    k_vertex's grid-stride loop — and the nearest surface over pixels of their own.  The frameset render (k_vertex with boxes ->
    k_chunks, a band far above k_bin's LDS stage) and srz_draw_scene (k_vertex without boxes -> k_setup<true>, then the render)
    against the oracle.  The condition: at least 200 of the last 300 faces own a pixel of the oracle's frame (where it differs from
    the oracle's frame without them, the colour is the face's own normal)."""
    v, faces, normals = stride_mesh()
    mvp = place(C_W, C_H, 0.0, 0.0)
    sf, f = scene_pair([(v, faces, abi.SHADER_NORMAL, -1, mvp, IDENT)], C_W, C_H, (0.0, 0.0, 1.0), [], 1.0, 0.0, ctx=ctx, slots=[7])
    _, f_without = scene_pair([(v, faces[:C_SMALL], abi.SHADER_NORMAL, -1, mvp, IDENT)], C_W, C_H, (0.0, 0.0, 1.0), [], 1.0, 0.0)
    ref, rst = oracle(orc, f)
    ref0, _ = oracle(orc, f_without)
    theirs = np.logical_or.reduce([bits(a) != bits(b) for a, b in zip(ref, ref0)])
    colour = np.stack([p[theirs] for p in ref[1:]], 1).astype(np.float64) / 255.0 * 2.0 - 1.0  # (NORMAL: (n + 1) / 2 * 255)
    dots = colour @ normals.T
    assert (dots.max(axis=1) > 0.985).all()  # (every such pixel shows one of the 300 normals, 0.2 rad apart, to a colour level or two)
    owners = np.unique(dots.argmax(axis=1))
    assert len(owners) >= 200, len(owners)
    assert rst["n_tris"] == C_SMALL + C_LAST and rst["n_culled"] == 0, rst
    check_sets(ctx, orc, [sf], [f], "grid stride", refs=[(ref, rst)])[0].close()
    check_draw(ctx, orc, sf, f, "grid stride", ref=(ref, rst))


# ------------------------------------------------------------------------------------------------ d. k_chunks' binning
def band_soup():
    """6000 small triangles in ONE 32-row band of a 2048 x 64 frame (tests/test_gpu_raster_paths.py's stage overflow)"""
    w = 2048
    rng = np.random.default_rng(3)
    n = 6000
    t = np.zeros(n, abi.TRI_DTYPE)
    cx, cy = rng.uniform(4, w - 4, n), rng.uniform(3, 28, n)
    t["pos"][:, 0, :2] = np.stack([cx - 3, cy - 2], 1)
    t["pos"][:, 2, :2] = np.stack([cx + 4, cy - 1], 1)
    t["pos"][:, 1, :2] = np.stack([cx, cy + 3], 1)
    t["pos"][:, :, 2] = rng.uniform(5, 50, (n, 1))
    t["nrm"][:] = [0, 0, -1]
    return t


def chunk_case(name):
    if name == "raw-entries":
        return big_tris(700, 160, 2400, 11, 150), 160, 2400
    if name == "raw-tall":
        return big_tris(40, 160, 2400, 11, 2300), 160, 2400
    return band_soup(), 2048, 64


def chunk_pair(name, c, flags=abi.FUSED_CLEAR):
    t, w, h = chunk_case(name)
    v, faces = unshared_mesh(t, w, h, 21)
    return scene_pair([(v, faces, abi.SHADER_NORMAL, -1, place(w, h, 0.0, 0.0), IDENT)], w, h, (0.0, 0.0, 1.0), [], 1.0, 0.0, flags, ctx=c,
                      slots=[3]), h


@pytest.mark.parametrize("name", ["raw-entries", "raw-tall", "lds-stage"])
def test_k_chunks_binning(ctx, orc, name):
    """the geometries of test_groups_with_huge_triangles_take_the_raw_walk and test_band_with_more_pairs_than_the_lds_stage delivered
    as meshes in unit coordinates: k_vertex with boxes -> k_chunks.  raw-entries: 700 triangles x 5-6 bands, a 512-triangle group
    above ENT_PER_GROUP entries (k_chunks raw); raw-tall: triangles more than 64 bands tall (k_chunks raw); lds-stage: 6000 triangles
    in one band, k_chunks' sorted entries above k_bin's 4096-entry LDS stage.  Both rasterisers."""
    for extra in (0, abi.ORDERED_RASTER):
        (sf, f), _ = chunk_pair(name, ctx, abi.FUSED_CLEAR | extra)
        ref, rst = oracle(orc, f)
        assert rst["n_culled"] < rst["n_tris"] // 10 and rst["visible"] > 10000, rst
        check_sets(ctx, orc, [sf], [f], f"k_chunks {name} flags+={extra}", flags=abi.FUSED_CLEAR | extra, refs=[(ref, rst)])[0].close()


def test_k_chunks_binning_under_a_shard(orc):
    """raw-entries as rank 1 of a world of 3: k_vertex with boxes -> k_chunks raw under shard_world > 1 (a box's local bands are every
    third band); the rank's rows against the oracle's"""
    import srz
    from srz import parallel
    c = srz.Context(0, 1, 3)
    try:
        (sf, f), h = chunk_pair("raw-entries", c)
        ref, _ = oracle(orc, f)
        for fr, what in ((f, "frameset"), (sf, "sceneset")):
            fs, got = set_planes(c, [fr])
            rows = parallel.band_rows(h, 1, 3)
            assert len(rows) >= 20
            for (lb, b, r0, r1) in rows:
                assert np.array_equal(bits(got[0][:, lb * 32: lb * 32 + (r1 - r0)]), bits(np.stack(ref)[:, r0:r1])), (what, b)
            fs.close()
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ e. pool overflow and growth
E_SIZE, E_TRIS = 1024, 24


def filling_mesh():
    """the screen-filling triangles of test_pool_overflow_then_growth (eye behind their winding: none is culled)"""
    n, w, h = E_TRIS, E_SIZE, E_SIZE
    t = np.zeros(n, abi.TRI_DTYPE)
    for i in range(n):
        t["pos"][i] = [[-40 + 3 * i, -30, 10 + i % 5], [w + 50 - i, 10 + 2 * i, 12 + (i * 7) % 5], [200 + 5 * i, h + 60, 11 + (i * 3) % 7]]
    nn = np.random.default_rng(5).normal(size=(n, 3, 3))
    t["nrm"] = nn / np.linalg.norm(nn, axis=2, keepdims=True)
    return unshared_mesh(t, w, h, 31)


def filling_pair(c, mvp):
    v, faces = filling_mesh()
    return scene_pair([(v, faces, abi.SHADER_NORMAL, -1, mvp, IDENT)], E_SIZE, E_SIZE, (0.0, 0.0, -1.0), [], 1.0, 0.0, ctx=c, slots=[5])


def renders(fs, n, refs, what):
    """n renders of a one-frame set into a buffer that starts as -1, each equal to the oracle's planes -> the debug counters after each"""
    out = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    counters = []
    for it in range(n):
        out.fill_(-1.0)
        fs.render(out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
        torch.cuda.synchronize()
        same(out[0].cpu().numpy(), refs, f"{what}, render {it}")
        counters.append(fs.debug_counters())
    return counters


def test_pool_overflow_then_growth_on_a_sceneset(ctx, orc):
    """SRZ_OPT_POOL_LAZY: a sceneset of 24 screen-filling triangles is created with the first guess of the list pool; k_chunks' entries
    (k_vertex with boxes -> k_chunks, sorted) overflow it, the first render serves those bands through the ordered rasteriser, the pool
    grows, and the last render has none left"""
    ctx.set_option(abi.OPT_POOL_LAZY, 1)
    try:
        sf, f = filling_pair(ctx, place(E_SIZE, E_SIZE, 0.0, 0.0))
        ref, rst = oracle(orc, f)
        assert rst["n_culled"] == 0 and rst["visible"] > 500000, rst
        fs = ctx.frameset([sf])
        dc = renders(fs, 3, ref, "lazy pool")
        assert dc[0]["slow_tiles"] > 0 and dc[-1]["slow_tiles"] == 0, dc
        fs.close()
    finally:
        ctx.set_option(abi.OPT_POOL_LAZY, 0)


def test_sceneset_update_outgrows_the_pool(ctx, orc):
    """srz_sceneset_update moving the geometry: the set is created (and its pool sized) with matrices that shrink the 24 triangles
    into one tile; the update makes them fill the 1024 x 1024 frame, so the next render's demand (k_vertex with boxes -> k_chunks,
    sorted) exceeds the capacity creation gave — asserted — and the pool follows: growth.  Every render equals the oracle of its own
    matrices.  The count stays at 24: a set of 24 triangles starts with (4 * 24 + 4096) + 64 = 4256 entries, one tile asks for 24,
    and 24 triangles over 32 x 32 tiles ask for well over 10 000 (the same triangles overflow the same first guess in
    test_pool_overflow_then_growth); the assertion below holds the test to it."""
    small, filling = place(24.0, 24.0, 2.0, 3.0), place(E_SIZE, E_SIZE, 0.0, 0.0)
    sf0, f0 = filling_pair(ctx, small)
    sf1, f1 = filling_pair(None, filling)
    ref0, st0 = oracle(orc, f0)
    ref1, st1 = oracle(orc, f1)
    assert st0["n_culled"] == 0 and st0["visible"] > 100 and st1["n_culled"] == 0 and st1["visible"] > 500000, (st0, st1)
    fs = ctx.frameset([sf0])
    before = renders(fs, 1, ref0, "one tile")[0]
    assert before["slow_tiles"] == 0 and before["pool_sub_cap"] >= before["pool_demand"] > 0, before
    sceneset_update(ctx, fs, [sf1])
    after = renders(fs, 3, ref1, "after the update")
    print(f"[sceneset update] before {before} after {after}")
    assert after[0]["pool_demand"] > before["pool_sub_cap"], (before, after[0])  # the overflow this test is about did happen
    assert after[-1]["slow_tiles"] == 0 and after[-1]["pool_sub_cap"] >= after[-1]["pool_demand"], after
    fs.close()


# ------------------------------------------------------------------------------------------------ f. srz_draw_scene and re-uploads
def test_draw_scene_across_a_mesh_re_upload(ctx, orc):
    """srz_draw_scene keeps its one-frame set by a signature of size, light count and draw count.  A slot uploaded anew with another
    face count makes srz_sceneset_update refuse and the set is rebuilt; with the same face count and other contents the buffers are
    new ones all the same; uploaded twice between two draws, the second upload's buffers may get the addresses the set remembers,
    and it is the upload's ordinal, not the address, that the update compares.  Each draw (k_vertex without boxes -> k_setup<true>, then k_vertex with boxes -> k_chunks) must show the
    mesh then resident."""
    for step, (n, seed) in enumerate(((130, 1), (77, 2), (77, 3), (77, 5))):
        if step == 3:  # two uploads since the last draw: the second one's buffers may sit where the set's freed ones were
            ctx.mesh_upload(9, *quad_mesh(n, 4)[:2])
        v, faces, _ = quad_mesh(n, seed)
        sf, f = scene_pair([(v, faces, abi.SHADER_NORMAL, -1, place(70.0, 50.0, 9.0 + step, 6.0, sz=30.0, oz=4.0), IDENT)], 96, 64,
                           (0.0, 0.0, 1.0), [], 1.0, 0.0, ctx=ctx, slots=[9])
        rst = check_draw(ctx, orc, sf, f, f"re-upload step {step}")
        assert rst["n_tris"] == n and rst["n_culled"] == 0 and rst["visible"] > 2000, rst


# ------------------------------------------------------------------------------------------------ g. refusals
def refused(call, fn):
    import srz
    with pytest.raises(srz.SrzError) as e:
        fn()
    assert call in str(e.value), (call, str(e.value))


def test_refusals(ctx):
    """host-side checks, nothing is launched: srz_sceneset_update on a set that is no sceneset, with another frame count, size, light
    count, draw count or slot, and after the slot was uploaded anew with another face count (that set is then destroyed, never
    rendered: its draws point at freed buffers); srz_frameset_update_shading on a sceneset; srz_sceneset_create with a negative slot
    and with n_draws > 0 but no draws"""
    va, fa, _ = quad_mesh(10, 5)
    vb, fb, _ = quad_mesh(10, 6)
    light = [((1.0, 2.0, 3.0), (4.0, 5.0, 6.0))]
    mvp = place(40.0, 40.0, 4.0, 4.0)

    def pair(w=64, h=48, lights=light, slots=(20, 21), n=2, c=None):
        draws = [(va, fa, abi.SHADER_NORMAL, -1, mvp, IDENT), (vb, fb, abi.SHADER_PHONG, -1, mvp, IDENT)][:n]
        return scene_pair(draws, w, h, (0.0, 0.0, 1.0), lights, 1.0, 0.0, ctx=c, slots=list(slots)[:n])

    sf, f = pair(c=ctx)
    ctx.mesh_upload(22, vb, fb)
    fs, plain = ctx.frameset([sf, sf]), ctx.frameset([f, f])
    refused("srz_sceneset_update", lambda: sceneset_update(ctx, plain, [sf, sf]))               # not a sceneset
    refused("srz_sceneset_update", lambda: sceneset_update(ctx, fs, [sf]))                      # another frame count
    refused("srz_sceneset_update", lambda: sceneset_update(ctx, fs, [sf, pair(w=32)[0]]))       # another size
    refused("srz_sceneset_update", lambda: sceneset_update(ctx, fs, [pair(lights=[])[0], sf]))  # another light count
    refused("srz_sceneset_update", lambda: sceneset_update(ctx, fs, [sf, pair(n=1)[0]]))        # another draw count
    refused("srz_sceneset_update", lambda: sceneset_update(ctx, fs, [sf, pair(slots=(20, 22))[0]]))  # a draw names another slot
    refused("srz_frameset_update_shading", lambda: fs.update_shading([f, f]))
    sceneset_update(ctx, fs, [sf, sf])  # (the set itself is fine: the same structure is accepted)
    vc, fc, _ = quad_mesh(11, 7)
    ctx.mesh_upload(21, vc, fc)
    refused("srz_sceneset_update", lambda: sceneset_update(ctx, fs, [sf, sf]))                  # the slot has another face count now
    fs.close(), plain.close()
    refused("srz_sceneset_create", lambda: ctx.frameset([pair(slots=(20, -1))[0]]))
    broken = pair()[0]
    broken.c.draws = None
    refused("srz_sceneset_create", lambda: ctx.frameset([broken]))
    ctx.sync()
