"""What the tests share, each thing once: the frame builders (inputs, numpy only), the comparisons with their stated bounds, the
oracle-vs-GPU steps, the kit of the passes over a visibility buffer (and of their references) and the context fixtures.  A plain module like tests/scenes.py: importable without a GPU and without pytest
running (tools/fuzz_probe.py imports it as a script); torch and srz are imported by the functions that need them.  Test modules
import from here and from scenes, never from one another."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import scenes
from srz import abi

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------ inputs
def tri(a, b, c, z=50.0, nrm=(0, 0, -1), uv=((0, 0), (0, 0), (0, 0))):
    t = np.zeros(1, abi.TRI_DTYPE)
    za, zb, zc = (z, z, z) if np.isscalar(z) else z
    t["pos"][0] = [[a[0], a[1], za], [b[0], b[1], zb], [c[0], c[1], zc]]
    t["nrm"][0] = [nrm] * 3 if np.ndim(nrm) == 1 else nrm
    t["uv"][0] = uv
    return t


def ccw(a, b, c, **kw):  # a winding that survives the cull for eye=(0,0,1)
    return tri(a, c, b, **kw)


def frame(tris, w=64, h=64, shader=abi.SHADER_NORMAL, eye=(0, 0, 1), lights=(), flags=abi.FUSED_CLEAR, tex=-1, **kw):
    batches = tris if isinstance(tris, list) else [(shader, tex, tris)]
    return abi.Frame(w, h, eye, np.asarray(lights, np.float32).reshape(-1, 2, 3), batches, flags, **kw)


def lit(f, lights=None, **kw):
    """a copy of abi.Frame f with other lights / shading constants (same triangles)"""
    c = f.c
    args = dict(ka=tuple(c.ka), ks=tuple(c.ks), p=c.p, kh=c.kh, kn=c.kn)
    args.update(kw)
    batches = kw.pop("batches", None) or [(f._batches[i].shader, f._batches[i].tex_id, t) for i, t in enumerate(f.tris)]
    args.pop("batches", None)
    return abi.Frame(c.width, c.height, tuple(c.eye), f.lights if lights is None else np.asarray(lights, np.float32).reshape(-1, 2, 3),
                     batches, c.flags, **args)


def soup(seed, n, w, h, zs, big=False):
    rng = np.random.default_rng(seed)
    t = np.zeros(n, abi.TRI_DTYPE)
    c = rng.uniform(-8, [w + 8, h + 8], (n, 1, 2))
    r = rng.uniform(1, 70 if big else 24, (n, 1, 1))
    xy = c + rng.uniform(-1, 1, (n, 3, 2)) * r
    xy = np.round(xy * 4) / 4 if seed % 2 else xy  # half the seeds: quarter-pixel vertices → exact edge hits and ties
    t["pos"][:, :, :2] = xy
    t["pos"][:, :, 2] = rng.choice(zs, (n, 1)) if seed % 3 == 0 else rng.choice(zs, (n, 3))
    nn = rng.normal(size=(n, 3, 3))
    t["nrm"] = nn / np.linalg.norm(nn, axis=2, keepdims=True)
    t["uv"] = rng.uniform(0, 1, (n, 3, 2))
    return t


def stack(n, w=64, h=64, jitter=0):
    """n triangles stacked over one 32x32 tile (the list of tile (0,0) has n entries), depths shuffled, some ties"""
    rng = np.random.default_rng(n + jitter)
    t = np.zeros(n, abi.TRI_DTYPE)
    c = rng.uniform(4, 28, (n, 1, 2))
    t["pos"][:, :, :2] = np.round((c + rng.uniform(-1, 1, (n, 3, 2)) * rng.uniform(6, 30, (n, 1, 1))) * 4) / 4
    t["pos"][:, :, 2] = rng.choice(np.float32([1, 2, 3, 4, 5, 6, 7, 8]), (n, 3))
    t["nrm"] = [0, 0, -1]
    return frame(t, w, h)


def big_tris(n, w, h, seed, tall):
    """n triangles about `tall` pixels high at random places (depths distinct per triangle)"""
    rng = np.random.default_rng(seed)
    t = np.zeros(n, abi.TRI_DTYPE)
    cx, cy = rng.uniform(0, w, n), rng.uniform(0, h, n)
    t["pos"][:, 0, :2] = np.stack([cx - 9, cy - tall / 2], 1)
    t["pos"][:, 2, :2] = np.stack([cx + 11, cy - tall / 2 + 3], 1)  # (this winding faces the eye at (0, 0, 1))
    t["pos"][:, 1, :2] = np.stack([cx + 2, cy + tall / 2], 1)
    t["pos"][:, :, 2] = rng.uniform(5, 50, (n, 1))
    nn = rng.normal(size=(n, 3, 3))
    t["nrm"] = nn / np.linalg.norm(nn, axis=2, keepdims=True)
    return t


def adversarial_tris(seed, n, w, h):
    """the shapes the tightened rectangles (k_raster's slab clips, bucket_group's band clips) must stay conservative for:
    needles, slivers, huge and far-off-screen vertices (past the 2^20 guard too), sub-pixel triangles around pixel centres,
    edges exactly through pixel centres and along tile borders, ordinary large triangles — in both windings"""
    rng = np.random.default_rng(seed)
    t = np.zeros(n, abi.TRI_DTYPE)
    kind = rng.integers(0, 9, n)
    c = rng.uniform([0, 0], [w, h], (n, 2))
    ang = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(ang), np.sin(ang)], 1)
    nrm = np.stack([-d[:, 1], d[:, 0]], 1)
    xy = np.zeros((n, 3, 2))
    L = rng.uniform(100, 600, n)[:, None]
    # 0 needles: a very short base, the apex far away
    k = kind == 0
    base = (10.0 ** rng.uniform(-3, 0, n))[:, None]
    xy[k] = np.stack([c, c + nrm * base, c + d * L], 1)[k]
    # 1 slivers: a long edge, a height of 1e-4 .. 0.5 pixels
    k = kind == 1
    hgt = (10.0 ** rng.uniform(-4, -0.3, n))[:, None]
    xy[k] = np.stack([c, c + d * L, c + d * L * rng.uniform(0, 1, (n, 1)) + nrm * hgt], 1)[k]
    # 2 huge: vertices 1e3 .. 1e6 pixels out;  3 past the guard: one vertex 2e6 .. 1e8 out
    k = kind == 2
    xy[k] = (c[:, None, :] + rng.normal(size=(n, 3, 2)) * (10.0 ** rng.uniform(3, 6, (n, 1, 1))))[k]
    k = kind == 3
    far = c[:, None, :] + rng.normal(size=(n, 3, 2)) * 300.0
    far[:, 0] += d * (10.0 ** rng.uniform(6.3, 8, n))[:, None]
    xy[k] = far[k]
    # 4 sub-pixel triangles around pixel centres
    k = kind == 4
    xy[k] = (np.round(c)[:, None, :] + rng.uniform(-1, 1, (n, 3, 2)) * (10.0 ** rng.uniform(-3, 0, (n, 1, 1))))[k]
    # 5 integer / half-integer / tile-border vertices: edges through pixel centres, exact zeros of the edge functions
    k = kind == 5
    grid = rng.choice([1.0, 0.5, 32.0], (n, 1, 1))
    xy[k] = (np.round((c[:, None, :] + rng.uniform(-1, 1, (n, 3, 2)) * rng.uniform(2, 200, (n, 1, 1))) / grid) * grid)[k]
    # 6 ordinary large triangles
    k = kind == 6
    xy[k] = (c[:, None, :] + rng.uniform(-1, 1, (n, 3, 2)) * rng.uniform(30, 400, (n, 1, 1)))[k]
    # 7 tiny triangles (extent 2^-12 .. 2^-4 pixels) at coordinates < 64 around pixel centres, near the sliver limit of the guard:
    #   below 2^-5 the tightened rectangles must fall back to the plain box (tight_margin), above it the margin must hold
    k = kind == 7
    Dt = (2.0 ** rng.uniform(-12, -4, n))[:, None]
    c7 = np.round(rng.uniform([0, 0], [64, 64], (n, 2))) + rng.uniform(-1, 1, (n, 2)) * Dt
    xy[k] = np.stack([c7, c7 + d * Dt, c7 + d * Dt * rng.uniform(0, 1, (n, 1)) + nrm * Dt * (2.0 ** rng.uniform(-7.5, 0, n))[:, None]], 1)[k]
    # 8 small or ulp-sized triangles 1e4 .. 1e7 pixels off screen on ONE axis: the clamped box is an edge column / row at a
    #   distance from the triangle that has nothing to do with its extent (plain box there)
    k = kind == 8
    off = np.zeros((n, 2))
    off[np.arange(n), rng.integers(0, 2, n)] = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(4, 7, n)
    D8 = (10.0 ** rng.uniform(-3, 2.5, n))[:, None, None]
    xy[k] = ((c + off)[:, None, :] + rng.uniform(-1, 1, (n, 3, 2)) * D8)[k]
    flip = rng.random(n) < 0.5
    xy[flip] = xy[flip][:, ::-1]
    t["pos"][:, :, :2] = xy
    # (the screen-filling kinds lie behind the others, so that every small shape decides pixels of the final image)
    t["pos"][:, :, 2] = np.where((kind == 2) | (kind == 3), rng.uniform(60, 80, n), rng.uniform(2, 60, n))[:, None] + rng.uniform(-1, 1, (n, 3))
    nn = rng.normal(size=(n, 3, 3))
    t["nrm"] = nn / np.linalg.norm(nn, axis=2, keepdims=True)
    t["uv"] = rng.uniform(0, 1, (n, 3, 2))
    return t


def random_frame(rng, w, h, n_tris, flags):
    """Random soup: mostly small triangles, some large / off-screen / sliver ones, random normals, uvs beyond [0,1],
    every shader, 0-3 lights — the shapes the tile masks, the per-frame work lists and the FastMath paths must survive."""
    def tris(n):
        t = np.zeros(n, abi.TRI_DTYPE)
        c = rng.uniform([-0.1 * w, -0.1 * h], [1.1 * w, 1.1 * h], (n, 1, 2))
        size = np.where(rng.random((n, 1, 1)) < 0.85, rng.uniform(1, 24, (n, 1, 1)), rng.uniform(24, 1.5 * max(w, h), (n, 1, 1)))
        xy = c + rng.uniform(-1, 1, (n, 3, 2)) * size
        snap = rng.random((n, 1, 1)) < 0.3          # vertices exactly on pixel corners: on-edge samples, exact zeros
        xy = np.where(snap, np.round(xy), xy)
        t["pos"][:, :, :2] = xy
        t["pos"][:, :, 2] = rng.uniform(1, 90, (n, 1)) + rng.uniform(-0.5, 0.5, (n, 3))
        t["nrm"] = rng.normal(0, 1, (n, 3, 3)) * rng.choice([1.0, 1e-3, 50.0], (n, 1, 1))
        t["uv"] = rng.uniform(-0.2, 1.2, (n, 3, 2))
        return t
    shaders = [abi.SHADER_NORMAL, abi.SHADER_TEXTURE, abi.SHADER_PHONG, abi.SHADER_BUMP, abi.SHADER_DISPLACEMENT]
    nb = int(rng.integers(1, 4))
    batches = []
    for b in range(nb):
        sh = shaders[int(rng.integers(0, len(shaders)))]
        batches.append((sh, 0 if sh in (abi.SHADER_TEXTURE, abi.SHADER_BUMP, abi.SHADER_DISPLACEMENT) else -1, tris(max(1, n_tris // nb))))
    nl = int(rng.integers(0, 4))
    lights = np.concatenate([rng.uniform([0, 0, -50], [w, h, 120], (nl, 1, 3)), rng.uniform(0, 400, (nl, 1, 3))], 1).astype(np.float32)
    return abi.Frame(w, h, (0.0, 0.0, float(rng.uniform(0.5, 2.0))), lights, batches, flags, p=float(rng.choice([150.0, 8.0, 2.5])))


# ------------------------------------------------------------------------------------------------ the vertex stage
def xform_div_w(m, v):
    """the tests' OWN restatement in numpy binary32 of the vertex stage's transform (Tools::to_vec3 of mat4 * vec4 in glm's order, as
    csrc/srz_kernels.hip xform_div_w and the oracle's orc_vertex_stage have it): (m0 x + m1 y) + (m2 z + m3), divided by the fourth
    row's.  m: 16 floats, column-major; v: [n, 3].  (The product's host vertex stage is C++, libsrz_host: it takes model / view /
    projection, not a free normal_m.)"""
    m, v = np.asarray(m, np.float32).reshape(16), np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        r = [(m[0 * 4 + i] * v[:, 0] + m[1 * 4 + i] * v[:, 1]) + (m[2 * 4 + i] * v[:, 2] + m[3 * 4 + i]) for i in range(4)]
        return np.stack([r[0] / r[3], r[1] / r[3], r[2] / r[3]], 1)


def vertex_stage(verts8, faces, ndc_mvp, normal_m, zscale, zoffset):
    """Scene::loadTriangleStream restated in numpy binary32 (k_vertex, the oracle's orc_vertex_stage): positions through ndc_mvp with
    z * zscale + zoffset, normals through normal_m, uv copied, the three vertices of every face gathered -> TRI_DTYPE[n_faces]"""
    v = np.ascontiguousarray(verts8, np.float32).reshape(-1, 8)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    pos = xform_div_w(ndc_mvp, v[:, 0:3])
    with np.errstate(all="ignore"):
        pos[:, 2] = pos[:, 2] * np.float32(zscale) + np.float32(zoffset)
    nrm = xform_div_w(normal_m, v[:, 3:6])
    assert pos.dtype == np.float32 and nrm.dtype == np.float32
    t = np.zeros(len(f), abi.TRI_DTYPE)
    t["pos"], t["nrm"], t["uv"] = pos[f], nrm[f], v[:, 6:8][f]
    return t


def col_major(rows):
    """a 4 x 4 matrix written row by row -> the 16 floats of glm's layout m[col * 4 + row]"""
    return np.asarray(rows, np.float64).T.astype(np.float32).reshape(16)


def place(sx, sy, ox, oy, w=2.0, sz=1.0, oz=0.0):
    """unit coordinates -> pixels: x' = sx x + ox, y' = sy y + oy, z' = sz z + oz, every row scaled by w and divided by it again
    (w a power of two: the division is exact, but it is a division by something other than 1)"""
    return col_major([[sx * w, 0, 0, ox * w], [0, sy * w, 0, oy * w], [0, 0, sz * w, oz * w], [0, 0, 0, w]])


def unshared_mesh(t, w, h, seed):
    """TRI_DTYPE triangles in pixels -> (verts8 in unit coordinates, faces): three vertices of its own per triangle, stored in a
    shuffled order, so that `faces` is no arange"""
    n = len(t)
    v = np.zeros((3 * n, 8), np.float32)
    v[:, 0:3] = t["pos"].reshape(-1, 3) / np.array([w, h, 1.0])
    v[:, 3:6], v[:, 6:8] = t["nrm"].reshape(-1, 3), t["uv"].reshape(-1, 2)
    perm = np.random.default_rng(seed).permutation(3 * n)
    where = np.empty(3 * n, np.int64)
    where[perm] = np.arange(3 * n)
    return v[perm], where.reshape(n, 3).astype(np.uint32)


def scene_pair(draws, w, h, eye, lights, zscale, zoffset, flags=abi.FUSED_CLEAR, ctx=None, slots=None, **shading):
    """One frame both ways.  draws: [(verts8, faces, shader, tex, ndc_mvp, normal_m)]; slots: the mesh slot of each draw (default 0, 1,
    ...; a slot named twice must be given the same mesh object both times and is uploaded once).  ctx given: the meshes are uploaded
    to their slots.  -> (abi.SceneFrame of the slots and matrices, abi.Frame whose batches hold vertex_stage()'s triangles)"""
    slots = list(range(len(draws))) if slots is None else list(slots)
    assert len(slots) == len(draws)
    sdraws, batches, seen = [], [], {}
    for slot, (v, f, shader, tex, mvp, nm) in zip(slots, draws):
        if slot in seen:
            assert seen[slot] is v, "one slot, two meshes"
        elif ctx is not None:
            ctx.mesh_upload(slot, v, np.asarray(f, np.uint32).reshape(-1, 3))
        seen[slot] = v
        sdraws.append((slot, shader, tex, mvp, nm))
        batches.append((shader, tex, vertex_stage(v, f, mvp, nm, zscale, zoffset)))
    L = np.asarray(lights, np.float32).reshape(-1, 2, 3)
    return (abi.SceneFrame(w, h, eye, L, sdraws, zscale, zoffset, flags, **shading), abi.Frame(w, h, eye, L, batches, flags, **shading))


# ------------------------------------------------------------------------------------------------ hostile shading inputs
# Tame geometry, hostile values in everything the SHADERS read (uv, normals, lights, eye, ka / ks / kh / kn, the exponent, the
# textures' shapes).  A fragment's position is (column, row, depth); the tame defaults put the eye and the lights far above the image
# (depth 200..400, the triangles lie at 5..90 with normals near (0, 0, 1)), so that the diffuse and the specular term are alive.
HOSTILE_FAMILIES = ("uv-edge", "uv-overflow", "uv-nonfinite", "normal-nonfinite", "light-edge", "eye-edge", "constants", "exponent",
                    "texture-shape")
HOSTILE_EXPONENTS = (0.0, 1.0, 2.0, 255.0, 256.0, 257.0, 0.5, 7.5, 4095.5, 4096.0, 4097.0, -1.0, 1e30, float("inf"), float("nan"))
TEXTURED = (abi.SHADER_TEXTURE, abi.SHADER_BUMP, abi.SHADER_DISPLACEMENT)
# slot -> (width, height, row_stride): slots away from the ones other modules register in the session's oracle (0, 1, 5..11); the
# default texture of the hostile frames is the 5 x 7 one
HOSTILE_TEX = 40
HOSTILE_TEX_SHAPES = {12: (1, 1, 3), 23: (1, 7, 3), 31: (7, 1, 21), HOSTILE_TEX: (5, 7, 15), 47: (2, 2, 6), 62: (64, 64, 3 * 64 + 13),
                      63: (5, 7, 15 + 2)}
_F32 = np.float32
_NAN, _INF = _F32(np.nan), _F32(np.inf)


def hostile_textures():
    """slot -> ((h, w, 3) uint8 texels, row_stride): no byte is zero (a black pixel can only come from the fetch's out-of-range
    case), texel (0, 0) is bright; deterministic"""
    out = {}
    for slot, (w, h, stride) in sorted(HOSTILE_TEX_SHAPES.items()):
        t = np.random.default_rng(1000 + slot).integers(24, 256, (h, w, 3)).astype(np.uint8)
        t[0, 0] = (250, 200, 150)
        out[slot] = (t, stride)
    return out


def padded_rows(texels, row_stride):
    """the (h, w, 3) texels as h rows of row_stride bytes, the padding 0xFF (a fetch that ignores the stride reads it)"""
    h, w, _ = texels.shape
    buf = np.full((h, row_stride), 0xFF, np.uint8)
    buf[:, :3 * w] = texels.reshape(h, 3 * w)
    return buf


def register_hostile_textures(orc, ctx=None):
    """hostile_textures() into the oracle's table and (ctx given) into the context's, each from its padded rows with its row_stride"""
    for slot, (t, stride) in hostile_textures().items():
        h, w, _ = t.shape
        buf = padded_rows(t, stride)
        assert orc.lib().orc_texture_set(slot, buf.ctypes.data, w, h, stride) == 0
        if ctx is not None:
            import srz
            ctx._check(srz.lib().srz_texture_upload(ctx.h, slot, buf.ctypes.data, w, h, stride))


def _hostile_geometry(rng, w, h):
    """(positions [n, 3, 3], thin [n]): triangle 0 fills the screen at depth 90; then triangles 10..40 pixels wide (8-wide "V" columns
    and a scalar tail) and triangles narrower than 8 pixels (scalar-tail "S" columns only), all finite, on screen, flat in depth, with
    the winding that survives the cull for an eye above the image; the last four wound the other way (culled unless the eye is NaN)"""
    scale = (w * h) / (64.0 * 64.0)
    n_med, n_thin = int(14 * scale ** 0.5) + 10, int(20 * scale ** 0.5) + 12
    pos = [np.array([[-8.0, -8.0, 90.0], [-8.0, 2.0 * h + 8.0, 90.0], [2.0 * w + 8.0, -8.0, 90.0]])]
    for i in range(n_med + 4):
        c = rng.uniform([10, 10], [w - 10, h - 10])
        ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.4, 0.4, 3)
        r = rng.uniform(6, 20, 3)
        xy = c + np.stack([np.cos(ang), np.sin(ang)], 1) * r[:, None]
        pos.append(np.concatenate([np.clip(xy, 0.25, [w - 1.25, h - 1.25]), np.full((3, 1), 30.0 + 0.25 * i)], 1))
    for i in range(n_thin):
        x0, y0 = rng.uniform(1, w - 8), rng.uniform(1, h - 26)
        dx, ln = rng.uniform(0, 5.9, 3), rng.uniform(6, 24)
        dx[int(rng.integers(0, 3))] = 0.0
        xy = np.array([[x0 + dx[0], y0], [x0 + dx[1], y0 + ln], [x0 + dx[2], y0 + 0.45 * ln]])
        pos.append(np.concatenate([xy, np.full((3, 1), 5.0 + 0.25 * i)], 1))
    pos = np.asarray(pos, np.float32)
    ab, ac = pos[:, 1, :2] - pos[:, 0, :2], pos[:, 2, :2] - pos[:, 0, :2]
    swap = (ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]) > 0  # kept: cross(B - A, C - A).z < 0 for an eye at z > 0
    swap[1 + n_med:1 + n_med + 4] ^= True
    pos[swap] = pos[swap][:, [0, 2, 1]]
    thin = np.zeros(len(pos), bool)
    thin[1 + n_med + 4:] = True
    return pos, thin


def _pick(rng, values, shape):
    return np.asarray(values, np.float32)[rng.integers(0, len(values), shape)]


def hostile_shading_frame(seed, family, shader_mix=(abi.SHADER_TEXTURE, abi.SHADER_PHONG), n_lights=2, p=150.0, w=64, h=64,
                          flags=abi.FUSED_CLEAR, tame=False):
    """One frame of tame geometry whose SHADING inputs are hostile in the way `family` names (HOSTILE_FAMILIES); numpy only,
    deterministic in its arguments.  The triangles are dealt round-robin to one batch per entry of shader_mix (texture-shape: one batch
    per texture slot, the textured shaders of the mix in turn).  Odd seeds of light-edge, eye-edge and constants use non-finite values
    too, even seeds finite ones only; the exponent family takes its exponent from `p` like every other (HOSTILE_EXPONENTS is the list
    to cross it with) and arranges normals for cosines near 0 and near 1.  tame=True: the same geometry, batches, lights and seed with
    the family's hostile values left out (uv inside [0, 1]) — the twin a test compares with.  The frame carries .family and .label:
    "finite" when every shading input is finite, else "nonfinite" (by the INPUTS, whatever the interpolation makes of them)."""
    assert family in HOSTILE_FAMILIES, family
    rng = np.random.default_rng([seed, HOSTILE_FAMILIES.index(family)])
    pos, thin = _hostile_geometry(np.random.default_rng([seed, 77]), w, h)  # (the geometry depends on the seed alone)
    n = len(pos)
    t = np.zeros(n, abi.TRI_DTYPE)
    t["pos"] = pos
    nn = np.array([0.0, 0.0, 1.0]) + rng.normal(0, 0.25, (n, 3, 3))
    t["nrm"] = nn / np.linalg.norm(nn, axis=2, keepdims=True)
    t["uv"] = rng.uniform(0.05, 0.95, (n, 3, 2))
    s = w / 64.0
    eye = np.array([w / 2.0, h / 2.0, 300.0], np.float32)
    L = np.zeros((5, 2, 3), np.float32)
    L[:, 0] = np.array([[-20.0, -15.0, 300.0], [89.0, 10.0, 250.0], [-12.0, 85.0, 400.0], [80.0, 90.0, 220.0], [32.0, -30.0, 350.0]]) * [s, s, 1.0]
    L[:, 1] = (np.array([14.0, 9.0, 11.0, 7.0, 8.0]) * s)[:, None]
    if seed % 3 == 1:
        L[:, 1] *= np.array([0.6, 1.0, 1.3], np.float32)  # not grey
    L = L[:n_lights].copy()
    ka, ks, kh, kn = list(abi.DEFAULT_KA), list(abi.DEFAULT_KS), abi.DEFAULT_KH, abi.DEFAULT_KN
    k = np.arange(n)
    whole = (k % 3 == 0)[:, None, None]  # every third triangle takes ONE value for its three vertices
    if tame:
        pass
    elif family == "uv-edge":
        vals = [0.0, 1.0, 1.0 - 2.0 ** -24, -0.0, 1e-40, -0.3, 1.7, 1e6, 0.5]
        per_tri = _pick(rng, vals, (n, 1, 2))
        t["uv"] = np.where(whole, per_tri, _pick(rng, vals, (n, 3, 2)))
        t["uv"][k % 6 == 1, :, 1] = 0.5  # (some with a tame v, so that u alone decides)
    elif family == "uv-overflow":
        big = _pick(rng, [3e38, -3e38], (n, 3, 2))
        t["uv"] = np.where(rng.random((n, 3, 2)) < 0.6, big, t["uv"])
    elif family == "uv-nonfinite":
        bad = _pick(rng, [np.nan, np.inf, -np.inf], (n, 3, 2))
        count = 1 + k % 3  # one, two or three vertices
        hit = (np.arange(3)[None, :] < count[:, None])[:, :, None] & (rng.random((n, 1, 2)) < 0.7)
        t["uv"] = np.where(hit, bad, t["uv"])
    elif family == "normal-nonfinite":
        kinds = np.array([[np.nan, 0.3, 1.0], [np.inf, 0.0, 1.0], [0.2, -np.inf, 1.0], [1e30, 1e-30, 1.0], [1e20, 1e20, 1e20],
                          [1e-30, 1e-30, 1e-30], [0.0, 0.0, 0.0], [-1e30, 1e30, 1e-38], [np.inf, np.inf, -np.inf]], np.float32)
        choice = kinds[rng.integers(0, len(kinds), (n, 3))]
        hit = (rng.random((n, 3)) < 0.6)[:, :, None]
        t["nrm"] = np.where(hit, choice, t["nrm"])
    elif family == "light-edge":
        far = pos[1, 0]  # a vertex of a triangle: the light ON a fragment's (x, y)
        finite_pos = [[round(w / 2.0), round(h / 2.0), 200.0], list(eye), [w / 2.0, h / 2.0, -100.0], [1e30, 1e30, 1e30],
                      [float(round(far[0])), float(round(far[1])), 40.0], [-1e30, h / 2.0, 50.0]]
        wild_pos = [[np.nan, 10.0, 100.0], [np.inf, 10.0, 100.0], [10.0, -np.inf, np.inf], [w / 2.0, h / 2.0, np.nan]]
        finite_I = [[0, 0, 0], [-5, -5, -5], [1e-40, 1e-40, 1e-40], [1e30, 1e30, 1e30], [12, 12, 12], [6, 12, 18], [-3, 8, 1e30], [0.0, -0.0, 0.0]]
        wild_I = [[np.inf, np.inf, np.inf], [np.nan, np.nan, np.nan], [5, np.nan, 5], [np.inf, 3, -np.inf]]
        pp, ii = (finite_pos, finite_I) if seed % 2 == 0 else (finite_pos + wild_pos, finite_I + wild_I)
        for l in range(n_lights):
            if (seed + l) % 4 != 3:  # (one light in four keeps a tame position, one in five a tame intensity)
                L[l, 0] = pp[(seed // 2 * 3 + 5 * l) % len(pp)]
            if (seed + l) % 5 != 4:
                L[l, 1] = ii[(seed // 2 * 5 + 3 * l) % len(ii)]
        if seed % 2 and n_lights and np.isfinite(L).all():  # (an odd seed always has a non-finite value: in the LAST light)
            if seed % 4 == 1:
                L[-1, 0] = wild_pos[(seed // 4) % len(wild_pos)]
            else:
                L[-1, 1] = wild_I[(seed // 4) % len(wild_I)]
    elif family == "eye-edge":
        v = pos[2, 1]
        eyes = [v, [np.nan, 0.0, 1.0], [w / 2.0, h / 2.0, 0.0], [0.0, np.inf, 300.0], pos[len(pos) - 3, 0], [w / 2.0, h / 2.0, np.nan],
                [1e30, -1e30, 1e30], [np.inf, np.inf, np.inf]]
        eye = np.asarray(eyes[(seed % 2) + 2 * ((seed // 2) % 4)], np.float32)  # even seeds: the finite ones
    elif family == "constants":
        fin = [[-0.5, -0.5, -0.5], [0, 0, 0], [3, 3, 3], [0.005, 0.02, 0.005], [-0.1, 2.0, 0.3], [1e30, 1e30, 1e30], [1e-40, 0, -0.0]]
        wild = [[np.nan, np.nan, np.nan], [np.inf, np.inf, np.inf], [0.1, np.nan, 0.1], [-np.inf, 0.5, np.inf]]
        hs_fin, hs_wild = [0.0, -0.2, 1e30, 5.0, -1e30, 1e-40], [np.nan, np.inf, -np.inf]
        kk, hh = (fin, hs_fin) if seed % 2 == 0 else (fin + wild, hs_fin + hs_wild)
        j = seed // 2
        ka, ks = kk[(3 * j) % len(kk)], kk[(5 * j + 2) % len(kk)]
        if j % 3 == 1:
            ka = list(abi.DEFAULT_KA)  # (one of the two stays tame in a third of the seeds)
        if j % 3 == 2:
            ks = list(abi.DEFAULT_KS)
        kh, kn = hh[(2 * j) % len(hh)], hh[(3 * j + 1) % len(hh)]
        if seed % 2 and np.isfinite(np.float32(list(ka) + list(ks) + [kh, kn])).all():  # (an odd seed always has a non-finite value)
            ks = wild[j % len(wild)]
    elif family == "exponent":
        # the half-vector is (0, 0, 1) within a few degrees everywhere (eye and lights far above the image): normals near it give
        # cosAlpha near 1, normals near the image plane give cosAlpha near 0 (some just below: clamped to exactly 0)
        L[:, 0] = np.array([w / 2.0 + 0.37, h / 2.0 + 0.21, 3000.0], np.float32) + np.arange(n_lights, dtype=np.float32)[:, None] * _F32(7.0)
        eye = np.array([w / 2.0 + 3.0, h / 2.0 - 2.0, 3000.0], np.float32)
        flat = np.array([1.0, 0.3, 0.0]) + rng.normal(0, 0.02, (n, 3, 3))
        nn = np.where((k % 2 == 1)[:, None, None], flat, np.array([0.0, 0.0, 1.0]) + rng.normal(0, 0.03, (n, 3, 3)))
        t["nrm"] = nn / np.linalg.norm(nn, axis=2, keepdims=True)
    if family == "texture-shape":
        slots = sorted(HOSTILE_TEX_SHAPES)
        textured = [sh for sh in shader_mix if sh in TEXTURED] or [abi.SHADER_TEXTURE]
        plan = [(textured[(b + seed) % len(textured)], slots[(b + seed) % len(slots)]) for b in range(len(slots))]
        if not tame:  # uv over the whole texture and its borders: every texel of the small ones, both ends of the padded rows
            t["uv"] = np.where(whole, _pick(rng, [0.0, 0.999, 0.5, 1.0], (n, 1, 2)), rng.uniform(-0.05, 1.05, (n, 3, 2)))
    else:
        plan = [(sh, HOSTILE_TEX if sh in TEXTURED else -1) for sh in shader_mix]
    batches = [(sh, slot, t[b::len(plan)]) for b, (sh, slot) in enumerate(plan)]
    f = abi.Frame(w, h, tuple(float(x) for x in eye), L, batches, flags, ka=ka, ks=ks, p=p, kh=kh, kn=kn)
    f.family = family
    f.label = hostile_label(f)
    return f


def hostile_label(f):
    """"finite" when every value the shaders read from frame f is finite (uv, normals, lights, eye, ka, ks, p, kh, kn)"""
    parts = [np.float32([f.c.p, f.c.kh, f.c.kn]), np.float32(list(f.c.eye) + list(f.c.ka) + list(f.c.ks)), f.lights["pos"], f.lights["intensity"]]
    parts += [x[key] for x in f.tris for key in ("uv", "nrm")]
    return "finite" if all(np.isfinite(x).all() for x in parts) else "nonfinite"


MIX_PLAIN = (abi.SHADER_TEXTURE, abi.SHADER_PHONG, abi.SHADER_NORMAL)
MIX_ALL = (abi.SHADER_TEXTURE, abi.SHADER_PHONG, abi.SHADER_BUMP, abi.SHADER_DISPLACEMENT, abi.SHADER_NORMAL)
# families whose every frame / whose even seeds are labelled finite (the others: never)
HOSTILE_ALWAYS_FINITE = ("uv-edge", "uv-overflow", "exponent", "texture-shape")
HOSTILE_EVEN_FINITE = ("light-edge", "eye-edge", "constants")


def tolerance_frames(family, size=64):
    """the frames the tolerance mode is held to (tests/test_gpu_shading_edges.py) -> [(name, frame, bounded)]: four seeds x {a mix the
    ApproxMath builds shade, a mix with a BUMP batch: the exact generic build}.  bounded = the frame is labelled finite and (pinned on
    the CPU by tests/test_oracle_shading_edges.py) the oracle's pre-truncation probe is finite at every covered pixel: the frames on
    which check_approx's value bounds are asserted"""
    out = []
    for seed in (0, 1, 2, 3):
        for mix in (MIX_PLAIN, MIX_ALL):
            p = (150.0, 32.0, 0.0, 1.0)[seed] if family == "exponent" else (150.0, 7.5)[seed % 2]
            f = hostile_shading_frame(seed, family, mix, 1 + seed % 4, p, size, size)
            bounded = family in HOSTILE_ALWAYS_FINITE or (family in HOSTILE_EVEN_FINITE and seed % 2 == 0)
            out.append((f"{family} seed {seed} {'plain' if mix is MIX_PLAIN else 'all'}", f, bounded))
    return out


def dump_frames(path, frames):
    """hostile_textures() and the frames as the file tests/cpp/oracle_asan_main.c reads (its header states the layout)"""
    import struct
    with open(path, "wb") as o:
        tex = hostile_textures()
        o.write(b"SRZF" + struct.pack("<I", len(tex)))
        for slot, (t, stride) in tex.items():
            o.write(struct.pack("<4i", slot, t.shape[1], t.shape[0], stride) + padded_rows(t, stride).tobytes())
        o.write(struct.pack("<I", len(frames)))
        for f in frames:
            c = f.c
            o.write(struct.pack("<2i12f3I", c.width, c.height, *c.eye, *c.ka, *c.ks, c.p, c.kh, c.kn, c.n_lights, c.n_batches, c.flags))
            o.write(f.lights.tobytes())
            for b, t in enumerate(f.tris):
                o.write(struct.pack("<2iI", f._batches[b].shader, f._batches[b].tex_id, len(t)) + t.tobytes())


# ------------------------------------------------------------------------------------------------ comparison
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def words(t):
    return t.cpu().numpy().view(np.uint32)


def same(gpu, ref, what):
    """the four planes are bit-identical (gpu[p], ref[p]: plane p, of one frame or of a whole set)"""
    for p in range(4):
        g, r = bits(gpu[p]), bits(ref[p])
        bad = g != r
        assert not bad.any(), f"{what}: plane {p} differs at {int(bad.sum())} pixels, first {np.argwhere(bad)[:4].tolist()}: " \
                              f"got {g[bad][:4]} want {r[bad][:4]}"


def compare(gpu, ref, name):
    """the stated tolerance of the exact mode (tests/test_gpu_parity.py): z bit-identical, |Δcolour| <= 1e-3 on at most 1e-5 of the
    covered pixels (the pow corner).  Returns the number of colour values that are not bit-identical."""
    gz, rz = gpu[0], ref[0]
    n_cov = max(1, int(np.isfinite(rz).sum()))
    z_same = np.array_equal(bits(gz), bits(rz))
    dc = np.maximum.reduce([np.abs(g.astype(np.float64) - r.astype(np.float64)) for g, r in zip(gpu[1:], ref[1:])])
    nan_differs = np.logical_or.reduce([np.isnan(g) != np.isnan(r) for g, r in zip(gpu[1:], ref[1:])])  # (in ANY colour plane)
    dc = np.nan_to_num(dc, nan=0.0) + np.where(nan_differs, 1e9, 0.0)
    n_diff = int(sum((bits(g) != bits(r)).sum() for g, r in zip(gpu[1:], ref[1:])))
    print(f"[{name}] covered={n_cov} z_bit_identical={z_same} colour_values_not_bit_identical={n_diff} max_dcolour={dc.max():.3g}")
    assert z_same, f"{name}: z-buffer is not bit-identical"
    assert dc.max() <= 1e-3 and (dc > 0).sum() <= max(1, int(1e-5 * n_cov)), f"{name}: colour outside the stated tolerance"
    return n_diff


def changed(a, b):
    """fraction of the covered pixels of oracle frame a whose colour differs from b's by more than the stated tolerance"""
    cov = np.isfinite(a[0])
    d = np.maximum.reduce([np.abs(x.astype(np.float64) - y.astype(np.float64)) for x, y in zip(a[1:], b[1:])])
    return float((d[cov] > 1e-3).mean())


V_TOL, S_EPS = 0.5, 1e-3


def check_approx(gpu, gst, ref, rst, pre, s_class, name):
    """the stated tolerance of the tolerance mode (tests/test_gpu_approx.py), on what oracle_with_probes returns"""
    assert gst == rst, (name, gst, rst)
    assert np.array_equal(bits(gpu[0]), bits(ref[0])), f"{name}: z plane is not bit-identical in the tolerance mode"
    cov = np.isfinite(ref[0])
    n_cov, n_s = int(cov.sum()), int((s_class & cov).sum())
    worst_v, flips, exact = 0.0, 0, 0
    for c in (1, 2, 3):
        g, r, p = gpu[c].astype(np.float64), ref[c].astype(np.float64), pre[c].astype(np.float64)
        assert np.array_equal(g[~cov], r[~cov]), f"{name}: uncovered pixels differ"
        # (a NaN on one side only makes d a NaN, and every `d > bound` below false: NaN-ness is compared on its own)
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{name}: channel {c}: {int((np.isnan(g) != np.isnan(r)).sum())} pixels are NaN on one side only"
        d = np.abs(g - r)
        v = cov & ~s_class
        worst_v = max(worst_v, float(d[v].max()) if v.any() else 0.0)
        out = v & (d > V_TOL)
        if out.any():
            ys, xs = np.nonzero(out)
            print(f"[approx {name}] channel {c}: {int(out.sum())} V values outside {V_TOL}, first at (x, y) {list(zip(xs[:6].tolist(), ys[:6].tolist()))}: "
                  f"gpu {g[out][:6]} oracle {r[out][:6]}")
        assert not out.any(), f"{name}: V pixel outside {V_TOL}: max {d[v].max()}"
        s = cov & s_class
        diff = s & (d != 0)
        near = np.abs(p - np.rint(p)) <= S_EPS
        assert not (diff & ~near).any(), (f"{name}: S pixel differs where the pre-truncation value is not within {S_EPS} of an integer: "
                                          f"{int((diff & ~near).sum())} values, e.g. pre {p[diff & ~near][:4]} gpu {g[diff & ~near][:4]}")
        assert not (d[diff] > 1.0).any(), f"{name}: S pixel off by more than one level"
        flips += int(diff.sum())
        exact += int((bits(gpu[c]) == bits(ref[c]))[cov].sum())
    print(f"[approx {name}] covered={n_cov} S-class={n_s} max|dV|={worst_v:.4g} S truncation flips={flips} (of {3 * n_s} values) "
          f"bit-identical colour values={exact} of {3 * n_cov}")
    assert flips <= max(3, int(2e-3 * 3 * max(n_s, 1))), f"{name}: too many truncation flips"
    return worst_v, flips


@functools.lru_cache(maxsize=None)
def golden():
    """(golden.json, golden_samples.npz, the make_golden module that wrote them)"""
    sys.path.insert(0, GOLDEN_DIR)
    import make_golden
    return json.load(open(os.path.join(GOLDEN_DIR, "golden.json"))), np.load(os.path.join(GOLDEN_DIR, "golden_samples.npz")), make_golden


def check_against_golden(name, planes, stats=None, exact=True):
    """compare planes (the oracle's or the GPU's) with the committed fixture `name`"""
    gold, samples, make_golden = golden()
    g = gold[name]
    s = samples[name]
    z, c0, c1, c2 = planes
    xs, ys = s[:, 0].astype(int), s[:, 1].astype(int)
    assert np.array_equal(z[ys, xs].view(np.uint32), s[:, 2]), "sampled z differs"
    for k, p in enumerate((c0, c1, c2)):
        got = p[ys, xs]
        want = s[:, 3 + k].view(np.float32)
        if exact:
            assert np.array_equal(got.view(np.uint32), s[:, 3 + k]), f"sampled c{k} differs"
        else:
            assert np.abs(got - want).max() <= 0.5
    assert int(np.isfinite(z).sum()) == g["covered"]
    assert make_golden.digest(z) == g["sha256"]["z"]
    if exact:
        for k, p in zip(("c0", "c1", "c2"), (c0, c1, c2)):
            assert make_golden.digest(p) == g["sha256"][k]
    if stats is not None:
        assert stats == g["stats"]


# ------------------------------------------------------------------------------------------------ running
def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def render(ctx, frames, flags=abi.FUSED_CLEAR, prefill=None, vis=False):
    """a set of the frames and its colour (or visibility) render into a fresh buffer (prefill: [n, 4, rows, W] float32 the buffer
    starts with, else zeros) → (frameset, [n, 4, local_rows, W] float32 tensor)"""
    import torch
    fs = ctx.frameset(frames)
    out = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    if prefill is not None:
        out.copy_(torch.as_tensor(prefill))
    (fs.render_visibility if vis else fs.render)(out.data_ptr(), fs.out_bytes, flags, stream())
    torch.cuda.synchronize()
    return fs, out


def sceneset_update(ctx, fs, sframes, sync=True):
    """srz_sceneset_update of set fs with the abi.SceneFrame's (the binding has no method for it); SrzError when it refuses.  The
    upload is asynchronous on the context's own stream, which is not ordered against the stream the tests render on: waited for
    (sync=False: not waited for — for work that follows on the context's own stream, srz_target_draw)"""
    import srz
    sframes = list(sframes)
    ctx._check(srz.lib().srz_sceneset_update(ctx.h, fs.h, abi.scene_frames_array(sframes), len(sframes)))
    fs.frames = sframes  # (the set's frames own the arrays the call read: kept alive like the constructor's)
    if sync:
        ctx.sync()


def run(fs, flags=abi.FUSED_CLEAR):
    """(colour render, shade of the visibility render into a second buffer) of the set, both as uint32 words, and the visibility buffer"""
    import torch
    col = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    vis, out = torch.zeros_like(col), torch.zeros_like(col)
    s = stream()
    fs.render(col.data_ptr(), fs.out_bytes, flags, s)
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, flags, s)
    fs.shade_visibility(vis.data_ptr(), out.data_ptr(), fs.out_bytes, flags, s)
    torch.cuda.synchronize()
    return words(col), words(out), vis


def run_both(ctx, orc, f, planes_init=None, want_stats=True, what=""):
    """one frame through the oracle and through srz_draw, each from a copy of the incoming planes if there are any; the counters are
    equal → (gpu planes, oracle planes)"""
    def clone():
        return None if planes_init is None else tuple(p.copy() for p in planes_init)
    rc, ref, rst = orc.draw(f, clone())
    assert rc == 0
    gpu, gst = ctx.draw(f, clone(), want_stats=want_stats)
    if want_stats:
        assert gst == rst, (what, gst, rst)
    return gpu, ref


def both_paths(ctx, orc, f_builder, planes_init=None, what=""):
    """run_both through the order-independent rasteriser and through the ordered one (f_builder(extra flags) → frame); both must give
    the oracle's planes bit for bit."""
    for extra in (0, abi.ORDERED_RASTER):
        gpu, ref = run_both(ctx, orc, f_builder(extra), planes_init, what=f"{what} flags+={extra}")
        same(gpu, ref, f"{what} flags+={extra}")


def oracle_with_probes(orc, f):
    """the oracle's planes and counters, and per pixel the colour in front of the scalar-tail truncation and the class (oracle.debug_s)"""
    rc, ref, rst = orc.draw(f)
    assert rc == 0
    try:
        orc.debug_s(1)
        rc1, pre, _ = orc.draw(f)
        orc.debug_s(2)
        rc2, cls, _ = orc.draw(f)
    finally:
        orc.debug_s(0)
    assert rc1 == 0 and rc2 == 0
    s_class = cls[1] == -1.0
    return ref, rst, pre, s_class


# ------------------------------------------------------------------------------------------------ the passes over a visibility buffer
# What the tests of srz_frameset_gbuffer / _motion / _interpolate / _position_grad / _antialias and of their CPU references share.
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0xdeadbeef
MIN_CLASS, MAX_AMBIGUOUS = 200, 0.005
_ref_libs = {}


def build_c(name, out, *flags):
    """tests/<name>.c with the oracle's float rules (no contraction, no fast-math) and `flags` -> the file `out`"""
    import subprocess
    subprocess.check_call(["gcc", *flags, "-ffp-contract=off", "-fno-fast-math", "-o", out, os.path.join(HERE, name + ".c"), "-lm"])
    return out


def ref_lib(name, tmpdir, signatures):
    """the reference tests/<name>.c as a shared library, built (into tmpdir) and loaded once per session; signatures: function ->
    (restype, argtypes)"""
    if name not in _ref_libs:
        import ctypes
        L = ctypes.CDLL(build_c(name, os.path.join(str(tmpdir), f"lib{name}.so"), "-O2", "-shared", "-fPIC"))
        for fn, (restype, argtypes) in signatures.items():
            getattr(L, fn).restype, getattr(L, fn).argtypes = restype, argtypes
        _ref_libs[name] = L
    return _ref_libs[name]


def word_planes(vis_words):
    """[4, rows, W] words of one frame's visibility buffer -> ([z, id, alpha, beta] as contiguous uint32 planes, (rows, W))"""
    w = np.ascontiguousarray(vis_words, np.uint32)
    assert w.ndim == 3 and w.shape[0] == 4
    return [np.ascontiguousarray(w[p]) for p in range(4)], w.shape[1:]


def frame_positions(frame):
    """[n, 9] float32: ax ay z0 bx by z1 cx cy z2 of every triangle of an abi.Frame, in stream order"""
    if not sum(len(t) for t in frame.tris):
        return np.zeros((0, 9), np.float32)
    return np.ascontiguousarray(np.concatenate([t["pos"] for t in frame.tris]).reshape(-1, 9), np.float32)


def padded_positions(frames, T):
    """[n, T, 9] float32: every frame's dense position stream, zeros behind its last triangle"""
    pos = np.zeros((len(frames), T, 9), np.float32)
    for i, f in enumerate(frames):
        pos[i, :f.n_tris] = frame_positions(f)
    return pos


def visibility(fs, flags=abi.FUSED_CLEAR):
    """the set's visibility render into a fresh buffer -> [n, 4, local_rows, W] float32 tensor"""
    import torch
    vis = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, flags, stream())
    torch.cuda.synchronize()
    return vis


def filled(shape, fill=SENTINEL):
    """an int32 tensor on the device, every word `fill` (a uint32 value)"""
    import torch
    return torch.full(shape, fill - (1 << 32) if fill >= 1 << 31 else fill, dtype=torch.int32, device="cuda")


def visibility_of(tmp_path, orc, f, max_ambiguous=None):
    """the oracle's visibility buffer of frame f (visref.Reference.expected) -> a namespace: words [4, H, W]; the masks own, v_class,
    s_class; amb, the pixels left out (id 0) because their colour decodes to no single owner; n, the frame's triangle count.  Asserted,
    so that no comparison passes vacuously: >= MIN_CLASS owned pixels of each class, the id words
    name the owned pixels and nobody else, and (max_ambiguous given) amb <= max_ambiguous of the owned and left-out pixels"""
    import types
    import visref
    words, _, amb, _, own = visref.Reference(tmp_path, f).expected(orc)
    n = sum(len(t) for t in f.tris)
    assert np.array_equal(own, ((words[1] & 0x7fffffff) - np.uint32(1)) < n)
    s_class = own & ((words[1] >> 31) != 0)
    v_class = own & ~s_class
    n_v, n_s = int(v_class.sum()), int(s_class.sum())
    print(f"owned V {n_v} S {n_s} ambiguous {amb}")
    assert n_v >= MIN_CLASS and n_s >= MIN_CLASS, (n_v, n_s)
    if max_ambiguous is not None:
        assert amb <= max_ambiguous * (n_v + n_s + amb), amb
    return types.SimpleNamespace(words=words, own=own, v_class=v_class, s_class=s_class, amb=amb, n=n)


# ------------------------------------------------------------------------------------------------ the context
def make_ctx(approx=False):
    import srz
    c = srz.Context(0)
    c.texture_upload(scenes.TEX_SPOT, scenes.spot_texture())
    if approx:
        c.set_option(abi.OPT_APPROX_SHADE, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx():
    """one context per test module that imports this fixture (`from support import ctx  # noqa: F401`), the spot texture in slot 0"""
    yield from make_ctx()


@pytest.fixture()
def actx():
    """a fresh context in the tolerance mode (SRZ_OPT_APPROX_SHADE) for every test"""
    yield from make_ctx(approx=True)


# ------------------------------------------------------------------------------------------------ the device-resident target
Z_CLEAR = 0x7f800000  # +inf: the z word of a cleared pixel; a cleared colour word is 0 (+0.0)


def overhang_pair(w, h):
    """the two triangles of test_gpu_parity.test_odd_sizes: one inside the w x h frame, one overhanging every edge behind it"""
    return np.concatenate([ccw((w * 0.1, h * 0.1), (w * 0.95, h * 0.2), (w * 0.3, h * 0.9)),
                           ccw((-5, -5), (w + 9.5, 3), (2, h + 7.25), z=60.0)])


def copy_planes(planes):
    return tuple(p.copy() for p in planes)


def assert_clear(planes, what):
    """every z word is +inf and every colour word +0.0 (words, not values: -0.0 and a NaN are not clear values)"""
    assert (bits(planes[0]) == Z_CLEAR).all(), f"{what}: z is not +inf everywhere"
    for p in (1, 2, 3):
        assert not bits(planes[p]).any(), f"{what}: colour plane {p} is not +0.0 everywhere"


def oracle_draws(orc, frames, planes=None, primitive=abi.PRIMITIVE_TRIANGLES):
    """the oracle's draws of the frames one after the other onto a copy of `planes` (None: fresh ones), none of them clearing ->
    (the planes after each draw, the counters of each draw)"""
    cur = orc.new_planes(frames[0].width, frames[0].height) if planes is None else copy_planes(planes)
    after, stats = [], []
    for f in frames:
        assert not f.c.flags & abi.FUSED_CLEAR, "a frame that clears does not accumulate"
        rc, cur, st = orc.draw(f, copy_planes(cur), primitive)
        assert rc == 0
        after.append(cur)
        stats.append(st)
    return after, stats


# ------------------------------------------------------------------------------------------------ the C++ programs of tests/cpp
def compile_cpp_program(name, out_dir):
    """tests/cpp/<name>.cpp against the host layer's headers and libraries, as a user's program would be built -> the executable"""
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "software-rasterizer_amd")
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(repo, "tests", "cpp", name + ".cpp"), "-I", os.path.join(pkg, "host", "include"),
                           "-L", pkg, "-lsrz_host", "-lsrz", f"-Wl,-rpath,{pkg}", "-o", exe])
    return exe
