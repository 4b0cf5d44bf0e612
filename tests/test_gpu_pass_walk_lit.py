"""-m gpu: the newer passes over a visibility buffer, beyond the grid's cap — tests/test_gpu_pass_walk.py's two sets (tests/walkkit.py:
`many`, 6,144 frames of four tiles, 24,576 tiles; `large`, 7 frames of 49 x 49 tiles, 16,807 tiles; tile_grid launches at most 16,384
workgroups, k_ibl_grad<true> at most 1,024) under the twenty host entries that came after that file.  What a workgroup carries from
one tile to the next, and what it computes from a frame index in the thousands, is per kernel:
  k_cube, k_cube_mip, k_cube_level                     texture_cube, texture_cube_mip, cube_level: f * tex_frame_stride
  k_cube_grad, k_cube_mip_grad                         texture_cube_grad, texture_cube_mip_grad: the LDS table of texels, per-frame cubes
  k_persp, k_interp_deriv_persp, k_persp_grad          perspective, interpolate_deriv_persp, perspective_grad: per-frame q; the LDS table
  k_shadow, k_shadow_grad<true>, k_shadow_grad<false>  shadow, shadow_grad with and without d_gmap: per-frame maps; the LDS table
  k_normal_map, k_normal_map_grad                      normal_map, normal_map_grad
  k_light, k_light_grad<true>, <false>, k_light_fold   light, light_grad with and without d_gpar: the LDS partials, the work buffer's
  k_microfacet, k_microfacet_grad<true>, <false>       microfacet, microfacet_grad the same         rows, the fold over tiles and frames
  k_reflect, k_reflect_grad                            reflect, reflect_grad: f * par_stride of the eye
  k_ibl, k_ibl_grad<true>, k_ibl_grad<false>           ibl, ibl_grad with and without d_gtab: one LDS table per workgroup, flushed once
Every kernel of that list is launched on both sets.  The visibility buffer is the GPU's own render_visibility; directions, their
derivatives and the shading normals are the GPU's own interpolate / interpolate_deriv of seeded attributes; the other planes are
seeded per world, NaN at nobody's pixels.  The expected values are the references' of the passes' own tests (cuberef, cubemipref,
perspref, shadowref, tangentref, lightref, microfacetref, iblref) on the device's words, with those tests' bounds: the deterministic
planes bit for bit (a NaN on one side must be a NaN on the other); the float-atomic sums within the reference's Grad.bound, gamma_n *
sum |term|, gamma_n = n u / (1 - n u), u = 2^-24 — bit for bit where n = 1, exactly 0 where n = 0.  Every output starts from the
sentinel; `many` also runs with SRZ_FUSED_CLEAR.

gamma_n grows with n, so a sum of millions of terms would pass with a whole tile lost.  The inputs are therefore dealt so that the
bound can see a tile (walkkit.teeth, asserted from the reference alone, after the kernel's own checks): per-frame cubes, maps and q on
`many`; on `large` a 64 x 64 cube and a 256 x 256 map, which directions and coordinates spread thinly enough; the ibl table's
coordinates dealt per tile (walkkit.deal_ibl).  On `large` the per-tile pass of the reference takes every 7th tile and all tiles of
frame 6, and the condition is stated over that sample; gq on `large` (a few huge triangles) cannot meet it: its share is printed.

d_gpar is reduced in a fixed tree — the tile, a frame's tiles in tile order, the frames in frame order (include/srz.h) —, so beyond
the bound it is held bit for bit to the rows the same frames give in a set below the cap, to the frame-order float32 sum for a shared
parameter frame, and to a second launch."""
import numpy as np
import pytest
import torch

import cubemipref
import cuberef
import iblref
import lightref
import microfacetref
import perspref
import shadowref
import tangentref
import walkkit
from support import SENTINEL, ctx, filled, stream, visibility, words  # noqa: F401
from walkkit import F, SHAPES, Shares, check_gpar, check_gtab, check_nobody, check_sum, dev, pre, same, teeth

pytestmark = pytest.mark.gpu

N_LIGHTS, P = 3, 5
BIAS, WIDTH = 0.375, 5.0  # tests/test_gpu_shadow.py's: one of shadowref.BIASES, the soft width
CUBE_N = {"many": 4, "large": 64}
MAP_WH = {"many": 8, "large": 256}
TABLE = {"many": 64, "large": 8}
SMALL_SET = (0, 7, 8, 4095, 4096, 4103, 6143)  # many: with 16,384 workgroups the frames from 4,096 on are reached on a later trip


@pytest.fixture(scope="module")
def worlds(ctx):
    yield from walkkit.make_worlds(ctx)


def ptr(t):
    return None if t is None else t.data_ptr()


def fl(fused):
    return F if fused else 0


def per_frame(w):
    """many has one cube and one shadow map per frame, large one for all"""
    return w.name == "many"


def of(a, i, per):
    """frame i's part of a per-frame input, or the shared one"""
    return a[i] if per else a


def last_owned(w):
    """(frame, row, column) of the last owned pixel of the last frame: a pixel of the walk's second trip"""
    f = w.n - 1
    r, c = np.argwhere(w.own[f])[-1]
    return f, int(r), int(c)


def reads_its_own(w, expect, what):
    """expect(i, j): frame i's expected words with frame j's part of a per-frame input — at least 90 % of the sampled frames must give
    other words with their neighbour's part"""
    some = range(0, w.n, max(1, w.n // 64))
    differ = [expect(i, i).tobytes() != expect(i, (i + 1) % w.n).tobytes() for i in some]
    assert np.mean(differ) >= 0.9, (what, float(np.mean(differ)))


def tile_shares(w, shape, per, tile_mag):
    """walkkit.Shares of an output of `shape` (per: its first axis is the frame) from tile_mag(f, rs, cs), the sums of |term| of one
    tile's pixels alone in the shape of one frame's part"""
    shares = Shares(shape)
    for _, f, rs, cs in w.tiles():
        shares.add(tile_mag(f, rs, cs), f if per else ...)
    return shares


# ------------------------------------------------------------------------------------------------------ inputs, once per world
def make_dirs(w):
    """seeded direction attributes through the GPU's interpolate and interpolate_deriv → (dirs, its copy on the device, dird, its copy)"""
    a = w.rng(11).normal(0, 1, (w.n, w.T, 3, 3)).astype(np.float32)
    return w.interpolated(a) + w.interpolated(a, deriv=True)


def make_lookup_dirs(w, tmp):
    """the directions of the cube lookups.  many: make_dirs' — every frame has a cube of its own.  large: the dozen triangles of a
    frame sweep the shared cube so slowly that a texel collects from hundreds of tiles, most of them with a sliver of a weight, and the
    bound sees none of them; so the planes are dealt per tile (walkkit.cube_dirs) — checked against the reference's own taps —, and one
    pixel of the second trip points into the corner cell of -Z that the deal leaves free: texels of a single add → (dirs, its copy)"""
    if w.name == "many":
        return dirs_of(w)[:2]
    N = CUBE_N[w.name]
    d, face, x, y = walkkit.cube_dirs(w.tile_of, int(w.tile_of.max()) + 1, N, w.rng(26))
    f, r, c = last_owned(w)
    nrm, su, sv = np.float32(cuberef.AXES[5])
    d[f, :, r, c] = nrm + np.float32((0.6 / N) * 2 - 1) * (su + sv)  # (x = y = 0.1: between the texel centres 0 and 1)
    some = d[::3, :, ::97, ::89]
    taps = cuberef.taps(tmp, N, np.moveaxis(some, 1, -1))
    t = w.tile_of[::3, ::97, ::89].ravel()
    assert np.array_equal(taps["face"], face[t]) and np.array_equal(taps["x0y0"], np.stack([x[t], y[t]], 1)), "cube_dirs' cells are not the reference's"
    lone = cuberef.taps(tmp, N, d[f, :, r, c][None])
    assert lone["face"][0] == 5 and tuple(lone["x0y0"][0]) == (0, 0)
    return w.nobody_nan(d)


def make_cube(w):
    """many: one 4 x 4 cube of five channels per frame; large: one 64 x 64 cube of two channels → (levels, the cube on the device, the
    pyramid's levels above 0 on the device)"""
    N = CUBE_N[w.name]
    cube = cuberef.make_cube(21, N, w.C, frames=w.n if w.name == "many" else None)
    levels = cubemipref.build(cube)
    assert len(levels) > 1
    return levels, dev(cube), dev(cubemipref.flat(levels, 1))


def make_lam(w):
    """the level of detail, reaching beyond both ends.  many: uniform over (-0.5, L - 0.5) per pixel.  large: a texel of a level
    above 0 takes in sixteen cells and more of cube_dirs' deal, so there one tile in sixteen (by hash) draws its pixels' levels over
    (0, L - 0.5) and the others stay at or below 0 — the levels above 0 then collect from few tiles too"""
    L, rng = len(w.memo("cube", make_cube)[0]), w.rng(12)
    lam = rng.uniform(-0.5, L - 0.5, w.shape(1))
    if w.name == "large":
        high = (walkkit.mix(np.arange(int(w.tile_of.max()) + 1) * 2 + 1) % np.uint64(16) == 0)[w.tile_of][:, None]
        low = np.where(rng.random(lam.shape) < 0.5, rng.uniform(-0.5, 0.0, lam.shape), 0.0)
        lam = np.where(high, rng.uniform(0.0, L - 0.5, lam.shape), low)
    lam, d = w.nobody_nan(lam)
    assert (lam[:, 0][w.own] < 0).any() and (lam[:, 0][w.own] > L - 1).any()  # both ends
    return lam, d


def make_q(w):
    rng = w.rng(13)
    q = (rng.uniform(0.25, 4.0, (w.n, w.T, 3)) * 2.0 ** rng.integers(-3, 4, (w.n, w.T, 1))).astype(np.float32)
    return q, dev(q)


def make_shadow(w):
    """(map, its copy, sc, its copy).  many: one 8 x 8 map per frame, shadowref.make_coords' coordinates.  large: one map of 256 x 256;
    with coordinates drawn per pixel over the whole map every texel would collect a term or two from each of some seventy tiles, which
    the bound just fails to tell apart, so sx, sy are dealt per tile (walkkit.shadow_coords), sd is make_coords'; the last columns only
    one pixel of the second trip looks up, with e = 0 at one corner: a texel of a single add"""
    m = MAP_WH[w.name]
    depth = shadowref.make_map(31, m, m, frames=w.n if w.name == "many" else None)
    sc = np.ascontiguousarray(shadowref.make_coords(32, (w.n,) + tuple(w.v.shape[2:]), m, m).transpose(1, 0, 2, 3))
    if w.name == "large":
        sc = walkkit.shadow_coords(w.tile_of, int(w.tile_of.max()) + 1, m, sc[:, 2], w.rng(27))
        f, r, c = last_owned(w)
        sc[f, :, r, c] = (m - 1.5, 10.5, depth[10, m - 2] + np.float32(BIAS))
    scw, s = w.nobody_nan(sc)
    return depth, dev(depth), scw, s


def make_shading(w):
    """shading normals of any length facing +z through the GPU's interpolate, positions by hand: a ramp over the frame, x and y in
    [-1, 1), z a tilted plane that differs from frame to frame → (nrm, its copy, pos, its copy)"""
    rng = w.rng(14)
    a = rng.normal(0, 0.35, (w.n, w.T, 3, 3))
    a[..., 2] = np.abs(a[..., 2]) + 0.6
    a *= rng.uniform(0.5, 3.0, (w.n, w.T, 3, 1))
    nw, nrm = w.interpolated(a.astype(np.float32))
    rows, W = w.v.shape[2:]
    ys, xs = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    x, y = 2 * xs / W - 1, 2 * ys / rows - 1
    z = (0.1 * x - 0.2 * y)[None] + 0.05 * (np.arange(w.n) % 16)[:, None, None]
    pw, pos = w.nobody_nan(np.stack([np.broadcast_to(x, z.shape), np.broadcast_to(y, z.shape), z], 1))
    return nw, nrm, pw, pos


def make_colour(w):
    """kd / base colour in (0.1, 1), given on many and null on large → (planes or None, their copy or None)"""
    if w.name == "large":
        return None, None
    return w.nobody_nan(w.rng(15).uniform(0.1, 1.0, w.shape(3)))


def make_mat(w):
    """roughness and metallic as microfacetref.make_planes draws them: one in four over [-0.1, 1.1], the others inside (0.1, 0.95)"""
    rng = w.rng(16)
    s = w.shape(2)
    return w.nobody_nan(np.where(rng.random(s) < 0.25, rng.uniform(-0.1, 1.1, s), rng.uniform(0.1, 0.95, s)))


def make_tangent(w):
    """(tan [n, 4, ..], m [n, 3, ..]) as tangentref.make_planes draws them, and their copies"""
    rng = w.rng(17)
    tan = np.zeros(w.shape(4))
    tan[:, 0:3] = rng.normal(0, 0.3, w.shape(3))
    tan[:, 0] = np.abs(tan[:, 0]) + 0.6
    tan[:, 0:3] *= rng.uniform(0.3, 2.0, w.shape(1))
    tan[:, 3] = np.where(rng.random(tan[:, 3].shape) < 0.5, -1.0, 1.0)
    m = rng.normal(0, 0.5, w.shape(3))
    m[:, 2] = np.abs(m[:, 2]) + 0.4
    return w.nobody_nan(tan) + w.nobody_nan(m)


def make_ibl(w):
    """ibl's planes with nv and the roughness dealt per tile (walkkit.deal_ibl, ibl_coords) → (tab, base, mat, nv, irr, spec) as
    float32 arrays and the same on the device (base None on large)"""
    t, rng = TABLE[w.name], w.rng(18)
    counts = np.bincount(w.tile_of[w.own], minlength=int(w.tile_of.max()) + 1)
    cx, cy = walkkit.deal_ibl(counts, t)
    assert (cx >= 0).sum() >= 100 and (cx < 0).sum() >= 100
    nv, rough = walkkit.ibl_coords(w.tile_of, w.own, cx, cy, t, rng)
    s = w.shape(1)
    beyond = np.where(rng.random(s) < 0.5, rng.uniform(-0.2, -0.03, s), rng.uniform(1.03, 1.2, s))
    metal = np.where(rng.random(s) < 0.125, beyond, rng.uniform(0.05, 0.95, s))
    mat = np.concatenate([rough[:, None], metal], 1)
    arrays = [iblref.smooth_table(t), w.memo("colour", make_colour)[0], mat, nv, rng.uniform(0, 2, w.shape(3)), rng.uniform(0, 2, w.shape(3))]
    arrays[2:] = [w.nobody_nan(a)[0] for a in arrays[2:]]
    return arrays, [None if a is None else dev(a) for a in arrays]


def make_params(w, ref):
    """one parameter frame per frame of the set"""
    return ref.make_params(19, N_LIGHTS, frames=w.n)


def dirs_of(w):
    return w.memo("dirs", make_dirs)


def lookup_dirs_of(w, tmp):
    return w.memo("lookup dirs", lambda w: make_lookup_dirs(w, tmp))


def cube_of(w):
    return w.memo("cube", make_cube)


def shading_of(w):
    return w.memo("shading", make_shading)


def gout_of(w, n_ch, salt=20):
    return w.memo(("gout", n_ch), lambda w: w.seeded(salt + n_ch, n_ch, 2.0))


# ------------------------------------------------------------------------------------------------------ the cube lookups
def run_texture_cube(tmp, w, fused):
    fs, C = w.fs, w.C
    (dw, dirs), (levels, t, _) = lookup_dirs_of(w, tmp), cube_of(w)
    cube = levels[0]
    out = filled(w.shape(C))
    fs.texture_cube(w.vis.data_ptr(), dirs.data_ptr(), t.data_ptr(), cube.shape[-2], C, w.n if per_frame(w) else 1, out.data_ptr(),
                    fs.interpolate_bytes(C), fl(fused), stream())
    torch.cuda.synchronize()
    expect = lambda i, j: cuberef.forward(tmp, of(cube, j, per_frame(w)), w.n_tris[i], w.v[i, 1], dw[i], fused, pre(w, C))  # noqa: E731
    got = words(out)
    same(got, np.stack([expect(i, i) for i in range(w.n)]), "texture_cube")
    check_nobody(w, got, fused, "texture_cube")
    if per_frame(w) and not fused:
        reads_its_own(w, expect, "texture_cube")


def ref_cube_grad(tmp, w, fused):
    """(one cuberef.Grad per cube, the gdir planes of every frame)"""
    (dw, _), cube, (gout, _), per = lookup_dirs_of(w, tmp), cube_of(w)[0][0], w.gout, per_frame(w)
    accs = [cuberef.Grad(cube.shape[-4:]) for _ in range(w.n if per else 1)]
    return accs, [cuberef.grad(tmp, of(cube, i, per), w.n_tris[i], w.v[i, 1], dw[i], gout[i], accs[i if per else 0], True, fused, pre(w, 3))
                  for i in range(w.n)]


def summed(accs, per, mag="gabs", count=lambda a: a.count[..., None]):
    """(sums of |term|, counts) of the Grads, stacked over the frames for a per-frame output"""
    m, c = np.stack([getattr(a, mag) for a in accs]), np.stack([count(a) for a in accs])
    return (m, c) if per else (m[0], c[0])


def teeth_cube_grad(tmp, w, accs):
    (dw, _), cube, (gout, _), per = lookup_dirs_of(w, tmp), cube_of(w)[0][0], w.gout, per_frame(w)

    def tile(f, rs, cs):
        a = cuberef.Grad(cube.shape[-4:])
        cuberef.grad(tmp, of(cube, f, per), w.n_tris[f], w.v[f, 1][rs, cs], dw[f][:, rs, cs], gout[f][:, rs, cs], a, False)
        return a.gabs
    mag, cnt = summed(accs, per)
    teeth(tile_shares(w, mag.shape, per, tile), mag, cnt, "cube gtex")


def run_texture_cube_grad(tmp, w, fused):
    fs, C = w.fs, w.C
    (_, dirs), (levels, t, _), (_, g) = lookup_dirs_of(w, tmp), cube_of(w), w.gout
    cube = levels[0]
    per = per_frame(w)
    gt, gd = torch.zeros_like(t), filled(w.shape(3))
    fs.texture_cube_grad(w.vis.data_ptr(), dirs.data_ptr(), g.data_ptr(), t.data_ptr(), cube.shape[-2], C, w.n if per else 1, gt.data_ptr(),
                         gd.data_ptr(), fl(fused), stream())
    torch.cuda.synchronize()
    accs, want = ref_cube_grad(tmp, w, fused)
    got = words(gd)
    same(got, np.stack(want), "cube gdir")
    check_nobody(w, got, fused, "cube gdir")
    mag, cnt = np.stack([a.gabs for a in accs]), np.stack([a.count for a in accs])[..., None]
    check_sum(gt.cpu().numpy(), np.stack([a.gtex for a in accs]), mag, cnt, "cube gtex")
    if not fused:
        teeth_cube_grad(tmp, w, accs)


def levels_of(levels, i, per):
    return [of(l, i, per) for l in levels]


def run_texture_cube_mip(tmp, w, fused):
    fs, C = w.fs, w.C
    (dw, dirs), (levels, t, mip), (lw, lam) = lookup_dirs_of(w, tmp), cube_of(w), w.memo("lam", make_lam)
    per, L = per_frame(w), len(levels)
    out = filled(w.shape(C))
    fs.texture_cube_mip(w.vis.data_ptr(), dirs.data_ptr(), lam.data_ptr(), t.data_ptr(), levels[0].shape[-2], C, w.n if per else 1, mip.data_ptr(),
                        L, out.data_ptr(), fs.interpolate_bytes(C), fl(fused), stream())
    torch.cuda.synchronize()
    expect = lambda i, j: cubemipref.forward(tmp, levels_of(levels, j, per), w.n_tris[i], w.v[i, 1], dw[i], lw[i, 0], fused, pre(w, C))  # noqa: E731
    got = words(out)
    same(got, np.stack([expect(i, i) for i in range(w.n)]), "texture_cube_mip")
    check_nobody(w, got, fused, "texture_cube_mip")
    if per and not fused:
        reads_its_own(w, expect, "texture_cube_mip")


def ref_cube_mip_grad(tmp, w, fused):
    """(one cubemipref.Grad per cube, (gdir, glam) of every frame)"""
    (dw, _), levels, (lw, _), (gout, _), per = lookup_dirs_of(w, tmp), cube_of(w)[0], w.memo("lam", make_lam), w.gout, per_frame(w)
    accs = [cubemipref.Grad(levels[0].shape[-2], w.C, len(levels)) for _ in range(w.n if per else 1)]
    return accs, [cubemipref.grad(tmp, levels_of(levels, i, per), w.n_tris[i], w.v[i, 1], dw[i], lw[i, 0], gout[i], accs[i if per else 0], fused=fused,
                                  prefill=SENTINEL) for i in range(w.n)]


def teeth_cube_mip_grad(tmp, w, accs):
    """over the whole pyramid, level 0 first"""
    (dw, _), levels, (lw, _), (gout, _), per = lookup_dirs_of(w, tmp), cube_of(w)[0], w.memo("lam", make_lam), w.gout, per_frame(w)

    def tile(f, rs, cs):
        a = cubemipref.Grad(levels[0].shape[-2], w.C, len(levels))
        cubemipref.grad(tmp, levels_of(levels, f, per), w.n_tris[f], w.v[f, 1][rs, cs], dw[f][:, rs, cs], lw[f, 0][rs, cs], gout[f][:, rs, cs], a,
                        False, False)
        return a.gabs
    mag, cnt = summed(accs, per, count=lambda a: np.repeat(a.count, w.C))
    teeth(tile_shares(w, mag.shape, per, tile), mag, cnt, "cube gtex and gmip")


def run_texture_cube_mip_grad(tmp, w, fused):
    fs, C = w.fs, w.C
    (_, dirs), (levels, t, mip), (_, lam), (_, g) = lookup_dirs_of(w, tmp), cube_of(w), w.memo("lam", make_lam), w.gout
    per, L, N = per_frame(w), len(levels), levels[0].shape[-2]
    gt, gm, gd, gl = torch.zeros_like(t), torch.zeros_like(mip), filled(w.shape(3)), filled(w.shape(1))
    fs.texture_cube_mip_grad(w.vis.data_ptr(), dirs.data_ptr(), lam.data_ptr(), g.data_ptr(), t.data_ptr(), mip.data_ptr(), N, C, w.n if per else 1,
                             L, gt.data_ptr(), gm.data_ptr(), gd.data_ptr(), gl.data_ptr(), fl(fused), stream())
    torch.cuda.synchronize()
    accs, want = ref_cube_mip_grad(tmp, w, fused)
    for got, want_p, what in ((words(gd), np.stack([a for a, _ in want]), "cube mip gdir"), (words(gl), np.stack([b[None] for _, b in want]), "glam")):
        same(got, want_p, what)
        check_nobody(w, got, fused, what)
    glev, off, flat = [gt.cpu().numpy()], 0, gm.cpu().numpy()
    for l in levels[1:]:
        glev.append(flat[off:off + l.size])
        off += l.size
    for l in range(L):
        ref, mag = np.stack([a.level(a.g, l) for a in accs]), np.stack([a.level(a.gabs, l) for a in accs])
        cnt = np.stack([a.level(a.count, l) for a in accs])[..., None]
        if cnt.any():
            check_sum(glev[l], ref, mag, cnt, f"cube gtex level {l}")
        else:
            assert (glev[l] == 0).all()
    assert all(any(a.level(a.count, l).any() for a in accs) for l in (0, 1, L - 1))
    if not fused:
        teeth_cube_mip_grad(tmp, w, accs)


def run_cube_level(tmp, w, fused):
    fs = w.fs
    (dw, dirs, ddw, dird), levels = dirs_of(w), cube_of(w)[0]
    N, L = levels[0].shape[-2], len(levels)
    out = filled(w.shape(1))
    fs.cube_level(w.vis.data_ptr(), dirs.data_ptr(), dird.data_ptr(), N, L, out.data_ptr(), fs.interpolate_bytes(1), fl(fused), stream())
    torch.cuda.synchronize()
    want = np.stack([cubemipref.level(tmp, N, L, w.n_tris[i], w.v[i, 1], dw[i], ddw[i], fused, SENTINEL)[None] for i in range(w.n)])
    got = words(out)
    same(got, want, "cube_level")
    check_nobody(w, got, fused, "cube_level")


# ------------------------------------------------------------------------------------------------------ perspective
def run_perspective(tmp, w, fused):
    fs = w.fs
    q, qd = w.memo("q", make_q)
    out = filled(fs.out_shape)
    fs.perspective(w.vis.data_ptr(), qd.data_ptr(), w.n, w.T, out.data_ptr(), fs.out_bytes, fl(fused), stream())
    torch.cuda.synchronize()
    expect = lambda i, j: perspref.forward(tmp, q[j], w.n_tris[i], w.v[i])  # noqa: E731
    same(words(out), np.stack([expect(i, i) for i in range(w.n)]), "perspective")  # (every word is written, nobody's too)
    reads_its_own(w, expect, "perspective")


def ref_persp_grad(tmp, w, fused):
    (q, _), (gout, _) = w.memo("q", make_q), w.gout
    accs = [perspref.Grad(q.shape[1:]) for _ in range(w.n)]
    return accs, [perspref.grad(tmp, q[i], w.n_tris[i], w.v[i], gout[i, :2], accs[i], True, fused, pre(w, 2)) for i in range(w.n)]


def teeth_persp_grad(tmp, w, accs):
    (q, _), (gout, _) = w.memo("q", make_q), w.gout

    def tile(f, rs, cs):
        a = perspref.Grad(q.shape[1:])
        perspref.grad(tmp, q[f], w.n_tris[f], w.v[f][:, rs, cs], gout[f, :2][:, rs, cs], a, False)
        return a.gabs
    mag, cnt = summed(accs, True, count=lambda a: a.count[:, None])
    teeth(tile_shares(w, mag.shape, True, tile), mag, cnt, "gq", require=w.name == "many")  # (large: huge triangles, printed only)


def run_perspective_grad(tmp, w, fused):
    fs = w.fs
    (_, qd), (_, g) = w.memo("q", make_q), w.gout
    gbp = g[:, :2].contiguous()
    gq, gb = torch.zeros_like(qd), filled(w.shape(2))
    fs.perspective_grad(w.vis.data_ptr(), qd.data_ptr(), w.n, w.T, gbp.data_ptr(), gb.data_ptr(), gq.data_ptr(), fl(fused), stream())
    torch.cuda.synchronize()
    accs, want = ref_persp_grad(tmp, w, fused)
    got = words(gb)
    same(got, np.stack(want), "persp gbary")
    check_nobody(w, got, fused, "persp gbary")
    mag, cnt = np.stack([a.gabs for a in accs]), np.stack([a.count for a in accs])[:, :, None]
    check_sum(gq.cpu().numpy(), np.stack([a.gq for a in accs]), mag, cnt, "gq")
    if not fused:
        teeth_persp_grad(tmp, w, accs)


def run_interpolate_deriv_persp(tmp, w, fused):
    fs, C = w.fs, w.C
    (q, qd), a = w.memo("q", make_q), dev(w.attr)
    out = filled(w.shape(2 * C))
    fs.interpolate_deriv_persp(w.vis.data_ptr(), qd.data_ptr(), w.n, w.T, a.data_ptr(), C, w.n, w.T, out.data_ptr(), fs.interpolate_bytes(2 * C),
                               fl(fused), stream())
    torch.cuda.synchronize()
    got = words(out)
    same(got, np.stack([perspref.deriv(tmp, q[i], w.pos[i], w.attr[i], w.n_tris[i], w.v[i], fused, pre(w, 2 * C)) for i in range(w.n)]), "deriv persp")
    check_nobody(w, got, fused, "deriv persp")


# ------------------------------------------------------------------------------------------------------ shadow
def run_shadow(tmp, w, fused):
    fs = w.fs
    depth, d, scw, sc = w.memo("shadow", make_shadow)
    out = filled(w.shape(1))
    fs.shadow(w.vis.data_ptr(), sc.data_ptr(), d.data_ptr(), depth.shape[-1], depth.shape[-2], w.n if per_frame(w) else 1, BIAS, WIDTH,
              out.data_ptr(), fs.interpolate_bytes(1), fl(fused), stream())
    torch.cuda.synchronize()
    expect = lambda i, j: shadowref.forward(tmp, of(depth, j, per_frame(w)), w.n_tris[i], w.v[i, 1], scw[i], BIAS, WIDTH, fused, pre(w, 1))  # noqa: E731
    got = words(out)
    same(got, np.stack([expect(i, i) for i in range(w.n)]), "shadow")
    check_nobody(w, got, fused, "shadow")
    if per_frame(w) and not fused:
        reads_its_own(w, expect, "shadow")


def ref_shadow_grad(tmp, w, fused):
    (depth, _, scw, _), (gout, _), per = w.memo("shadow", make_shadow), w.gout, per_frame(w)
    accs = [shadowref.Grad(depth.shape[-2:]) for _ in range(w.n if per else 1)]
    return accs, [shadowref.grad(tmp, of(depth, i, per), w.n_tris[i], w.v[i, 1], scw[i], gout[i, :1], BIAS, WIDTH, accs[i if per else 0], True, fused,
                                 pre(w, 3)) for i in range(w.n)]


def teeth_shadow_grad(tmp, w, accs):
    (depth, _, scw, _), (gout, _), per = w.memo("shadow", make_shadow), w.gout, per_frame(w)

    def tile(f, rs, cs):
        a = shadowref.Grad(depth.shape[-2:])
        shadowref.grad(tmp, of(depth, f, per), w.n_tris[f], w.v[f, 1][rs, cs], scw[f][:, rs, cs], gout[f, :1][:, rs, cs], BIAS, WIDTH, a, False)
        return a.gabs
    mag, cnt = summed(accs, per, count=lambda a: a.count)
    teeth(tile_shares(w, mag.shape, per, tile), mag, cnt, "gmap")


def run_shadow_grad(tmp, w, fused):
    fs = w.fs
    (depth, d, _, sc), (_, g) = w.memo("shadow", make_shadow), w.gout
    per = per_frame(w)
    g1 = g[:, :1].contiguous()
    res = []
    for want_map in (True, False):
        gm, gs = (torch.zeros_like(d) if want_map else None), filled(w.shape(3))
        fs.shadow_grad(w.vis.data_ptr(), sc.data_ptr(), g1.data_ptr(), d.data_ptr(), depth.shape[-1], depth.shape[-2], w.n if per else 1, BIAS,
                       WIDTH, ptr(gm), gs.data_ptr(), fl(fused), stream())
        torch.cuda.synchronize()
        res.append((gm, words(gs)))
    accs, want = ref_shadow_grad(tmp, w, fused)
    got = res[0][1]
    same(got, np.stack(want), "gsc")
    check_nobody(w, got, fused, "gsc")
    assert np.array_equal(res[1][1], got), "gsc without d_gmap"
    mag, cnt = np.stack([a.gabs for a in accs]), np.stack([a.count for a in accs])
    check_sum(res[0][0].cpu().numpy(), np.stack([a.gmap for a in accs]), mag, cnt, "gmap")
    if not fused:
        teeth_shadow_grad(tmp, w, accs)


# ------------------------------------------------------------------------------------------------------ normal mapping
def run_normal_map(tmp, w, fused):
    fs = w.fs
    (nw, nrm, _, _), (tw, tan, mw, m) = shading_of(w), w.memo("tangent", make_tangent)
    out = filled(w.shape(3))
    fs.normal_map(w.vis.data_ptr(), nrm.data_ptr(), tan.data_ptr(), m.data_ptr(), out.data_ptr(), fs.interpolate_bytes(3), fl(fused), stream())
    torch.cuda.synchronize()
    got = words(out)
    same(got, np.stack([tangentref.nm_forward(tmp, w.n_tris[i], w.v[i, 1], nw[i], tw[i], mw[i], fused, SENTINEL) for i in range(w.n)]), "normal_map")
    check_nobody(w, got, fused, "normal_map")


def run_normal_map_grad(tmp, w, fused):
    fs = w.fs
    (nw, nrm, _, _), (tw, tan, mw, m), (gout, g) = shading_of(w), w.memo("tangent", make_tangent), gout_of(w, 3)
    outs = [filled(w.shape(k)) for k in (3, 4, 3)]
    fs.normal_map_grad(w.vis.data_ptr(), nrm.data_ptr(), tan.data_ptr(), m.data_ptr(), g.data_ptr(), *(o.data_ptr() for o in outs), fl(fused), stream())
    torch.cuda.synchronize()
    want = [tangentref.nm_grad(tmp, w.n_tris[i], w.v[i, 1], nw[i], tw[i], mw[i], gout[i], fused, SENTINEL) for i in range(w.n)]
    for k, what in enumerate(("nm gnrm", "nm gtan", "nm gm")):
        got = words(outs[k])
        same(got, np.stack([x[k] for x in want]), what)
        check_nobody(w, got, fused, what)


# ------------------------------------------------------------------------------------------------------ light and microfacet
class Lit:
    """light or microfacet: the planes each reads, its calls and its reference's"""

    def __init__(self, name):
        self.name, self.ref = name, lightref if name == "light" else microfacetref
        self.K = self.ref.par_len(N_LIGHTS)

    def inputs(self, w):
        """([float32 arrays or None], [their copies on the device]): nrm, pos, kd — or nrm, pos, base, mat"""
        nw, nrm, pw, pos = shading_of(w)
        cw, col = w.memo("colour", make_colour)
        extra = () if self.name == "light" else (w.memo("mat", make_mat),)
        return [nw, pw, cw] + [e[0] for e in extra], [nrm, pos, col] + [e[1] for e in extra]

    def out_planes(self, ins):
        """the plane count of every gradient plane output, None where the input is null"""
        return [3, 3, 3 if ins[2] is not None else None] + ([2] if self.name == "microfacet" else [])

    def work_bytes(self, fs):
        return fs.light_work_bytes(N_LIGHTS) if self.name == "light" else fs.microfacet_work_bytes(N_LIGHTS)

    def forward(self, fs, vis, ins, par, shape, flags):
        out, pt = filled(shape), dev(par)
        tail = (P,) if self.name == "light" else ()
        getattr(fs, self.name)(vis.data_ptr(), *(ptr(t) for t in ins), pt.data_ptr(), N_LIGHTS, len(par), *tail, out.data_ptr(),
                               int(np.prod(shape)) * 4, flags, stream())
        torch.cuda.synchronize()
        return words(out)

    def backward(self, fs, vis, ins, par, g, shape, flags, want_par=True):
        """→ (the gradient planes' words, each from the sentinel; gpar's words [par_frames, K] from the sentinel, or None)"""
        n_pl = self.out_planes(ins)
        outs = [None if k is None else filled((shape[0], k) + tuple(shape[2:])) for k in n_pl]
        pt = dev(par)
        gpar = filled((len(par), self.K)) if want_par else None
        nbytes = self.work_bytes(fs) if want_par else 0
        work = filled((nbytes // 4,)) if want_par else None
        assert not want_par or nbytes > 0
        tail = (P,) if self.name == "light" else ()
        getattr(fs, self.name + "_grad")(vis.data_ptr(), *(ptr(t) for t in ins), pt.data_ptr(), N_LIGHTS, len(par), *tail, g.data_ptr(),
                                         *(ptr(o) for o in outs), ptr(gpar), ptr(work), nbytes, flags, stream())
        torch.cuda.synchronize()
        return [None if o is None else words(o) for o in outs], (None if gpar is None else words(gpar))

    def ref_forward(self, tmp, n_tris, ids, ins, par, fused, prefill):
        tail = (P,) if self.name == "light" else ()
        return self.ref.forward(tmp, n_tris, ids, *ins, par, *tail, fused, prefill)

    def ref_grad(self, tmp, n_tris, ids, ins, par, gout, into, fused=True, prefill=None):
        tail = (P,) if self.name == "light" else ()
        return self.ref.grad(tmp, n_tris, ids, *ins, par, *tail, gout, into, fused, prefill)


def frame_ins(ins, i, rs=slice(None), cs=slice(None)):
    return [None if a is None else a[i][:, rs, cs] for a in ins]


def run_lit(kind, tmp, w, fused):
    lit = Lit(kind)
    ins_w, ins = lit.inputs(w)
    for par in ((make_params(w, lit.ref),) if w.name == "large" else (make_params(w, lit.ref), lit.ref.make_params(23, N_LIGHTS)[None])):
        got = lit.forward(w.fs, w.vis, ins, par, w.shape(3), fl(fused))
        expect = lambda i, j: lit.ref_forward(tmp, w.n_tris[i], w.v[i, 1], frame_ins(ins_w, i), par[j % len(par)], fused, pre(w, 3))  # noqa: E731
        same(got, np.stack([expect(i, i) for i in range(w.n)]), f"{kind} ({len(par)} parameter frames)")
        check_nobody(w, got, fused, kind)
        if len(par) > 1 and not fused:
            reads_its_own(w, expect, kind)


def ref_lit_grad(lit, tmp, w, fused):
    (ins_w, _), (gout, _), par = lit.inputs(w), gout_of(w, 3), make_params(w, lit.ref)
    accs = [lit.ref.Grad(N_LIGHTS) for _ in range(w.n)]
    return accs, [lit.ref_grad(tmp, w.n_tris[i], w.v[i, 1], frame_ins(ins_w, i), par[i], gout[i], accs[i], fused, pre(w, 3)) for i in range(w.n)]


def teeth_lit_grad(lit, tmp, w, accs):
    """(the rows are also held bit for bit; no entry has a single term)"""
    (ins_w, _), (gout, _), par = lit.inputs(w), gout_of(w, 3), make_params(w, lit.ref)

    def tile(f, rs, cs):
        a = lit.ref.Grad(N_LIGHTS)
        lit.ref_grad(tmp, w.n_tris[f], w.v[f, 1][rs, cs], frame_ins(ins_w, f, rs, cs), par[f], gout[f][:, rs, cs], a)
        return a.gabs
    mag, cnt = summed(accs, True, count=lambda a: a.count)
    teeth(tile_shares(w, mag.shape, True, tile), mag, cnt, f"{lit.name} gpar", single=False)


def run_lit_grad(kind, tmp, w, fused):
    lit = Lit(kind)
    fs, flags = w.fs, fl(fused)
    (ins_w, ins), (gout, g), par = lit.inputs(w), gout_of(w, 3), make_params(w, lit.ref)
    planes, rows = lit.backward(fs, w.vis, ins, par, g, w.shape(3), flags)
    accs, want = ref_lit_grad(lit, tmp, w, fused)
    for k, got in enumerate(planes):
        assert (got is None) == (want[0][k] is None), (kind, k)
        if got is not None:
            same(got, np.stack([x[k] for x in want]), f"{kind}_grad plane output {k}")
            check_nobody(w, got, fused, f"{kind}_grad plane output {k}")
    alone, none = lit.backward(fs, w.vis, ins, par, g, w.shape(3), flags, want_par=False)
    assert none is None and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(alone, planes)), f"{kind}_grad without d_gpar"
    if fused:
        return
    # (a) every entry is written; (b) the per-frame rows against the reference's double sums
    assert (rows != SENTINEL).all(), f"{kind} gpar: {int((rows == SENTINEL).sum())} entries were not written"
    check_gpar(rows.view(np.float32), accs, f"{kind} gpar, {w.name}")
    # (e) a second launch gives the same words
    assert np.array_equal(lit.backward(fs, w.vis, ins, par, g, w.shape(3), flags)[1], rows), f"{kind} gpar: a second launch differs"
    # (c) the rows do not depend on the grid: the same frames in sets below the cap give the same words
    if w.name == "many":
        others = w.rng(24).choice(np.setdiff1d(np.arange(w.n), SMALL_SET), 9, replace=False)
        small_sets = [np.concatenate([SMALL_SET, np.sort(others)])]
    else:
        small_sets = [np.array([0]), np.array([w.n - 1])]
    for idx in small_sets:
        small = w.ctx.frameset([w.frames[i] for i in idx])
        vis = visibility(small)
        assert np.array_equal(words(vis), w.v[idx]), "the small set's visibility buffer is not the big set's slice"
        sub = [None if a is None else dev(a[idx]) for a in ins_w]
        shape = (len(idx),) + tuple(w.shape(3)[1:])
        assert tuple(small.interpolate_shape(3)) == shape and lit.work_bytes(small) < lit.work_bytes(fs)
        small_rows = lit.backward(small, vis, sub, par[idx], dev(gout[idx]), shape, flags)[1]
        small.close()
        assert np.array_equal(small_rows, rows[idx]), f"{kind} gpar: the rows of frames {idx.tolist()} depend on the grid"
    # (d) one shared parameter frame: 0 + row 0 + row 1 + ... in float32 of the rows the same frame repeated gives
    if w.name == "many":
        one = lit.ref.make_params(23, N_LIGHTS)[None]
        total = lit.backward(fs, w.vis, ins, one, g, w.shape(3), flags)[1]
        rep = lit.backward(fs, w.vis, ins, np.repeat(one, w.n, 0), g, w.shape(3), flags)[1].view(np.float32)
        s = np.zeros(lit.K, np.float32)
        for i in range(w.n):
            s = s + rep[i]
        assert total.shape == (1, lit.K) and np.array_equal(total[0], s.view(np.uint32)) and (s != 0).all(), f"{kind} gpar: shared parameters"
        teeth_lit_grad(lit, tmp, w, accs)


# ------------------------------------------------------------------------------------------------------ reflect and ibl
def make_eye(w):
    return iblref.make_eye(25, w.n) if w.name == "many" else iblref.make_eye(25)[None]


def run_reflect(tmp, w, fused):
    fs = w.fs
    (nw, nrm, pw, pos), eye = shading_of(w), make_eye(w)
    e, out = dev(eye), filled(w.shape(4))
    fs.reflect(w.vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), e.data_ptr(), len(eye), out.data_ptr(), fs.interpolate_bytes(4), fl(fused), stream())
    torch.cuda.synchronize()
    expect = lambda i, j: iblref.reflect(tmp, w.n_tris[i], w.v[i, 1], nw[i], pw[i], eye[j % len(eye)], fused, pre(w, 4))  # noqa: E731
    got = words(out)
    same(got, np.stack([expect(i, i) for i in range(w.n)]), "reflect")
    check_nobody(w, got, fused, "reflect")
    if len(eye) > 1 and not fused:
        reads_its_own(w, expect, "reflect")


def run_reflect_grad(tmp, w, fused):
    fs = w.fs
    (nw, nrm, pw, pos), eye, (gout, g) = shading_of(w), make_eye(w), gout_of(w, 4)
    e, outs = dev(eye), [filled(w.shape(3)), filled(w.shape(3))]
    fs.reflect_grad(w.vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), e.data_ptr(), len(eye), g.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                    fl(fused), stream())
    torch.cuda.synchronize()
    expect = lambda i, j: np.stack(iblref.reflect_grad(tmp, w.n_tris[i], w.v[i, 1], nw[i], pw[i], eye[j % len(eye)], gout[i], fused, pre(w, 3)))  # noqa: E731
    want = np.stack([expect(i, i) for i in range(w.n)])
    for k, what in enumerate(("reflect gnrm", "reflect gpos")):
        got = words(outs[k])
        same(got, want[:, k], what)
        check_nobody(w, got, fused, what)
    if len(eye) > 1 and not fused:
        reads_its_own(w, expect, "reflect_grad")


def run_ibl(tmp, w, fused):
    fs = w.fs
    (tab, *planes), (tt, *devs) = w.memo("ibl", make_ibl)
    out = filled(w.shape(3))
    fs.ibl(w.vis.data_ptr(), *(ptr(t) for t in devs), tt.data_ptr(), len(tab), out.data_ptr(), fs.interpolate_bytes(3), fl(fused), stream())
    torch.cuda.synchronize()
    got = words(out)
    same(got, np.stack([iblref.ibl(tmp, w.n_tris[i], w.v[i, 1], *frame_ins(planes, i), tab, fused, pre(w, 3)) for i in range(w.n)]), "ibl")
    check_nobody(w, got, fused, "ibl")


def ref_ibl_grad(tmp, w, fused):
    ((tab, *planes), _), (gout, _) = w.memo("ibl", make_ibl), gout_of(w, 3)
    acc = iblref.TabGrad(len(tab))
    return acc, [iblref.ibl_grad(tmp, w.n_tris[i], w.v[i, 1], *frame_ins(planes, i), tab, gout[i], acc, fused, pre(w, 3)) for i in range(w.n)]


def teeth_ibl_grad(tmp, w, acc):
    ((tab, *planes), _), (gout, _) = w.memo("ibl", make_ibl), gout_of(w, 3)

    def tile(f, rs, cs):
        a = iblref.TabGrad(len(tab))
        iblref.ibl_grad(tmp, w.n_tris[f], w.v[f, 1][rs, cs], *frame_ins(planes, f, rs, cs), tab, gout[f][:, rs, cs], a)
        return a.gabs
    teeth(tile_shares(w, acc.gabs.shape, False, tile), acc.gabs, acc.count, "gtab")


def run_ibl_grad(tmp, w, fused):
    fs = w.fs
    ((tab, *planes), (tt, *devs)), (_, g) = w.memo("ibl", make_ibl), gout_of(w, 3)
    n_pl = [3 if planes[0] is not None else None, 2, 1, 3, 3]
    res = []
    for want_tab in (True, False):
        outs = [None if k is None else filled(w.shape(k)) for k in n_pl]
        gtab = torch.zeros_like(tt) if want_tab else None
        fs.ibl_grad(w.vis.data_ptr(), *(ptr(t) for t in devs), tt.data_ptr(), len(tab), g.data_ptr(), *(ptr(o) for o in outs), ptr(gtab), fl(fused),
                    stream())
        torch.cuda.synchronize()
        res.append(([None if o is None else words(o) for o in outs], gtab))
    acc, want = ref_ibl_grad(tmp, w, fused)
    for k, what in enumerate(("ibl gbase", "ibl gmat", "ibl gnv", "ibl girr", "ibl gspec")):
        got = res[0][0][k]
        assert (got is None) == (want[0][k] is None), what
        if got is not None:
            same(got, np.stack([x[k] for x in want]), what)
            check_nobody(w, got, fused, what)
            assert np.array_equal(res[1][0][k], got), what + " without d_gtab"
    check_gtab(res[0][1].cpu().numpy(), acc, f"gtab, {w.name}")
    if not fused:
        teeth_ibl_grad(tmp, w, acc)


def lit_run(run, kind):
    return lambda tmp, w, fused: run(kind, tmp, w, fused)


# entry → (its run, whether it has SRZ_FUSED_CLEAR's two behaviours)
PASSES = {"texture_cube": (run_texture_cube, True), "texture_cube_grad": (run_texture_cube_grad, True),
          "texture_cube_mip": (run_texture_cube_mip, True), "texture_cube_mip_grad": (run_texture_cube_mip_grad, True),
          "cube_level": (run_cube_level, True), "perspective": (run_perspective, False), "perspective_grad": (run_perspective_grad, True),
          "interpolate_deriv_persp": (run_interpolate_deriv_persp, True), "shadow": (run_shadow, True), "shadow_grad": (run_shadow_grad, True),
          "light": (lit_run(run_lit, "light"), True), "light_grad": (lit_run(run_lit_grad, "light"), True),
          "normal_map": (run_normal_map, True), "normal_map_grad": (run_normal_map_grad, True),
          "microfacet": (lit_run(run_lit, "microfacet"), True), "microfacet_grad": (lit_run(run_lit_grad, "microfacet"), True),
          "reflect": (run_reflect, True), "reflect_grad": (run_reflect_grad, True), "ibl": (run_ibl, True), "ibl_grad": (run_ibl_grad, True)}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", list(PASSES))
def test_more_tiles_than_workgroups(worlds, tmp_path, name, shape):
    """(many: with and without the fused clear; large: without it, the stricter of the two — nobody's words must survive)"""
    run, has_fused = PASSES[name]
    w = worlds(shape)
    for fused in ((False, True) if has_fused and shape == "many" else (False,)):
        run(tmp_path, w, fused)
