"""-m gpu: k_background and k_background_grad<false / true> beyond tile_grid's cap, on tests/walkkit.py's `many` (6,144 frames of four
tiles) and `large` (seven frames of 2,401) sets: a workgroup's second trip round the walk, with what it carries — the table of
distinct texels handed from one tile to the next, the tile's row of partial sums named by the tile's index.  It follows
tests/test_gpu_pass_walk_lit.py: per-frame cubes and blocks on `many`, one 64 x 64 cube on `large`, so that a lost or doubled tile
moves an element of gtex by more than its bound (walkkit.teeth, asserted from the reference alone, before the sums are checked); gray
bit for bit against the reference's fixed tree, against the rows the same frames give in a set below the cap, against the frame-order
sum for a shared block, and against a second launch."""
import numpy as np
import pytest
import torch

import backgroundref as br
import cuberef
import walkkit
from support import SENTINEL, ctx, filled, stream, visibility, words  # noqa: F401
from walkkit import F, SHAPES, Shares, check_sum, dev, pre, same, teeth

pytestmark = pytest.mark.gpu

CUBE_N = {"many": 4, "large": 64}
SMALL_SET = (0, 7, 8, 4095, 4096, 4103, 6143)  # many: with 16,384 workgroups the frames from 4,096 on are reached on a later trip


@pytest.fixture(scope="module")
def worlds(ctx):
    yield from walkkit.make_worlds(ctx)


def per_frame(w):
    return w.name == "many"


def of(a, i, per):
    return a[i] if per else a


def aligned_block(kx, ky):
    """large: a block under which the +Z face of the 64 x 64 cube has one texel per 32 x 32 TILE, texel centres on the tiles' corners:
    the ray of pixel (x, y) is (x / 1024 + (7.5 + kx) / 32 - 1, -(y / 1024 + (7.5 + ky) / 32 - 1), 1), all dyadic, so fx = x / 32 + 7 +
    kx exactly and the 1,568 pixels stay inside the face (fx < 59).  An element of gtex — a texel's tent, two texels wide — then
    gathers the pixels of exactly 2 x 2 tiles, about a quarter from each: with at most 4,096 adds, gamma_n = 2.4e-4 is far below a
    quarter of any tile's share unless the owners leave that tile a handful of pixels — the condition walkkit.teeth asserts.  A
    frame far larger than the cube cannot have few adds per element; it can have every tile matter.  kx, ky: whole texels, so that
    the frames' blocks differ"""
    ox, oy = (7.5 + kx) / 32 - 1, (7.5 + ky) / 32 - 1
    return np.float32([ox, -oy, 1, 1 / 1024, 0, 0, 0, -1 / 1024, 0])


def make_inputs(w):
    """(cube, its copy on the device, the per-frame blocks [n, 9], gout [n, C, rows, W] with NaN at the owned pixels, its copy)"""
    cube = cuberef.make_cube(31, CUBE_N[w.name], w.C, frames=w.n if per_frame(w) else None)
    h, wd = w.v.shape[2:]
    if per_frame(w):
        rays = np.stack([br.camera_block(wd, h, i, 1.6) for i in range(w.n)])
    else:
        rays = np.stack([aligned_block(i % 3, i // 3) for i in range(w.n)])
    g = w.rng(32).normal(0, 2, w.shape(w.C)).astype(np.float32)
    g[np.broadcast_to(w.own[:, None], g.shape)] = np.nan  # the words at the owned pixels are never read
    return cube, dev(cube), rays, g, dev(g)


def inputs_of(w):
    return w.memo("background", make_inputs)


def forward(fs, vis, t, rays, N, C, tf, fused):
    r = dev(rays)
    out = filled(fs.interpolate_shape(C))
    fs.background(vis.data_ptr(), r.data_ptr(), len(rays), t.data_ptr(), N, C, tf, br.NOBODY, out.data_ptr(), fs.interpolate_bytes(C),
                  F if fused else 0, stream())
    torch.cuda.synchronize()
    return words(out)


def backward(fs, vis, t, rays, g, N, C, tf, want_tex=True, want_ray=True):
    r = dev(rays)
    gt = torch.zeros_like(t) if want_tex else None
    gr = filled((len(rays), 9)) if want_ray else None
    wb = fs.background_work_bytes() if want_ray else 0
    work = filled((wb // 4 + 1,)) if want_ray else None
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    fs.background_grad(vis.data_ptr(), r.data_ptr(), len(rays), g.data_ptr(), t.data_ptr(), N, C, tf, br.NOBODY, p(gt), p(gr), p(work), wb, F,
                       stream())
    torch.cuda.synchronize()
    return (gt.cpu().numpy() if want_tex else None), (words(gr) if want_ray else None)


def reference(tmp, w):
    """(one Grad per cube, the frames' rows [n, 9] float32), made once per world"""
    def make(w):
        cube, _, rays, g, _ = inputs_of(w)
        per = per_frame(w)
        accs = [br.Grad(cube.shape[-4:]) for _ in range(w.n if per else 1)]
        rows = [br.grad(tmp, of(cube, i, per), w.n_tris[i], w.v[i, 1], rays[i], g[i], accs[i if per else 0])[0] for i in range(w.n)]
        return accs, np.stack(rows)
    return w.memo("background ref", make)


@pytest.mark.parametrize("shape", SHAPES)
def test_background_forward_beyond_the_cap(worlds, tmp_path, shape):
    """(many: with and without the fused clear; large: without it, the stricter of the two — the owned words must survive)"""
    w = worlds(shape)
    cube, t, rays, _, _ = inputs_of(w)
    per, N, C = per_frame(w), CUBE_N[shape], w.C
    for fused in ((False, True) if shape == "many" else (False,)):
        got = forward(w.fs, w.vis, t, rays, N, C, w.n if per else 1, fused)
        expect = lambda i, j: br.forward(tmp_path, of(cube, j, per), w.n_tris[i], w.v[i, 1], rays[j], br.NOBODY, fused, pre(w, C))  # noqa: E731
        same(got, np.stack([expect(i, i) for i in range(w.n)]), "background")
        owned = np.broadcast_to(w.own[:, None], got.shape)
        assert (got[owned] == (0 if fused else SENTINEL)).all() and (got[~owned] != SENTINEL).all()
        if not fused:  # every frame reads its own block (and cube): its neighbour's gives other words
            some = range(0, w.n, max(1, w.n // 64))
            assert np.mean([expect(i, i).tobytes() != expect(i, (i + 1) % w.n).tobytes() for i in some]) >= 0.9


@pytest.mark.parametrize("shape", SHAPES)
def test_background_grad_beyond_the_cap(worlds, tmp_path, shape):
    w = worlds(shape)
    cube, t, rays, gout, g = inputs_of(w)
    per, N, C = per_frame(w), CUBE_N[shape], w.C
    tf = w.n if per else 1
    accs, rows = reference(tmp_path, w)
    # ---- teeth, from the reference alone: the smallest share one tile has in an element of gtex against the element's bound
    mag, cnt = np.stack([a.gabs for a in accs]), np.stack([a.count for a in accs])[..., None]
    shares = Shares(mag.shape)
    for _, f, rs, cs in w.tiles():
        a = br.Grad(cube.shape[-4:])
        br.grad_box(tmp_path, of(cube, f, per), w.n_tris[f], w.v[f, 1], rays[f], gout[f], a, rs, cs)
        shares.add(a.gabs, f if per else 0)
    teeth(shares, mag, cnt, f"background gtex, {shape}", single=per)  # (large: one cube for 17 million pixels has no element of one add)
    # ---- both builds
    gt, gr = backward(w.fs, w.vis, t, rays, g, N, C, tf)
    check_sum(gt, np.stack([a.gtex for a in accs]).reshape(gt.shape), mag.reshape(gt.shape), np.broadcast_to(cnt, mag.shape).reshape(gt.shape),
              f"background gtex, {shape}")
    alone = backward(w.fs, w.vis, t, rays, g, N, C, tf, want_ray=False)[0]
    check_sum(alone, np.stack([a.gtex for a in accs]).reshape(gt.shape), mag.reshape(gt.shape),
              np.broadcast_to(cnt, mag.shape).reshape(gt.shape), f"background gtex alone, {shape}")
    # ---- gray: every row written, bit for bit the reference's tree; a second launch and the other build give the same words
    assert (gr != SENTINEL).all()
    same(gr, rows, f"background gray, {shape}")
    assert (rows != 0).all(1).mean() >= 0.9
    assert np.array_equal(backward(w.fs, w.vis, t, rays, g, N, C, tf)[1], gr), "a second launch differs"
    assert np.array_equal(backward(w.fs, w.vis, t, rays, g, N, C, tf, want_tex=False)[1], gr), "gray depends on d_gtex"
    # ---- the rows do not depend on the grid: the same frames in sets below the cap give the same words
    if shape == "many":
        others = w.rng(24).choice(np.setdiff1d(np.arange(w.n), SMALL_SET), 9, replace=False)
        small_sets = [np.concatenate([SMALL_SET, np.sort(others)])]
    else:
        small_sets = [np.array([0]), np.array([w.n - 1])]
    for idx in small_sets:
        small = w.ctx.frameset([w.frames[i] for i in idx])
        vis = visibility(small)
        assert np.array_equal(words(vis), w.v[idx]), "the small set's visibility buffer is not the big set's slice"
        assert small.background_work_bytes() < w.fs.background_work_bytes()
        ts = dev(cube[idx]) if per else t
        small_rows = backward(small, vis, ts, rays[idx], dev(gout[idx]), N, C, len(idx) if per else 1, want_tex=False)[1]
        small.close()
        assert np.array_equal(small_rows, gr[idx]), f"the rows of frames {idx.tolist()} depend on the grid"
    # ---- one shared block: 0 + row 0 + row 1 + ... in float32 of the rows the same block repeated gives
    one = rays[:1]
    total = backward(w.fs, w.vis, t, one, g, N, C, tf, want_tex=False)[1]
    rep = backward(w.fs, w.vis, t, np.repeat(one, w.n, 0), g, N, C, tf, want_tex=False)[1].view(np.float32)
    s = np.zeros(9, np.float32)
    for i in range(w.n):
        s = s + rep[i]
    assert total.shape == (1, 9) and np.array_equal(total[0], s.view(np.uint32)) and (s != 0).all(), "a shared block"
    assert np.array_equal(s, br.fold(tmp_path, rep))
