"""-m gpu: the SH9 pixel pass beyond the grid's cap — tests/walkkit.py's two sets (`many`, 6,144 frames of four tiles, 24,576 tiles;
`large`, 7 frames of 49 x 49 tiles, 16,807 tiles; tile_grid launches at most 16,384 workgroups) under srz_frameset_sh and
srz_frameset_sh_grad: k_sh, k_sh_grad<true> (the LDS partials a workgroup reuses from tile to tile, the work buffer's rows, k_light_fold
over tiles and frames) and k_sh_grad<false>.  What a workgroup computes from a frame index in the thousands is f * sh_stride and the
plane offsets.  The visibility buffer is the GPU's own render_visibility, the normals the GPU's own interpolate of seeded
attributes, gout seeded, NaN at nobody's pixels.  The expected values are tests/shref.py's on the device's words: the planes bit
for bit; gsh within the reference's Grad.bound — and, being reduced in a fixed tree, bit for bit the rows the same frames give in
a set below the cap, the frame-order float32 sum for shared coefficients, and a second launch.  gamma_n grows with n, so that the
bound can see a tile is asserted from the reference alone (walkkit.teeth) on `many`, whose rows sum a frame's four tiles.  Every
output starts from the sentinel; `many` also runs with SRZ_FUSED_CLEAR."""
import numpy as np
import pytest
import torch

import shref
import walkkit
from support import SENTINEL, ctx, filled, stream, visibility, words  # noqa: F401
from walkkit import F, SHAPES, Shares, check_bound, check_nobody, dev, pre, same, teeth

pytestmark = pytest.mark.gpu

N_CH = {"many": 7, "large": 3}
KIND = {"many": shref.RADIANCE, "large": shref.IRRADIANCE}
SMALL_SET = (0, 7, 8, 4095, 4096, 4103, 6143)  # many: with 16,384 workgroups the frames from 4,096 on are reached on a later trip


@pytest.fixture(scope="module")
def worlds(ctx):
    yield from walkkit.make_worlds(ctx)


def ptr(t):
    return None if t is None else t.data_ptr()


def make_normals(w):
    """shading normals of any length and direction through the GPU's interpolate → (nrm, its copy on the device)"""
    rng = w.rng(31)
    a = rng.normal(0, 1.0, (w.n, w.T, 3, 3)) * rng.uniform(0.5, 3.0, (w.n, w.T, 3, 1))
    return w.interpolated(a.astype(np.float32))


def inputs(w):
    C = N_CH[w.name]
    return (C, w.memo("sh normals", make_normals), w.memo(("sh gout", C), lambda w: w.seeded(32, C, 2.0)), shref.make_sh(33, C, frames=w.n))


def forward(fs, vis, nrm, sh, kind, shape, flags):
    out, st = filled(shape), dev(sh)
    fs.sh(vis.data_ptr(), nrm.data_ptr(), st.data_ptr(), sh.shape[-1], len(sh), kind, out.data_ptr(), int(np.prod(shape)) * 4, flags, stream())
    torch.cuda.synchronize()
    return words(out)


def backward(fs, vis, nrm, sh, kind, g, n_frames, flags, want_sh=True, want_nrm=True):
    """→ (gnrm's words from the sentinel or None, gsh's words [sh_frames, 9, C] from the sentinel or None)"""
    C = sh.shape[-1]
    gn = filled((n_frames, 3) + tuple(nrm.shape[2:])) if want_nrm else None
    st = dev(sh)
    gsh = filled((len(sh), 9, C)) if want_sh else None
    nbytes = fs.sh_work_bytes(C) if want_sh else 0
    work = filled((nbytes // 4,)) if want_sh else None
    assert not want_sh or nbytes > 0
    fs.sh_grad(vis.data_ptr(), nrm.data_ptr(), st.data_ptr(), C, len(sh), kind, g.data_ptr(), ptr(gn), ptr(gsh), ptr(work), nbytes, flags, stream())
    torch.cuda.synchronize()
    return (None if gn is None else words(gn)), (None if gsh is None else words(gsh))


def run_sh(tmp, w, fused):
    C, (nw, nrm), _, per = inputs(w)
    kind, flags = KIND[w.name], F if fused else 0
    for sh in ((per,) if w.name == "large" else (per, shref.make_sh(34, C)[None])):
        got = forward(w.fs, w.vis, nrm, sh, kind, w.shape(C), flags)
        expect = lambda i, j: shref.forward(tmp, w.n_tris[i], w.v[i, 1], nw[i], sh[j % len(sh)], kind, fused, pre(w, C))  # noqa: E731
        same(got, np.stack([expect(i, i) for i in range(w.n)]), f"sh ({len(sh)} coefficient frames)")
        check_nobody(w, got, fused, "sh")
        if len(sh) > 1 and not fused:  # a frame reads its own coefficients: its neighbour's give other words
            some = range(0, w.n, max(1, w.n // 64))
            assert np.mean([expect(i, i).tobytes() != expect(i, (i + 1) % w.n).tobytes() for i in some]) >= 0.9


def run_sh_grad(tmp, w, fused):
    C, (nw, nrm), (gout, g), per = inputs(w)
    fs, kind, flags = w.fs, KIND[w.name], F if fused else 0
    gn, rows = backward(fs, w.vis, nrm, per, kind, g, w.n, flags)
    accs = [shref.Grad(C) for _ in range(w.n)]
    want = np.stack([shref.grad(tmp, w.n_tris[i], w.v[i, 1], nw[i], per[i], kind, gout[i], accs[i], fused, pre(w, 3)) for i in range(w.n)])
    same(gn, want, "sh_grad gnrm")
    check_nobody(w, gn, fused, "sh_grad gnrm")
    alone, none = backward(fs, w.vis, nrm, per, kind, g, w.n, flags, want_sh=False)  # k_sh_grad<false>
    assert none is None and np.array_equal(alone, gn), "sh_grad without d_gsh"
    if fused:
        return
    # (a) every entry is written; (b) the per-frame rows against the reference's double sums
    assert (rows != SENTINEL).all(), f"gsh: {int((rows == SENTINEL).sum())} entries were not written"
    gsum, gabs, cnt = (np.stack([getattr(a, k) for a in accs]) for k in ("gsum", "gabs", "count"))
    check_bound(rows.view(np.float32), gsum, gabs, cnt, f"gsh, {w.name}")
    # (e) a second launch, without the plane, gives the same words
    none, again = backward(fs, w.vis, nrm, per, kind, g, w.n, flags, want_nrm=False)
    assert none is None and np.array_equal(again, rows), "gsh: a second launch differs"
    # (c) the rows do not depend on the grid: the same frames in sets below the cap give the same words
    if w.name == "many":
        others = w.rng(35).choice(np.setdiff1d(np.arange(w.n), SMALL_SET), 9, replace=False)
        small_sets = [np.concatenate([SMALL_SET, np.sort(others)])]
    else:
        small_sets = [np.array([0]), np.array([w.n - 1])]
    for idx in small_sets:
        small = w.ctx.frameset([w.frames[i] for i in idx])
        vis = visibility(small)
        assert np.array_equal(words(vis), w.v[idx]), "the small set's visibility buffer is not the big set's slice"
        assert small.sh_work_bytes(C) < fs.sh_work_bytes(C)
        small_rows = backward(small, vis, dev(nw[idx]), per[idx], kind, dev(gout[idx]), len(idx), flags, want_nrm=False)[1]
        small.close()
        assert np.array_equal(small_rows, rows[idx]), f"gsh: the rows of frames {idx.tolist()} depend on the grid"
    if w.name == "many":
        # (d) shared coefficients: 0 + row 0 + row 1 + ... in float32 of the rows the same coefficients repeated give
        one = shref.make_sh(34, C)[None]
        total = backward(fs, w.vis, nrm, one, kind, g, w.n, flags, want_nrm=False)[1]
        rep = backward(fs, w.vis, nrm, np.repeat(one, w.n, 0), kind, g, w.n, flags, want_nrm=False)[1].view(np.float32)
        s = np.zeros((9, C), np.float32)
        for i in range(w.n):
            s = s + rep[i]
        assert total.shape == (1, 9, C) and np.array_equal(total[0], s.view(np.uint32)) and (s != 0).all(), "gsh: shared coefficients"
        # the bound can see a tile
        shares = Shares(gabs.shape)
        for _, f, rs, cs in w.tiles():
            a = shref.Grad(C)
            shref.grad(tmp, w.n_tris[f], w.v[f, 1][rs, cs], nw[f][:, rs, cs], per[f], kind, gout[f][:, rs, cs], a)
            shares.add(a.gabs, f)
        teeth(shares, gabs, cnt, "gsh", single=False)


PASSES = {"sh": run_sh, "sh_grad": run_sh_grad}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", list(PASSES))
def test_more_tiles_than_workgroups(worlds, tmp_path, name, shape):
    """(many: with and without the fused clear; large: without it, the stricter of the two — nobody's words must survive)"""
    w = worlds(shape)
    for fused in ((False, True) if shape == "many" else (False,)):
        PASSES[name](tmp_path, w, fused)
