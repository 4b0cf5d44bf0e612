"""The checkers of tests/walkkit.py bite: on the CPU, without the library.  tests/test_gpu_pass_walk_lit.py holds the float-atomic sums of
the passes to gamma_n * sum |term|, which grows with n — so it deals its inputs in such a way that one tile's contribution is larger
than the bound (walkkit.teeth), and this file pins that to something executable.  A small case dealt by the same functions — nine
frames of 64 x 64, four full tiles each, hand-written owner words with holes —, the references' own results rounded to float32 as the
"device's" answer: the unmodified answer passes check_sum, check_gtab, check_gpar and same; with one tile's contribution removed, one
tile's added twice, or one frame's contribution added into the next frame's element instead of its own, the checker raises."""
import numpy as np
import pytest

import cuberef
import iblref
import lightref
import walkkit
from walkkit import Shares, check_gpar, check_gtab, check_sum, same, teeth

N, H, W, TRIS = 9, 64, 64, 20
TILES = list(walkkit.tile_boxes(N, H, W))


@pytest.fixture(scope="module")
def ids():
    return iblref.rand_ids(np.random.default_rng(5), N, H, W, TRIS)


def owners(ids):
    return ((ids & 0x7fffffff) - np.uint32(1)) < TRIS


def raises(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def test_check_sum_sees_a_tile_of_a_per_frame_cube(tmp_path, ids):
    """texture_cube_grad's gtex with one 4 x 4 cube of five channels per frame, as the `many` set has it"""
    rng = np.random.default_rng(6)
    cube = cuberef.make_cube(2, 4, 5, frames=N)
    dirs, gout = rng.normal(0, 1, (N, 3, H, W)).astype(np.float32), rng.normal(0, 2, (N, 5, H, W)).astype(np.float32)
    accs, shares = [cuberef.Grad(cube.shape[1:]) for _ in range(N)], Shares(cube.shape)
    for f in range(N):
        cuberef.grad(tmp_path, cube[f], TRIS, ids[f], dirs[f], gout[f], accs[f], False)
    per_tile = {}
    for t, f, rs, cs in TILES:
        a = cuberef.Grad(cube.shape[1:])
        cuberef.grad(tmp_path, cube[f], TRIS, ids[f][rs, cs], dirs[f][:, rs, cs], gout[f][:, rs, cs], a, False)
        shares.add(a.gabs, f)
        per_tile[t] = (f, a.gtex)
    ref, mag, cnt = np.stack([a.gtex for a in accs]), np.stack([a.gabs for a in accs]), np.stack([a.count for a in accs])[..., None]
    toothed = teeth(shares, mag, cnt, "gtex", require=False)
    assert toothed[(mag > 0) & (cnt > 0)].mean() >= 0.9
    got = ref.astype(np.float32)
    check_sum(got, ref, mag, cnt, "gtex")
    for t, (f, part) in per_tile.items():
        assert (toothed[f] & (part != 0)).any(), t
        for sign in (-1, 1):  # removed, added twice
            bad = got.copy()
            bad[f] = (ref[f] + sign * part).astype(np.float32)
            raises(check_sum, bad, ref, mag, cnt, "gtex")
    for f in range(N - 1):  # a frame's gradient in the next frame's cube
        bad = got.copy()
        bad[f], bad[f + 1] = 0, (ref[f + 1] + ref[f]).astype(np.float32)
        raises(check_sum, bad, ref, mag, cnt, "gtex")


@pytest.mark.parametrize("t", [8, 64])
def test_check_gtab_sees_a_dealt_tile(tmp_path, ids, t):
    """ibl_grad's gtab under deal_ibl and ibl_coords: every live tile has words on which the bound sees it lost or doubled; the words
    the dumped tiles add into are the ones it cannot, and they are few"""
    own = owners(ids)
    tile_of = walkkit.tile_index(N, H, W)
    counts = np.bincount(tile_of[own], minlength=len(TILES))
    cx, cy = walkkit.deal_ibl(counts, t)
    assert (cx >= 0).sum() >= 24 and (cx < 0).any()
    rng = np.random.default_rng(7)
    base, mat, _, irr, spec, gout = (np.stack(a) for a in zip(*(iblref.ibl_planes(i, (H, W), t) for i in range(N))))
    nv, mat[:, 0] = walkkit.ibl_coords(tile_of, own, cx, cy, t, rng)
    tab = iblref.smooth_table(t)
    acc, shares = iblref.TabGrad(t), Shares((t, t, 2))
    for f in range(N):
        iblref.ibl_grad(tmp_path, TRIS, ids[f], base[f], mat[f], nv[f], irr[f], spec[f], tab, gout[f], acc)
    per_tile = {}
    for k, f, rs, cs in TILES:
        a = iblref.TabGrad(t)
        iblref.ibl_grad(tmp_path, TRIS, ids[f][rs, cs], base[f][:, rs, cs], mat[f][:, rs, cs], nv[f][:, rs, cs], irr[f][:, rs, cs], spec[f][:, rs, cs],
                        tab, gout[f][:, rs, cs], a)
        shares.add(a.gabs)
        per_tile[k] = a.gsum
    toothed = teeth(shares, acc.gabs, acc.count, f"gtab {t}")
    got = acc.gsum.astype(np.float32)
    check_gtab(got, acc, "gtab")
    for k, part in per_tile.items():
        if cx[k] < 0:
            continue
        assert (toothed & (part != 0)).any(), k
        for sign in (-1, 1):
            raises(check_gtab, (acc.gsum + sign * part).astype(np.float32), acc, "gtab")


def test_check_gpar_sees_a_tile_and_a_frame(tmp_path, ids):
    """light_grad's per-frame gpar rows: four tiles a row"""
    L = 3
    par = lightref.make_params(4, L, frames=N)
    planes = [lightref.make_planes(10 + f, (H, W)) for f in range(N)]
    accs, shares = [lightref.Grad(L) for _ in range(N)], Shares((N, lightref.par_len(L)))
    for f, (nrm, pos, kd, gout) in enumerate(planes):
        lightref.grad(tmp_path, TRIS, ids[f], nrm, pos, kd, par[f], 5, gout, accs[f])
    per_tile = {}
    for k, f, rs, cs in TILES:
        a = lightref.Grad(L)
        nrm, pos, kd, gout = (p[:, rs, cs] for p in planes[f])
        lightref.grad(tmp_path, TRIS, ids[f][rs, cs], nrm, pos, kd, par[f], 5, gout, a)
        shares.add(a.gabs, f)
        per_tile[k] = (f, a.gsum)
    ref = np.stack([a.gsum for a in accs])
    toothed = teeth(shares, np.stack([a.gabs for a in accs]), np.stack([a.count for a in accs]), "gpar", require=False)
    assert toothed.all()
    got = ref.astype(np.float32)
    check_gpar(got, accs, "gpar")
    for k, (f, part) in per_tile.items():
        for sign in (-1, 1):
            bad = got.copy()
            bad[f] = (ref[f] + sign * part).astype(np.float32)
            raises(check_gpar, bad, accs, "gpar")
    for f in range(N - 1):
        bad = got.copy()
        bad[f], bad[f + 1] = 0, (ref[f + 1] + ref[f]).astype(np.float32)
        raises(check_gpar, bad, accs, "gpar")


def test_same_sees_a_tile_of_the_next_frame(tmp_path, ids):
    """the deterministic planes: light's colour planes with one tile taken from the frame behind, and a NaN on one side only"""
    par = lightref.make_params(4, 3)
    want = np.stack([lightref.forward(tmp_path, TRIS, ids[f], *lightref.make_planes(10 + f, (H, W))[:3], par, 5) for f in range(N)])
    same(want.copy(), want, "light")
    for _, f, rs, cs in TILES:
        bad = want.copy()
        bad[f][:, rs, cs] = want[(f + 1) % N][:, rs, cs]
        raises(same, bad, want, "light")
    bad = want.copy()
    bad[3, 1, 40, 7] = np.nan
    raises(same, bad, want, "light")
    raises(same, want, bad, "light")
