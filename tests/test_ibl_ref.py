"""not-gpu: the image-based-lighting passes' CPU reference (tests/ibl_ref.c through iblref.py) is pinned before the GPU is held to it.
Its binary64 build against the same rules written in torch float64 ops with autograd (both binary64: they differ in the order of
operations only); its binary32 build — the rules themselves — against the binary64 build, at 8 x the error measured here; hand KATs
with closed forms; the table against the same rule at many more samples and against an independent trigonometric quadrature, at 2 x
the discretisation error measured here."""
import numpy as np
import pytest
import torch

import iblref as ib

SHAPE = (48, 64)
N_TRIS = 7
TABLES = (2, 3, 8, 17)
# the table's discretisation error at m = 64 over an n = 8 table, binary64, MEASURED here (test_table_discretisation prints them): the
# worst |A| or |B| difference against the same rule at m = 256, and against iblref.table_polar on the rows nv > 0 and the columns of
# roughness >= 0.33 (where the polar quadrature, which has no importance sampling, has itself converged).  Asserted at 2 x.
MEASURED_TABLE_M256, MEASURED_TABLE_POLAR = 1.31e-3, 3.54e-4
TABLE_POLAR_MIN_COLUMN = 3  # of 8: roughness 0.33


def ids_of(seed, holes=True):
    return ib.rand_ids(np.random.default_rng(seed), 1, *SHAPE, N_TRIS, holes)[0]


def rel(got, want, mask):
    """the largest difference over the masked pixels relative to the plane set's largest magnitude there"""
    g, w = np.float64(got)[:, mask], np.float64(want)[:, mask]
    return float(np.abs(g - w).max() / max(np.abs(w).max(), 1e-300))


# ------------------------------------------------------------------------------------------------ reflect
@pytest.fixture(scope="module")
def reflect_case(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("iblref")
    ids, eye = ids_of(1), ib.make_eye(2)
    nrm, pos, gout = ib.reflect_planes(3, SHAPE)
    return tmp, ids, eye, nrm, pos, gout


def test_reflect_binary64_is_the_torch_rule(reflect_case):
    tmp, ids, eye, nrm, pos, gout = reflect_case
    own = ((ids & 0x7fffffff) - np.uint32(1)) < N_TRIS
    well = own & ib.reflect_well_conditioned(nrm, pos, eye)
    assert well.sum() >= 0.9 * own.sum()
    t = [torch.tensor(np.float64(a)[None], requires_grad=True) for a in (nrm, pos)]
    e = torch.tensor(np.float64(eye), requires_grad=True)
    out = ib.torch_reflect(t[0], t[1], e)
    g = torch.tensor(np.float64(gout)[None]) * torch.tensor(own[None, None].astype(np.float64))
    out.backward(g)
    want = ib.reflect(tmp, N_TRIS, ids, nrm, pos, eye, dtype=np.float64)
    gn, gp = ib.reflect_grad(tmp, N_TRIS, ids, nrm, pos, eye, gout, dtype=np.float64)
    for name, got, ref in (("out", out.detach().numpy()[0], want), ("gnrm", t[0].grad.numpy()[0], gn), ("gpos", t[1].grad.numpy()[0], gp)):
        err = rel(got, ref, well)
        print(f"reflect {name}: {err:.3g}")
        assert err <= 1e-9, name
    # the eye's gradient is minus the owned pixels' gpos, summed: translation invariance
    assert np.allclose(e.grad.numpy(), -gp[:, own].sum(1), rtol=1e-9, atol=1e-12)


def test_reflect_binary32_against_binary64(reflect_case):
    tmp, ids, eye, nrm, pos, gout = reflect_case
    own = ((ids & 0x7fffffff) - np.uint32(1)) < N_TRIS
    well = own & ib.reflect_well_conditioned(nrm, pos, eye)
    worst = 0.0
    for name, a, b in zip(("out", "gnrm", "gpos"),
                          (ib.reflect(tmp, N_TRIS, ids, nrm, pos, eye),) + ib.reflect_grad(tmp, N_TRIS, ids, nrm, pos, eye, gout),
                          (ib.reflect(tmp, N_TRIS, ids, nrm, pos, eye, dtype=np.float64),) +
                          ib.reflect_grad(tmp, N_TRIS, ids, nrm, pos, eye, gout, dtype=np.float64)):
        err = rel(a, b, well)
        print(f"reflect {name}: binary32 against binary64 {err:.3g} of the plane's max")
        worst = max(worst, err)
    print(f"worst {worst:.3g}; recorded {ib.MEASURED_REFLECT:.3g}")
    assert worst <= 8 * ib.MEASURED_REFLECT


def test_reflect_kats(tmp_path):
    one = np.uint32([[1]])

    def px(n, P, eye, g=(0, 0, 0, 0)):
        n, P = np.float32(n).reshape(3, 1, 1), np.float32(P).reshape(3, 1, 1)
        out = ib.reflect(tmp_path, 1, one, n, P, np.float32(eye))
        gn, gp = ib.reflect_grad(tmp_path, 1, one, n, P, np.float32(eye), np.float32(g).reshape(4, 1, 1))
        return out.ravel(), gn.ravel(), gp.ravel()
    # N = Vd: R = N and nv = 1 (lengths that are powers of two: every step exact)
    out, _, _ = px((0, 0, 4), (0.5, 0.25, 0), (0.5, 0.25, 2))
    assert out.tolist() == [0, 0, 1, 1]
    # the mirror: the eye at 45 degrees in the xz plane over a normal +z: R = (-x, 0, z) of Vd, nv = Vd.z
    out, _, _ = px((0, 0, 1), (0, 0, 0), (3, 0, 3))
    s = np.float32(3) * (np.float32(1) / np.sqrt(np.float32(18)))
    assert out[1] == 0 and out[3] == s and abs(out[0] + s) <= 1e-7 and abs(out[2] - s) <= 1e-7
    # not lit (a zero, NaN or infinite normal), no view (the eye at P): four zeros, no gradient
    for n, P in (((0, -0.0, 0), (0, 0, 0)), ((np.nan, 0, 1), (0, 0, 0)), ((np.inf, 0, 1), (0, 0, 0)), ((0, 0, 1), (1, 2, 3))):
        out, gn, gp = px(n, P, (1, 2, 3), (1, -2, 3, 0.5))
        assert (out.view(np.uint32) == 0).all() and (gn == 0).all() and (gp == 0).all()
    # a nobody pixel: untouched without the fused clear, zeros with it
    pre = np.full((4, 1, 1), 0xdeadbeef, np.uint32)
    z = np.zeros((3, 1, 1), np.float32)
    assert (ib.reflect(tmp_path, 1, np.uint32([[0]]), z, z, np.float32([0, 0, 1]), fused=False, prefill=pre).view(np.uint32) == 0xdeadbeef).all()
    assert (ib.reflect(tmp_path, 1, np.uint32([[0]]), z, z, np.float32([0, 0, 1]), fused=True, prefill=pre).view(np.uint32) == 0).all()
    # a gradient along N through nv only: gnrm is perpendicular to N, gpos to Vd
    _, gn, gp = px((0.3, -0.2, 2), (0.1, 0.2, 0), (1, 1, 4), (0, 0, 0, 1))
    N, V = np.float64([0.3, -0.2, 2]), np.float64([0.9, 0.8, 4])
    assert abs(gn @ N) <= 1e-6 and abs(gp @ V) <= 1e-6 and np.abs(gn).max() > 1e-3


def test_reflect_hostile_case_meets_every_branch(tmp_path):
    case = ib.hostile_reflect(**ib.HOSTILE)
    for name, m in ib.reflect_branches(tmp_path, ib.HOSTILE["tris"], *case).items():
        assert int(m.sum()) >= 50, (name, int(m.sum()))


# ------------------------------------------------------------------------------------------------ ibl
@pytest.fixture(scope="module")
def ibl_cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("iblref2")
    return tmp, {t: (ids_of(10 + t), ib.smooth_table(t)) + ib.ibl_planes(20 + t, SHAPE, t) for t in TABLES}


def test_ibl_binary64_is_the_torch_rule(ibl_cases):
    tmp, cases = ibl_cases
    for t, (ids, tab, base, mat, nv, irr, spec, gout) in cases.items():
        own = ((ids & 0x7fffffff) - np.uint32(1)) < N_TRIS
        well = own & ib.ibl_well_conditioned(mat, nv, t)
        print(f"table {t}: {well.sum() / own.sum():.3f} of the owned pixels are well-conditioned")
        assert well.sum() >= 0.9 * own.sum()
        for with_base in (True, False):
            ins = [torch.tensor(np.float64(a)[None], requires_grad=True) for a in (base, mat, nv, irr, spec)]
            tt = torch.tensor(np.float64(tab), requires_grad=True)
            out = ib.torch_ibl(ins[0] if with_base else None, ins[1], ins[2], ins[3], ins[4], tt)
            # gout on the well-conditioned pixels only: the table's gradient is a sum over pixels
            g = np.float64(gout) * well
            out.backward(torch.tensor(g[None]))
            b = base if with_base else None
            want = ib.ibl(tmp, N_TRIS, ids, b, mat, nv, irr, spec, tab, dtype=np.float64)
            acc = ib.TabGrad(t)
            grads = ib.ibl_grad(tmp, N_TRIS, ids, b, mat, nv, irr, spec, tab, g, into=acc, dtype=np.float64)
            names = ("out", "gbase", "gmat", "gnv", "girr", "gspec")
            got = [out.detach().numpy()[0]] + [None if (i == 0 and not with_base) else x.grad.numpy()[0] for i, x in enumerate(ins)]
            for name, a, r in zip(names, got, (want,) + grads):
                assert (a is None) == (r is None), name
                if a is not None:
                    assert rel(a, r, well) <= 1e-9, (t, name, rel(a, r, well))
            err = np.abs(tt.grad.numpy() - acc.gsum).max() / np.abs(acc.gsum).max()
            assert err <= 1e-9, (t, "gtab", err)
            assert (acc.count.sum(), acc.gabs.min() >= 0) == (8 * own.sum(), True)


def test_ibl_binary32_against_binary64(ibl_cases):
    tmp, cases = ibl_cases
    worst = 0.0
    for t, (ids, tab, base, mat, nv, irr, spec, gout) in cases.items():
        own = ((ids & 0x7fffffff) - np.uint32(1)) < N_TRIS
        well = own & ib.ibl_well_conditioned(mat, nv, t)
        a32, a64 = ib.TabGrad(t), ib.TabGrad(t)
        g = gout * well
        lo = (ib.ibl(tmp, N_TRIS, ids, base, mat, nv, irr, spec, tab),) + ib.ibl_grad(tmp, N_TRIS, ids, base, mat, nv, irr, spec, tab, g, into=a32)
        hi = (ib.ibl(tmp, N_TRIS, ids, base, mat, nv, irr, spec, tab, dtype=np.float64),) + \
            ib.ibl_grad(tmp, N_TRIS, ids, base, mat, nv, irr, spec, tab, g, into=a64, dtype=np.float64)
        for name, a, b in zip(("out", "gbase", "gmat", "gnv", "girr", "gspec"), lo, hi):
            err = rel(a, b, well)
            print(f"table {t} {name}: binary32 against binary64 {err:.3g} of the plane's max")
            worst = max(worst, err)
        err = float(np.abs(a32.gsum - a64.gsum).max() / np.abs(a64.gsum).max())  # (both sums in double: the terms' error alone)
        print(f"table {t} gtab: {err:.3g} of the table's max")
        worst = max(worst, err)
    print(f"worst {worst:.3g}; recorded {ib.MEASURED_IBL:.3g}")
    assert worst <= 8 * ib.MEASURED_IBL


def one_px(tmp_path, tab, base, mat, nv, irr, spec, g=(1, 1, 1), dtype=np.float32):
    sh = lambda a, k: None if a is None else np.asarray(a, dtype).reshape(k, 1, 1)  # noqa: E731
    args = (sh(base, 3), sh(mat, 2), sh(nv, 1), sh(irr, 3), sh(spec, 3), np.asarray(tab, dtype))
    out = ib.ibl(tmp_path, 1, np.uint32([[1]]), *args, dtype=dtype)
    grads = ib.ibl_grad(tmp_path, 1, np.uint32([[1]]), *args, sh(g, 3), dtype=dtype, want_terms=True)
    return out.ravel(), grads


def test_ibl_kats(tmp_path):
    f32 = np.float32
    # a table of constants (A, B): out = cdif irr + spec (F0 A + B) in closed form, whatever nv and the roughness are
    tab = np.zeros((4, 4, 2), f32)
    tab[..., 0], tab[..., 1] = 0.75, 0.125
    base, irr, spec = f32([0.5, 0.25, 1.0]), f32([1.0, 2.0, 0.5]), f32([2.0, 1.0, 4.0])
    for nv, r in ((0.3, 0.4), (-1.0, 0.0), (2.0, 7.0), (np.nan, np.nan)):
        out, _ = one_px(tmp_path, tab, base, (r, 0.5), nv, irr, spec)
        F0 = f32(0.5) * (base - f32(0.04)) + f32(0.04)
        want = (base * f32(0.5)) * irr + spec * (F0 * f32(0.75) + f32(0.125))
        assert np.allclose(out, want, rtol=3e-7, atol=0), (nv, r, out, want)
    # metallic 1: the diffuse term is exactly 0 (cdif = base * (1 - 1)); F0 = base up to fmaf's one rounding
    out, _ = one_px(tmp_path, tab, base, (0.5, 1.0), 0.5, irr, spec)
    out0, _ = one_px(tmp_path, tab, base, (0.5, 1.0), 0.5, f32([0, 0, 0]), spec)
    assert np.array_equal(out.view(np.uint32), out0.view(np.uint32))
    # base null = ones
    for m in (0.0, 0.3, 1.0):
        a, ga = one_px(tmp_path, tab, None, (0.5, m), 0.5, irr, spec)
        b, gb = one_px(tmp_path, tab, (1, 1, 1), (0.5, m), 0.5, irr, spec)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and ga[0] is None and gb[0] is not None
        for x, y in zip(ga[1:5], gb[1:5]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # every clamp edge and NaN takes its stated branch: the value at the edge, and no gradient at or beyond it
    tab = ib.smooth_table(5)
    edge = {"nv": (0.0, 1.0), "r": (ib.RMIN, 1.0), "m": (0.0, 1.0)}
    for which, (lo, hi) in edge.items():
        for v, at in ((lo, lo), (-0.0 if lo == 0 else f32(lo) - f32(1e-3), lo), (-3.0, lo), (np.nan, lo), (-np.inf, lo), (hi, hi), (1.5, hi), (np.inf, hi)):
            arg = dict(nv=0.37, r=0.41, m=0.6)
            arg[which] = v
            out, g = one_px(tmp_path, tab, base, (arg["r"], arg["m"]), arg["nv"], irr, spec)
            arg[which] = at
            ref, _ = one_px(tmp_path, tab, base, (arg["r"], arg["m"]), arg["nv"], irr, spec)
            assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), (which, v)
            grad = {"nv": g[2].ravel()[0], "r": g[1].ravel()[0], "m": g[1].ravel()[1]}[which]
            assert grad == 0, (which, v, grad)
    # strictly inside: all three gradients are there
    _, g = one_px(tmp_path, tab, base, (0.41, 0.6), 0.37, irr, spec)
    assert g[2].ravel()[0] != 0 and (g[1].ravel() != 0).all()
    # nv, or a roughness, exactly on a node returns the node's word: a table of dyadic words (every difference exact, the last node
    # too), 17 rows (nv_i = i / 16 exact) and 16 columns' worth of roughness nodes (n = 16: sy = 16, rc_j = 1 / 16 + j / 16 exact)
    for t in (17, 16):
        rng = np.random.default_rng(t)
        tab = (rng.integers(1, 64, (t, t, 2)) / 64).astype(f32)
        for i in range(t):
            for j in range(t):
                nv = f32(i) / f32(t - 1)
                r = f32(ib.RMIN) + f32(ib.RSPAN) * (f32(j) / f32(t - 1))
                if t == 17 and j not in (0, 16):
                    continue  # (n = 17: only the edge columns are exact)
                if t == 16 and i not in (0, 15):
                    continue
                # base 1, metallic 1, irr 0, spec 1: out = fmaf(1, A, B) = A + B, one rounding of an exact dyadic sum: exact
                out, _ = one_px(tmp_path, tab, (1, 1, 1), (r, 1.0), nv, (0, 0, 0), (1, 1, 1))
                assert out[0] == tab[i, j, 0] + tab[i, j, 1], (t, i, j)
    # one pixel's table terms: the four weights sum to 1, so the A terms sum to gA = dot(g * spec, F0) and the B terms to dot(g, spec)
    tab = ib.smooth_table(8).astype(np.float64)
    _, g = one_px(tmp_path, tab, base, (0.41, 0.6), 0.37, irr, spec, g=(0.5, -2.0, 1.5), dtype=np.float64)
    terms, cell = g[5].ravel(), g[6].ravel()
    F0 = 0.6 * (np.float64(base) - ib.F004) + ib.F004
    gs = np.float64([0.5, -2.0, 1.5]) * np.float64(spec)
    assert abs(terms[:4].sum() - gs @ F0) <= 1e-12 and abs(terms[4:].sum() - gs.sum()) <= 1e-12
    assert cell.tolist() == [int(0.37 * 7), int((0.41 - ib.RMIN) * 7 / ib.RSPAN)]


def test_ibl_hostile_case_meets_every_branch(tmp_path):
    case = ib.hostile_ibl(**ib.HOSTILE)
    for name, m in ib.ibl_branches(tmp_path, ib.HOSTILE["tris"], *case).items():
        assert int(m.sum()) >= 50, (name, int(m.sum()))
    # and no pixel's cell leaves the table, whatever the planes hold
    _, tab, _, mat, nv = case[:5]
    assert ib.ibl_cell_words(tab, mat, nv).shape[-1] == 8


# ------------------------------------------------------------------------------------------------ the table
def test_table_discretisation(tmp_path):
    """binary64, n = 8, m = 64: against the same rule at m = 256 and against the independent polar quadrature.  The error is the
    quadrature's alone; measured here, asserted at 2 x"""
    n = 8
    tab = ib.table(tmp_path, n, 64, np.float64)
    fine = ib.table(tmp_path, n, 256, np.float64)
    polar = ib.table_polar(n)
    e_fine = float(np.abs(tab - fine).max())
    c0 = TABLE_POLAR_MIN_COLUMN
    e_polar = float(np.abs(tab[1:, c0:] - polar[1:, c0:]).max())
    print(f"n 8 m 64: against m 256 {e_fine:.3g} (recorded {MEASURED_TABLE_M256:.3g}), against the polar quadrature {e_polar:.3g} "
          f"(recorded {MEASURED_TABLE_POLAR:.3g}); m 256 against polar {np.abs(fine[1:, c0:] - polar[1:, c0:]).max():.3g}")
    assert e_fine <= 2 * MEASURED_TABLE_M256 and e_polar <= 2 * MEASURED_TABLE_POLAR
    # nv = 1, the smoothest lobe: A -> 1 and B -> 0 (F0 = 1: a white furnace returns everything Smith lets through, and at normal
    # incidence on a near-mirror that is all of it), within the bound
    assert abs(tab[n - 1, 0, 0] - 1) <= 2 * MEASURED_TABLE_M256 and abs(tab[n - 1, 0, 1]) <= 2 * MEASURED_TABLE_M256
    assert (tab >= 0).all() and (tab.sum(-1) <= 1 + 2 * MEASURED_TABLE_M256).all()
    # binary32 against binary64 at the same m: rounding only, far below the discretisation
    t32 = ib.table(tmp_path, n, 64)
    print(f"binary32 against binary64 at m 64: {np.abs(t32 - tab).max():.3g}")
    assert np.abs(t32 - tab).max() <= 1e-4


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_table_symmetry_at_normal_incidence(tmp_path, dtype):
    """nv = 1: v = (0, 0, 1), vx = 0, so vh = nv * hz whatever hx is: the two signs of hx give the same words"""
    for n, m in ((2, 4), (3, 16), (8, 64)):
        _, signs = ib.table(tmp_path, n, m, dtype, want_signs=True)
        assert np.array_equal(signs[n - 1, :, 0], signs[n - 1, :, 1]) and (signs[n - 1, :, 0] > 0).all()
        assert not np.array_equal(signs[0, :, 0], signs[0, :, 1])
