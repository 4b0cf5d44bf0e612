"""not-gpu: the position gradients of the whole chain (tests/chainref.py: visibility → interpolate [→ texture] [+ depth] → antialias →
loss, composed from the references the passes are pinned to) held to frames that are RENDERED AGAIN with the geometry moved.  Every
reference is pinned elsewhere to differences of its own float64 restatement with the owners held fixed; that shows kernel ==
reference == the rule of include/srz.h, not that the rule is the derivative of what the rasteriser does.  Here the oracle renders
P + h d and P - h d, and the difference of the two losses is compared with <interior term + silhouette term, d>.

The mip lookup is not among the variants: its backward holds the level fixed by contract, so a re-rendered difference contains a
d lambda term the gradient rightly lacks."""
import numpy as np
import pytest

import chainref as cr

SCENES = cr.VARIANTS
MAX_NON_QUIET, MIN_QUIET, MIN_SHARE = 0.25, 24, 0.30


def shares(base):
    sil, inner = float(base.silhouette.gabs.sum()), float(base.interior.gabs.sum())
    return sil / (sil + inner), inner / (sil + inner)


@pytest.mark.parametrize("variant", SCENES)
def test_local_differences_by_re_rendering(tmp_path, orc, variant):
    """for every probe (a vertex along one axis, a triangle translated along one axis; chainref.probes) the central difference of the
    re-rendered loss at h = 2^-9 pixel against <gpos_interior + gpos_silhouette, d>, the gap relative to the sum over both terms of
    |gpos_i d_i|, the step being the float32 difference of the moved positions.  A probe is quiet when the id planes of the three
    renders are equal and aa_forward64's decision planes at the two ends equal the middle's: only quiet probes are asserted — across
    a change of owner the antialiased image is not continuous (test_translation_sweeps measures that).  The cap on the scenes: at
    most 25 % of a scene's probes are not quiet, at least 24 are.  Tolerance: four times the worst quiet gap measured on the CPU
    over the five scenes, 4 * 1.22e-3 (the texture scene's; the others: 9e-5 .. 5.5e-4): what is left is the float32 rounding of
    alpha, beta and the blended words in a sum of some 2000 pixels, an absolute 1e-7 .. 2e-6 of a loss difference whatever the
    probe — it does not fall with h, and depends on the seed.  A wrong corner, sign, axis or term is a gap of 0.05 .. 1."""
    s = cr.evaluate(tmp_path, orc, variant)
    q = s.quiet
    worst = float(s.gap[q, 0].max())
    print(f"{variant}: {len(q)} probes, {int(q.sum())} quiet; quiet gap worst {worst:.3e} median {np.median(s.gap[q, 0]):.3e}, recorded "
          f"{cr.QUIET_GAP[variant]:.3e}, tolerance {cr.TOL:.3e}; not quiet: worst {s.gap[~q, 0].max() if (~q).any() else 0:.3e}")
    assert (~q).mean() <= MAX_NON_QUIET and q.sum() >= MIN_QUIET, (len(q), int(q.sum()))
    bad = np.flatnonzero(q & (s.gap[:, 0] > cr.TOL))
    assert not len(bad), [(s.names[i], s.gap[i].tolist()) for i in bad[:6]]


@pytest.mark.parametrize("variant", SCENES)
def test_neither_term_can_be_left_out(tmp_path, orc, variant):
    """on the same quiet probes: with the silhouette term left out the worst gap exceeds ten tolerances in every scene; in the
    flat-colour scene the interior term is exactly zero, so the gap without it IS the full gap; in every other scene each term
    holds at least 30 % of the sum of |term| (the flat scene: the silhouette term all of it); the pairs the scenes rely on exist —
    both targets, both directions, and in the quad scene the interior edge."""
    s = cr.evaluate(tmp_path, orc, variant)
    q, base = s.quiet, s.base
    sil, inner = shares(base)
    print(f"{variant}: silhouette left out: worst gap {s.gap[q, 1].max():.3f}; interior left out: {s.gap[q, 2].max():.3f}; shares of the "
          f"sum of |term|: silhouette {sil:.2f} interior {inner:.2f}; pairs {base.counters}")
    assert s.gap[q, 1].max() > 10 * cr.TOL
    if variant == "flat":
        assert not base.interior.gabs.any() and not base.interior.gpos.any() and np.array_equal(s.gap[:, 2], s.gap[:, 0])
    else:
        assert sil >= MIN_SHARE and inner >= MIN_SHARE
        assert s.gap[q, 2].max() > 10 * cr.TOL
    for name in ("target_n", "target_f", "horizontal", "vertical") + (("interior",) if variant == "quad" else ()):
        assert base.counters[name] > 0, (name, base.counters)
    if variant == "depth":
        z = np.array(["z" in n.split()[-1] for n in s.names])
        assert (z & q).sum() >= 8 and base.total[:, :, 2].any()
    else:
        assert not base.total[:, :, 2].any()


def sweep_table(tmp_path, orc):
    P, attr, gouts = cr.sweep_inputs()
    rows = {}
    for name, gout in gouts.items():
        def grad_of(Q, gout=gout):
            r = cr.loss_and_grad(tmp_path, orc, Q, attr, gout)
            return r.L, r.total
        for dn, d in cr.SWEEP_DIRS.items():
            rows[name, dn] = cr.sweep(grad_of, P, d)
    return rows


def test_translation_sweeps(tmp_path, orc):
    """the discontinuity, measured: an axis-aligned quad of two triangles translated through 1.5 pixels in 96 steps along x, y and
    (1, 0.5); the change of L, the trapezoid integral of the analytic derivative and the largest mismatch of one step, under a
    uniform and a smooth gout.  Measured: uniform — change 1.67 / 3.65 / 1.61 against integrals 0.26 / 1.59 / 0.91, single steps of
    1/64 pixel off by 1.5 / 2.0 / 2.4; smooth — 17.04 / 18.27 / 26.17 against 16.29 / 17.23 / 25.89 (4.4 %, 5.7 %, 1.1 %), single steps
    off by 0.23 / 0.37 / 0.35.  Asserted, under the smooth gout only: the same sign, and a relative difference of at most twice the
    one measured.  (DESIGN.md names the causes of the jumps.)"""
    rows = sweep_table(tmp_path, orc)
    for (name, dn), (change, integral, jump) in rows.items():
        print(f"{name:8s} {dn:9s} change {change:9.4f} integral {integral:9.4f} relative difference {abs(integral - change) / abs(change):.4f} "
              f"largest single-step mismatch {jump:.4f}")
    for dn, rel in cr.SWEEP_REL.items():
        change, integral, _ = rows["smooth", dn]
        assert change * integral > 0 and abs(integral - change) <= 2 * rel * abs(change), (dn, change, integral)


@pytest.mark.parametrize("seed", cr.POSE_SEEDS)
def test_pose_recovery(tmp_path, orc, seed):
    """five flat-coloured triangles, a target rendered at the offset (0.8, -0.6) pixel, the loss 0.5 * sum (out - target)^2, plain
    descent on the two translation parameters, lr 0.004, 60 steps.  The interior term of a flat colour is zero: alone it leaves
    the error at 1.0000 pixel.  With the silhouette term it falls to 0.120 / 0.026 / 0.000 / 0.024 pixel (seeds 2, 4, 5, 7: the
    ones of 0 .. 7 whose trajectory settles; chainref.POSE_FINAL says what the others do, DESIGN.md has them all); asserted: below
    twice the worst of these."""
    P, attr = cr.pose_scene(seed)
    zero = np.zeros((3, cr.H, cr.W), np.float32)
    target = cr.loss_and_grad(tmp_path, orc, cr.translated(P, cr.POSE_OFFSET), attr, zero, want_grad=False).out

    def step_of(Q, term):
        out = cr.loss_and_grad(tmp_path, orc, Q, attr, zero, want_grad=False).out
        r = cr.loss_and_grad(tmp_path, orc, Q, attr, cr.pose_gout(out, target))
        return r.total if term == "both" else r.interior.gpos
    full = cr.descend(lambda Q: step_of(Q, "both"), P)
    inner = cr.descend(lambda Q: step_of(Q, "interior"), P)
    print(f"seed {seed}: error {full[0]:.4f} -> {full[-1]:.4f} pixel (recorded {cr.POSE_FINAL[seed]:.4f}, bound {cr.POSE_BOUND:.4f}); interior "
          f"term alone -> {inner[-1]:.4f}")
    assert abs(full[0] - 1.0) < 1e-12 and inner[-1] > 0.95
    assert full[-1] < cr.POSE_BOUND
