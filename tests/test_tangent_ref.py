"""not-gpu: the CPU reference of the mesh tangents and of the normal-mapping pass (tests/tangent_ref.c through tangentref.py) is
pinned before the GPU is held to it: hand KATs; its binary64 build against the same rules written in torch float64 ops with autograd
(both binary64: they differ in the order of operations only) and against central differences away from the branch boundaries; its
binary32 build against the binary64 one within derived bounds; every fallback branch."""
import numpy as np
import pytest
import torch

import normalsref as nr
import tangentref as tr
import vgkit

SHAPE = (40, 56)
N_TRIS = 5
U = 2.0 ** -24


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("tangentref")


def dyadic_grid(n=5):
    """n x n vertices at multiples of 1 / (n - 1) (n - 1 a power of two) in the plane z = 0.5, two faces a cell, counter-clockwise seen
    from +z -> (pos, faces): every difference and product of the tangent rule is exact"""
    ys, xs = np.mgrid[0:n, 0:n]
    pos = np.stack([xs.reshape(-1) / (n - 1), ys.reshape(-1) / (n - 1), np.full(n * n, 0.5)], 1).astype(np.float32)
    faces = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            faces += [[a, a + 1, a + n + 1], [a, a + n + 1, a + n]]
    return pos, np.array(faces, np.uint32)


def sums64(L, pos, uv):
    """the tangent rule's sums in float64 from the float32 inputs -> (S [V, 3], SA [V, 3] the sums of |e1 dv2| + |e2 dv1| per component,
    the valences [V])"""
    p, q, f = np.float64(pos), np.float64(uv), L.f
    d1, d2 = q[f[:, 1]] - q[f[:, 0]], q[f[:, 2]] - q[f[:, 0]]
    det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
    e1, e2 = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
    Tf = (e1 * d2[:, 1:2] - e2 * d1[:, 1:2]) * np.where(det < 0, -1.0, 1.0)[:, None]
    A = np.abs(e1 * d2[:, 1:2]) + np.abs(e2 * d1[:, 1:2])
    S, SA, val = np.zeros_like(p), np.zeros_like(p), np.zeros(len(p))
    for k in range(3):
        np.add.at(S, f[:, k], Tf), np.add.at(SA, f[:, k], A), np.add.at(val, f[:, k], 1.0)
    return S, SA, val


# ------------------------------------------------------------------------------------------------ hand KATs: the tangents
@pytest.mark.parametrize("mirrored", [False, True])
def test_planar_grid_with_uv_equal_to_xy(tmp, mirrored):
    """uv = (x, y): every face's Tf is (det, 0, 0) exactly, S = (sum |det|, 0, 0) with sums valence / 16 — 1, 2, 3 or 6 sixteenths, for
    which x * fl(1 / x) rounds to 1 —, so t = (1, 0, 0) and w = +1 EXACTLY.  u mirrored (uv = (1 - x, y)): every det is negative, t still
    points along +u, which is -x: t = (-1, 0, 0), w = -1.  With the winding's normal (0, 0, 1), w * cross(N, t) = (0, 1, 0): +v"""
    pos, faces = dyadic_grid()
    uv = pos[:, :2].copy()
    if mirrored:
        uv[:, 0] = 1.0 - uv[:, 0]
    L = tr.Lists(tmp, faces, len(pos))
    sgn = -1.0 if mirrored else 1.0
    for dt in (np.float32, np.float64):
        t = tr.tangents(tmp, L, pos, uv, dtype=dt)
        assert np.array_equal(t, np.tile(dt([sgn, 0, 0, sgn]), (len(pos), 1))), t
        b = t[:, 3:4] * np.cross(np.tile([0.0, 0.0, 1.0], (len(pos), 1)), t[:, :3])
        assert np.array_equal(b, np.tile([0.0, 1.0, 0.0], (len(pos), 1)))
    n = nr.normals(tmp, L, pos)
    assert np.array_equal(n, np.tile(np.float32([0, 0, 1]), (len(pos), 1)))
    cls = tr.tangents_classify(tmp, L, pos, uv)
    assert (cls == (tr.NAMED | tr.NORMALISED | (tr.W_NEG if mirrored else 0))).all()


def test_a_face_weighs_in_by_its_uv_area(tmp):
    """two faces around vertex 0 with tangents along x and along y; the second face's uv are twice as large in both directions: Tf =
    det * dP/du, det grows fourfold and dP/du halves, so its term is twice as long.  t = (1, 2, 0) / sqrt(5)"""
    pos = np.float32([[0, 0, 0], [1, 0, 0], [0, 0, 1], [0, 1, 0], [0, 0, -1]])
    uv = np.float32([[0, 0], [1, 0], [0, 1], [2, 0], [0, 2]])
    faces = np.array([[0, 1, 2], [0, 3, 4]], np.uint32)
    t = tr.tangents(tmp, tr.Lists(tmp, faces, 5), pos, uv, dtype=np.float64)
    assert np.allclose(t[0], [1 / np.sqrt(5), 2 / np.sqrt(5), 0, 1], rtol=0, atol=1e-15)
    assert np.array_equal(t[1], [1, 0, 0, 1]) and np.array_equal(t[3], [0, 1, 0, 1])


# ------------------------------------------------------------------------------------------------ hand KATs: the pass
def _one(tmp, n, t, m, g=(1.0, 1.0, 1.0), dtype=np.float32):
    col = lambda v: np.asarray(v, dtype).reshape(-1, 1, 1)  # noqa: E731
    ids = np.ones((1, 1), np.uint32)
    out = tr.nm_forward(tmp, 1, ids, col(n), col(t), col(m), dtype=dtype)
    grads = tr.nm_grad(tmp, 1, ids, col(n), col(t), col(m), col(g), dtype=dtype)
    return out.reshape(3), [x.reshape(-1) for x in grads], int(tr.nm_classify(tmp, 1, ids, col(n), col(t), col(m))[0, 0])


def test_axis_aligned_frame_by_hand(tmp):
    """n = (0, 0, 2), t = (3, 0, 4): N = (0, 0, 1), d = 4, Tp = (3, 0, 0), T = (1, 0, 0) exactly (3 * fl(1 / 3) rounds to 1), B = (0, 1,
    0) * sign(w).  m = (1, 0, 0) gives T, m = (0, 1, 0) gives B, m = (0, 0, 1) gives N, m = (3, 0, 4) gives (0.6, 0, 0.8) to an ulp"""
    for w, by in ((1.0, 1.0), (-1.0, -1.0), (0.0, 1.0), (-0.0, 1.0), (7.0, 1.0)):
        t = (3, 0, 4, w)
        for m, want in (((1, 0, 0), (1, 0, 0)), ((0, 1, 0), (0, by, 0)), ((0, 0, 1), (0, 0, 1)), ((0, -2, 0), (0, -by, 0))):
            out, _, cls = _one(tmp, (0, 0, 2), t, m)
            assert cls == tr.OWNED | tr.LIT | tr.FRAME | tr.MAPPED
            assert np.array_equal(out, np.float32(want)), (w, m, out)
    out, (gn, gt, gm), _ = _one(tmp, (0, 0, 2), (3, 0, 4, 1), (3, 0, 4), g=(1, 0, 0), dtype=np.float64)
    assert np.allclose(out, [0.6, 0, 0.8], rtol=0, atol=2e-16)
    # out = R / |R|, R = (3, 0, 4) in the frame: d out.x / d m = (I - o o^T) e_x / 5 = (0.64, 0, -0.48) / 5
    assert np.allclose(gm, [0.128, 0, -0.096], rtol=0, atol=1e-15)
    assert gt[3] == 0 and np.allclose(gt[1], 0, atol=1e-16)


def test_flat_map_returns_the_normal_within_one_more_normalisation(tmp):
    """m = (0, 0, 1): R = fmaf(0, T, fmaf(0, B, 1 * N)) is N itself, so out = N * fl(1 / sqrt(fl(dot(N, N)))).  DERIVED: every N_c carries
    the relative error of inl (gamma_3 / 2 from the three roundings of dot under the root, the root, the division: 3.5 u) and of its own
    product (u): |N| = 1 + e, |e| <= 4.5 u; ir repeats that on dot(N, N) = |N|² (1 + gamma_3): ir = (1 / |N|)(1 + 3.5 u), and the last
    product adds u.  out_c = N_c (1 + 4.5 u) / (1 + e): |out_c - N_c| <= 9 u |N_c| to first order; gamma_10 |N_c| is asserted, in
    binary32 (u = 2^-24) and in binary64 (u = 2^-53) alike, and the worst ratio is printed"""
    nrm, tan, _, _ = tr.make_planes(3, SHAPE)
    ids = np.ones(SHAPE, np.uint32)
    m = np.zeros((3,) + SHAPE, np.float32)
    m[2] = 1.0
    for dt, u in ((np.float32, 2.0 ** -24), (np.float64, 2.0 ** -53)):
        out = np.float64(tr.nm_forward(tmp, 1, ids, nrm, tan, m, dtype=dt))
        N = np.float64(tr.nm_forward(tmp, 1, ids, nrm, np.zeros_like(tan), m, dtype=dt))  # (no frame: the unperturbed normal)
        assert (tr.nm_classify(tmp, 1, ids, nrm, tan, m) == 15).all()
        gamma10 = 10 * u / (1 - 10 * u)
        err = np.abs(out - N)
        print(dt.__name__, "worst |out - N| / (u |N_c|):", float((err / np.maximum(np.abs(N), 1e-300)).max() / u))
        assert (err <= gamma10 * np.abs(N)).all()
        assert np.abs(np.sqrt((N * N).sum(0)) - 1).max() <= 5 * u


def test_m_along_x_returns_the_orthonormalised_tangent(tmp):
    """m = (1, 0, 0) on random planes: out is T, the tangent made orthogonal to N and normalised — against numpy in float64"""
    nrm, tan, _, _ = tr.make_planes(4, SHAPE)
    m = np.zeros((3,) + SHAPE, np.float32)
    m[0] = 1.0
    out = tr.nm_forward(tmp, 1, np.ones(SHAPE, np.uint32), nrm, tan, m, dtype=np.float64)
    n, t = np.float64(nrm), np.float64(tan[:3])
    N = n / np.sqrt((n * n).sum(0))
    Tp = t - N * (N * t).sum(0)
    T = Tp / np.sqrt((Tp * Tp).sum(0))
    assert np.abs(out - T).max() <= 1e-14
    # binary32, DERIVED: N_c is off by 4.5 u (the test above), d = dot(N, t) by (4.5 + 3) u |t|, the product N_c d and the subtraction
    # add u |t| each: a component of Tp is off by at most 14 u |t|, the vector by sqrt(3) times that (24 u |t|);
    # || x / |x| - y / |y| || <= 2 |x - y| / |y| carries it through the normalisation (48 u |t| / |Tp|), whose own roundings and the
    # last normalisation of R = T add 4.5 u + 4.5 u more
    out32 = tr.nm_forward(tmp, 1, np.ones(SHAPE, np.uint32), nrm, tan, m)
    bound = (48.0 * np.sqrt((t * t).sum(0) / (Tp * Tp).sum(0)) + 9.0) * U
    print("binary32 T: worst error / bound", float((np.abs(out32 - T) / bound).max()))
    assert (np.abs(out32 - T) <= bound).all()


# ------------------------------------------------------------------------------------------------ binary64 against torch autograd
MESH_CASES = (("grid", "affine"), ("grid", "sheared"), ("grid", "mirrored"), ("soup", "random"), ("fan", "random"))


def mesh_case(name, kind):
    pos, faces = {"grid": lambda: vgkit.grid(7, 6, 3, extra=1), "soup": lambda: nr.soup(5), "fan": lambda: vgkit.fan(70, 2)}[name]()
    if name != "soup":
        pos[:, 2] += 0.3 * np.sin(5.0 * pos[:, 0]) * np.cos(3.0 * pos[:, 1])  # (off the plane: tangents that tilt)
    uv = tr.degenerate_face(tr.make_uv(pos, kind, 7), faces, 2)
    return pos.astype(np.float32), faces, uv


@pytest.mark.parametrize("name,kind", MESH_CASES)
def test_tangents_binary64_against_torch_autograd(tmp, name, kind):
    pos, faces, uv = mesh_case(name, kind)
    L = tr.Lists(tmp, faces, len(pos))
    g = np.random.default_rng(191).normal(0, 1, (len(pos), 4))
    t64 = tr.tangents(tmp, L, pos, uv, dtype=np.float64)
    gp64 = tr.tangents_grad(tmp, L, pos, uv, g, dtype=np.float64)
    P = torch.tensor(np.float64(pos), requires_grad=True)
    T = tr.torch_tangents(P, torch.tensor(np.float64(uv)), torch.tensor(faces.astype(np.int64)))
    (T * torch.tensor(g[:, :3])).sum().backward()
    assert np.abs(t64[:, :3] - T.detach().numpy()).max() <= 1e-12
    assert np.abs(gp64 - P.grad.numpy()).max() <= 1e-10 * max(1.0, np.abs(gp64).max())
    cls = tr.tangents_classify(tmp, L, pos, uv)
    if kind == "random":
        assert (cls & tr.W_NEG).any() and not (cls & tr.W_NEG).all()
    # the binary32 build against the binary64 one, DERIVED as normalsref.normals_bound: a component of a face's Tf carries two rounded
    # differences and a rounded product per term and the subtraction (gamma_4 of |e1 dv2| + |e2 dv1|; s * Tf is exact), then at most
    # `valence` adds of the sum: dS = |gamma_(valence + 4) SA|; || x / |x| - y / |y| || <= 2 |x - y| / |y| carries dS through the
    # normalisation, whose own roundings stay below gamma_6.  Held where dS < |S| / 2 (elsewhere the bound says nothing)
    S, SA, val = sums64(L, pos, uv)
    dS, ln = np.linalg.norm(nr.gamma(val + 4)[:, None] * SA, axis=1), np.linalg.norm(S, axis=1)
    e = (ln > 0) & (dS < 0.5 * ln)
    assert e.mean() >= 0.8, e.mean()
    t32 = tr.tangents(tmp, L, pos, uv)
    bound = 2.0 * dS[e] / ln[e] + nr.gamma(6)
    err = np.abs(t32[e, :3] - t64[e, :3]).max(1)
    print("binary32 tangents: worst error / bound", float((err / bound).max()))
    assert (err <= bound).all()


def test_normal_map_binary64_against_torch_autograd(tmp):
    nrm, tan, m, gout = tr.make_planes(5, SHAPE)
    good = tr.well_conditioned(nrm, tan, m)
    assert good.mean() >= 0.9, good.mean()
    ids = np.where(good, np.uint32(3), np.uint32(0))
    t = lambda a: torch.tensor(np.float64(a), requires_grad=True)  # noqa: E731
    N_, T_, M_ = t(nrm), t(tan), t(m)
    out = tr.torch_normal_map(N_, T_, M_) * torch.tensor(np.float64(good))
    (out * torch.tensor(np.float64(gout))).sum().backward()
    fwd = tr.nm_forward(tmp, N_TRIS, ids, nrm, tan, m, dtype=np.float64)
    gn, gt, gm = tr.nm_grad(tmp, N_TRIS, ids, nrm, tan, m, gout, dtype=np.float64)
    assert np.abs(fwd - out.detach().numpy()).max() <= 1e-13
    for got, want in ((gn, N_.grad), (gt, T_.grad), (gm, M_.grad)):
        want = want.numpy()
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    assert not gt[3].any()
    # binary32 against binary64 on the same pixels, DERIVED in units of u with rho = |t| / |Tp| (the projection's cancellation): N is off
    # by eN = 8 as a vector (4.5 u a component), T by eT = 48 rho + 5 (test_m_along_x_...), B = cross(N, T) * hw by eN + eT + 4; R, of
    # length |m|, is a combination of the three with coefficients at most |m| and four more roundings: |dR| / |R| <= eT + eB + eN + 4;
    # the normalisation doubles that and adds its own 5: (192 rho + 73) u on every component
    f32 = tr.nm_forward(tmp, N_TRIS, ids, nrm, tan, m)
    n64, t64 = np.float64(nrm), np.float64(tan[:3])
    Nn = n64 / np.sqrt((n64 * n64).sum(0))
    Tp = t64 - Nn * (Nn * t64).sum(0)
    bound = (192.0 * np.sqrt((t64 * t64).sum(0) / (Tp * Tp).sum(0)) + 73.0) * U
    err = np.abs(f32 - fwd).max(0)
    print("binary32 forward against binary64: worst error / bound", float((err / bound)[good].max()))
    assert (err <= bound)[good].all()


# ------------------------------------------------------------------------------------------------ central differences in binary64
def test_normal_map_central_differences(tmp):
    """every one of the ten inputs of every kept pixel; the left-out share (classify: not MAPPED; or near a boundary) stays under 10 %"""
    nrm, tan, m, gout = tr.make_planes(6, SHAPE)
    keep = tr.well_conditioned(nrm, tan, m) & (tr.nm_classify(tmp, 1, np.ones(SHAPE, np.uint32), nrm, tan, m) == 15)
    print("left out:", 1 - keep.mean())
    assert 1 - keep.mean() <= 0.10
    ids = np.where(keep, np.uint32(1), np.uint32(0))
    x = [np.float64(nrm), np.float64(tan), np.float64(m)]
    loss = lambda: (tr.nm_forward(tmp, 1, ids, x[0], x[1], x[2], dtype=np.float64) * np.float64(gout)).sum(0)  # noqa: E731  per pixel
    grads = tr.nm_grad(tmp, 1, ids, *x, gout, dtype=np.float64)
    h = 1e-6
    for a, g in zip(x, grads):
        for c in range(3):  # (the w plane has no gradient and a step across 0 flips the frame: not differenced)
            a[c] += h
            up = loss()
            a[c] -= 2 * h
            dn = loss()
            a[c] += h
            fd = (up - dn) / (2 * h)
            assert np.abs(fd - g[c])[keep].max() <= 1e-6 * max(1.0, np.abs(g[c]).max()), c
    assert not grads[1][3].any()


@pytest.mark.parametrize("name,kind", MESH_CASES[2:])
def test_tangents_central_differences(tmp, name, kind):
    pos, faces, uv = mesh_case(name, kind)
    L = tr.Lists(tmp, faces, len(pos))
    p = np.float64(pos)
    g = np.random.default_rng(193).normal(0, 1, (len(pos), 4))
    # away from the one boundary (S = 0, the root's singularity): the vertex's own sum and those of the vertices it shares a face with
    t64 = tr.tangents(tmp, L, p, uv, dtype=np.float64)
    cls = tr.tangents_classify(tmp, L, pos, uv)
    f = L.f
    S, SA, _ = sums64(L, pos, uv)
    named = (cls & tr.NAMED) != 0
    weak = named & (np.linalg.norm(S, axis=1) < 0.03 * np.linalg.norm(SA, axis=1))  # (the faces' terms cancel to 3 %, or to nothing)
    bad = weak.copy()
    for k in range(3):
        np.logical_or.at(bad, f[:, k], weak[f].any(1))
    print("left out:", bad.mean())
    assert bad.mean() <= 0.10
    gp = tr.tangents_grad(tmp, L, p, uv, g, dtype=np.float64)
    loss = lambda: (tr.tangents(tmp, L, p, uv, dtype=np.float64)[:, :3] * g[:, :3]).sum()  # noqa: E731
    h = 1e-6
    worst = 0.0
    for v in np.flatnonzero(~bad)[:40]:
        for c in range(3):
            p[v, c] += h
            up = loss()
            p[v, c] -= 2 * h
            dn = loss()
            p[v, c] += h
            worst = max(worst, abs((up - dn) / (2 * h) - gp[v, c]))
    assert worst <= 1e-5 * max(1.0, np.abs(gp).max()), worst
    assert t64.shape == (len(pos), 4)


# ------------------------------------------------------------------------------------------------ every fallback branch
def test_every_branch_of_the_pass(tmp):
    """branch_planes drives them all; a pixel that is not lit gives zeros everywhere; one without a frame, or with R = 0 or not finite,
    gives the unperturbed normal — the output of the same pixel with a zero tangent — and a gradient to the normal only: the
    normalisation's derivative, what the pass gives for that zero tangent"""
    nrm, tan, m, gout, kind = tr.branch_planes(7, SHAPE)
    ids = np.where(np.random.default_rng(197).random(SHAPE) < 0.9, np.uint32(2), np.uint32(0))
    cls = tr.nm_classify(tmp, N_TRIS, ids, nrm, tan, m)
    for want in (0, tr.OWNED, tr.OWNED | tr.LIT, tr.OWNED | tr.LIT | tr.FRAME, 15):
        assert (cls == want).sum() >= 20, (want, int((cls == want).sum()))
    assert set(np.unique(kind)) == set(range(tr.BRANCH_KINDS))
    out = tr.nm_forward(tmp, N_TRIS, ids, nrm, tan, m)
    gn, gt, gm = tr.nm_grad(tmp, N_TRIS, ids, nrm, tan, m, gout)
    unlit = cls <= tr.OWNED
    for a in (out, gn, gt, gm):
        assert not a[:, unlit].view(np.uint32).any()
    plain = (cls & tr.LIT).astype(bool) & ~(cls & tr.MAPPED).astype(bool)
    zt = np.zeros_like(tan)
    outN = tr.nm_forward(tmp, N_TRIS, ids, nrm, zt, m)
    gnN, _, _ = tr.nm_grad(tmp, N_TRIS, ids, nrm, zt, m, gout)
    assert not tr.same_or_nan(out[:, plain], outN[:, plain]).any() and not tr.same_or_nan(gn[:, plain], gnN[:, plain]).any()
    assert not gt[:, plain].view(np.uint32).any() and not gm[:, plain].view(np.uint32).any()
    assert not gt[3].view(np.uint32).any()
    # kinds and branches agree: 1, 2 not lit; 3, 4 no frame; 5 and the NaN m of 6 stop at R
    own = ids != 0
    assert (cls[own & ((kind == 1) | (kind == 2))] == tr.OWNED).all()
    assert (cls[own & ((kind == 3) | (kind == 4))] == (tr.OWNED | tr.LIT)).all()
    assert (cls[own & (kind == 5)] == (tr.OWNED | tr.LIT | tr.FRAME)).all()
    # not fused: nobody's words stay
    pre = tr.nm_forward(tmp, N_TRIS, ids, nrm, tan, m, fused=False, prefill=0xdeadbeef)
    assert (pre.view(np.uint32)[:, ~own] == 0xdeadbeef).all() and not tr.same_or_nan(pre[:, own], out[:, own]).any()


def test_tangent_fallbacks(tmp):
    """a vertex no face names, and all-equal uv: a zero tangent, w = +1, no gradient; a NaN position: the vertices of its faces are
    not normalised, and — phase 2 reads no position — every gpos stays finite"""
    pos, faces = vgkit.fan(12, 2)
    L = tr.Lists(tmp, faces, len(pos))
    uv = tr.make_uv(pos, "affine")
    g = np.ones((len(pos), 4), np.float32)
    cls = tr.tangents_classify(tmp, L, pos, uv)
    lone = (cls & tr.NAMED) == 0
    assert lone.sum() == 1
    t = tr.tangents(tmp, L, pos, uv)
    assert np.array_equal(t[lone].view(np.uint32), np.float32([[0, 0, 0, 1]]).view(np.uint32))
    assert not tr.tangents_grad(tmp, L, pos, uv, g)[lone].view(np.uint32).any()
    eq = tr.make_uv(pos, "equal")
    t = tr.tangents(tmp, L, pos, eq)
    assert np.array_equal(t.view(np.uint32), np.tile(np.float32([0, 0, 0, 1]), (len(pos), 1)).view(np.uint32))
    assert not tr.tangents_grad(tmp, L, pos, eq, g).view(np.uint32).any()
    assert (tr.tangents_classify(tmp, L, pos, eq) & tr.NORMALISED == 0).all()
    bad = pos.copy()
    bad[3, 1] = np.nan
    t = tr.tangents(tmp, L, bad, uv)
    touched = np.zeros(len(pos), bool)
    f = L.f
    touched[f[(f == 3).any(1)].reshape(-1)] = True
    assert not t[touched, :3].view(np.uint32).any() and np.isfinite(t).all()
    assert (np.linalg.norm(t[~touched & ~lone, :3], axis=1) > 0.99).all()
    assert np.isfinite(tr.tangents_grad(tmp, L, bad, uv, g)).all()
