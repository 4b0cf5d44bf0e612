"""-m gpu: the perspective-correct chain end to end in torch — scene_positions and clip_q into interpolate_persp, and
interpolate_deriv_persp into texture_mip — against a float64 restatement of the same chain differentiated by central differences,
with a tolerance derived from the float32 chain's roundings and the atomics' bound; the screen-linear chain (interpolate_geo) must
miss that tolerance by far, so the test cannot pass on the old path."""
import numpy as np
import pytest
import torch

import mipref
import perspref
import vgkit
from srz import abi
from srz import visibility as V
from support import ctx, stream, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
W = H = 64
SLOT = 2
IDENT = np.eye(4, dtype=np.float32).reshape(16)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    g_nan, w_nan = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = (g_nan != w_nan) | (~g_nan & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first {np.argwhere(bad)[:4].tolist()}: got {g[bad][:4]} want {w[bad][:4]}"


def chain_scene(c):
    """a 5 x 5-vertex vgkit.grid mesh (32 faces) in slot SLOT under a perspective whose w runs from about 1.7 to 4.7 over the mesh"""
    pos, faces = vgkit.grid(5, 5, 7)
    m = vgkit.perspective(95.0, 88.0, 1.5, 1.5, w=2.0, wx=2.5, wy=-0.3, wz=0.5)
    faces = vgkit.oriented(pos, faces, m)
    c.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    sf = abi.SceneFrame(W, H, (0.0, 0.0, 1.0), np.zeros((0, 2, 3), np.float32), [(SLOT, abi.SHADER_NORMAL, -1, m, IDENT)], 1.0, 0.0, abi.FUSED_CLEAR)
    return pos, faces, m, sf


def pixel_losses(verts, m, attr, faces, tri, ys, xs, G):
    """the chain restated in float64: vgkit's vertex stage → the barycentrics of every owned pixel's sample point (its integer corner)
    in its owner, the owners held fixed → the rule → the interpolation → the pixel's share of the loss [N]"""
    rows = np.asarray(m, np.float64).reshape(4, 4).T
    r = np.asarray(verts, np.float64) @ rows[:, :3].T + rows[:, 3]
    sx, sy, q = r[:, 0] / r[:, 3], r[:, 1] / r[:, 3], 1.0 / r[:, 3]
    i0, i1, i2 = (faces[tri, k].astype(np.int64) for k in range(3))
    ax, ay, bx, by, cx, cy = sx[i0], sy[i0], sx[i1], sy[i1], sx[i2], sy[i2]
    area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    al = ((bx - xs) * (cy - ys) - (by - ys) * (cx - xs)) / area
    be = ((cx - xs) * (ay - ys) - (cy - ys) * (ax - xs)) / area
    n0, n1, n2 = al * q[i0], be * q[i1], (1.0 - al - be) * q[i2]
    s = n0 + n1 + n2
    ap, bp = n0 / s, n1 / s
    a = np.asarray(attr, np.float64)[tri]  # [N, 3, C]
    out = ap[:, None] * a[:, 0] + bp[:, None] * a[:, 1] + (1.0 - ap - bp)[:, None] * a[:, 2]
    return (out * G[:, ys, xs].T).sum(1)


def central(f, theta, h):
    """per-pixel Jacobian of f (→ [N]) at theta by central differences with step h * max(1, |theta_k|) → [N, theta.size]"""
    flat = np.asarray(theta, np.float64).ravel()
    J = np.zeros((len(f(flat.reshape(theta.shape))), flat.size))
    for k in range(flat.size):
        d = h * max(1.0, abs(flat[k]))
        p, n = flat.copy(), flat.copy()
        p[k] += d
        n[k] -= d
        J[:, k] = (f(p.reshape(theta.shape)) - f(n.reshape(theta.shape))) / (2 * d)
    return J


def test_gradients_to_vertices_matrix_and_attributes(ctx, monkeypatch):
    """loss = a fixed random linear functional of interpolate_persp(fs, vis, attr, scene_positions(...), clip_q(...)), attr = the
    object-space position and uv of every corner.  verts.grad, mvp.grad and attr.grad against central differences of the float64
    restatement, per element k within
        tol_k = (64 kappa u + 4 gamma_N + 1e-6) A_k,    A_k = sum over the pixels of |d loss_pixel / d theta_k|  (from the restatement)
    — u = 2^-24; fewer than 64 float32 roundings lie between a parameter and a pixel's term (vertex stage 8, the rasteriser's
    barycentrics 12, the rule 10, interpolation 4, their backwards as many again), each relative to an intermediate that is at most
    kappa times the term it feeds, kappa = max over the triangles of (largest |screen coordinate| x longest edge / |doubled area|),
    the cancellation in the edge functions; every element is summed by at most four chains of float atomics (interpolate_grad,
    perspective_grad, position_grad, vertex_grad) of at most N terms each, N the owned pixels: 4 gamma_N, gamma_N = N u / (1 - N u);
    the central differences' own error is (kappa h)^2 <= 1e-6 relative at h = 1e-5 (the restatement is rational, its third
    derivatives are within kappa^2 of the first) and 2^-53 / h in rounding.  None of it is taken from the device's output."""
    pos, faces, m, sf = chain_scene(ctx)
    fs = ctx.frameset([sf])
    T = len(faces)
    vis = visibility(fs)
    v = words(vis)
    tri_map, _ = perspref.owners(v[0], T)
    ys, xs = np.nonzero(tri_map >= 0)
    tri = tri_map[ys, xs]
    N = len(tri)
    assert N > 1500 and len(np.unique(tri)) == T
    rng = np.random.default_rng(17)
    attr_n = np.concatenate([pos[faces.astype(np.int64)], pos[faces.astype(np.int64)][..., :2] * 3.0], -1).astype(np.float32)  # [T, 3, 5]
    G = rng.normal(0, 1, (5, H, W))
    # ---- the device
    verts = dev(pos).requires_grad_(True)
    mvp = dev(m.reshape(1, 1, 16)).requires_grad_(True)
    attr = dev(attr_n).requires_grad_(True)

    def run(fn):
        for t in (verts, mvp, attr):
            t.grad = None
        p = V.scene_positions(fs, {SLOT: verts}, mvp, None)
        out = fn(p)
        (out * dev(G)[None]).sum().backward()
        torch.cuda.synchronize()
        return out.detach(), [t.grad.cpu().numpy().astype(np.float64) for t in (verts, mvp, attr)]
    out, got = run(lambda p: V.interpolate_persp(fs, vis, attr, p, V.clip_q(fs, {SLOT: verts}, mvp)))
    _, geo = run(lambda p: V.interpolate_geo(fs, vis, attr, p))
    # the forward is interpolate over the perspective buffer of the plain calls
    q = V.clip_q(fs, {SLOT: verts.detach()}, mvp.detach())
    assert tuple(q.shape) == (1, T, 3)
    assert torch.equal(out, V.interpolate(fs, V.perspective(fs, vis, q), attr.detach()))
    # ---- the restatement
    f_v = lambda th: pixel_losses(th, m, attr_n, faces, tri, ys, xs, G)  # noqa: E731
    f_m = lambda th: pixel_losses(pos, th, attr_n, faces, tri, ys, xs, G)  # noqa: E731
    f_a = lambda th: pixel_losses(pos, m, th, faces, tri, ys, xs, G)  # noqa: E731
    rows = np.asarray(m, np.float64).reshape(4, 4).T
    r = pos.astype(np.float64) @ rows[:, :3].T + rows[:, 3]
    sxy = (r[:, :2] / r[:, 3:4])[faces.astype(np.int64)]  # [T, 3, 2]
    e1, e2 = sxy[:, 1] - sxy[:, 0], sxy[:, 2] - sxy[:, 0]
    area2 = np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])
    edge = np.max([np.hypot(*e1.T), np.hypot(*e2.T), np.hypot(*(e2 - e1).T)], 0)
    kappa = float((np.abs(sxy).max((1, 2)) * edge / area2).max())
    gamma_n = N * U / (1 - N * U)
    rel = 64 * kappa * U + 4 * gamma_n + 1e-6
    print(f"owned pixels {N}, kappa {kappa:.2f}, relative tolerance {rel:.3e}")
    assert kappa < 50 and rel < 2e-3
    for name, g, g_old, J in (("verts.grad", got[0], geo[0], central(f_v, pos.astype(np.float64), 1e-5)),
                              ("mvp.grad", got[1].reshape(16), geo[1].reshape(16), central(f_m, np.asarray(m, np.float64), 1e-5)),
                              ("attr.grad", got[2], geo[2], central(f_a, attr_n.astype(np.float64), 1e-5))):
        want, A = J.sum(0).reshape(g.shape), np.abs(J).sum(0).reshape(g.shape)
        tol = rel * A + 1e-12
        err = np.abs(g - want)
        print(f"{name}: max |value| {np.abs(want).max():.3e}, max err / tol {(err / tol).max():.3f}; screen-linear chain: max err / tol "
              f"{(np.abs(g_old - want) / tol).max():.1f}")
        assert np.abs(want).max() > 0 and (err <= tol).all(), (name, np.argwhere(err > tol)[:4].tolist(), float((err / tol).max()))
        if name == "verts.grad":  # (the case that cannot pass on the old path)
            assert float((np.abs(g_old - want) / tol).max()) > 100, "the screen-linear chain comes close: the test says nothing"
    # ---- only what needs a gradient is asked for: attr alone launches interpolate_grad, and neither perspective_grad nor position_grad
    import srz
    calls = []
    for name in ("interpolate_grad", "perspective_grad", "position_grad"):
        real = getattr(srz.FrameSet, name)
        monkeypatch.setattr(srz.FrameSet, name, lambda self, *a, _n=name, _r=real, **k: (calls.append(_n), _r(self, *a, **k))[1])
    a2 = dev(attr_n).requires_grad_(True)
    p = V.scene_positions(fs, {SLOT: verts.detach()}, mvp.detach(), None)
    V.interpolate_persp(fs, vis, a2, p, q).sum().backward()
    assert calls == ["interpolate_grad"] and a2.grad is not None and bool((a2.grad != 0).any())
    del calls[:]
    q2 = q.clone().requires_grad_(True)  # q alone: no position_grad
    V.interpolate_persp(fs, vis, attr.detach(), p, q2).sum().backward()
    assert calls == ["interpolate_grad", "perspective_grad"] and bool((q2.grad != 0).any())
    fs.close()


def test_clip_q_refuses_a_slot_drawn_twice(ctx):
    pos, faces, m, sf = chain_scene(ctx)
    m2 = m.copy()
    m2[12] += np.float32(3.0)
    twice = abi.SceneFrame(W, H, (0.0, 0.0, 1.0), np.zeros((0, 2, 3), np.float32),
                           [(SLOT, abi.SHADER_NORMAL, -1, m, IDENT), (SLOT, abi.SHADER_NORMAL, -1, m2, IDENT)], 1.0, 0.0, abi.FUSED_CLEAR)
    fs = ctx.frameset([twice])
    with pytest.raises(ValueError, match="draws mesh slot"):
        V.clip_q(fs, {SLOT: dev(pos)}, dev(np.stack([m, m2])[None]))
    fs.close()
    fs = ctx.frameset([sf])
    q = V.clip_q(fs, {SLOT: dev(pos)}, dev(m.reshape(1, 1, 16))).cpu().numpy()
    m32, p32 = np.asarray(m, np.float32), pos.astype(np.float32)
    r3 = (m32[3] * p32[:, 0] + m32[7] * p32[:, 1]) + (m32[11] * p32[:, 2] + m32[15])
    assert np.array_equal(q[0], (np.float32(1) / r3)[faces.astype(np.int64)])
    fs.close()


def test_mip_levels_follow_the_foreshortening(ctx, tmp_path):
    """a ground quad receding along x: the derivative planes of interpolate_deriv_persp are the reference's bit for bit, so
    texture_mip over them is tests/mipref.py's output on the reference's planes, bit for bit; and the levels they select differ from
    the ones the screen-linear constants select over much of the quad"""
    f, obj, q, _, faces = perspref.quad_scene()
    T = len(faces)
    fs = ctx.frameset([f])
    vis = visibility(fs)
    v = words(vis)
    own = perspref.owners(v[0], T)[0] >= 0
    uv_attr = (obj[..., :2] * 6.0).astype(np.float32)  # [T, 3, 2]: the texture repeats six times across the quad
    pos9 = f.tris[0]["pos"].reshape(-1, 9)
    qd, ad = dev(q), dev(uv_attr)
    d = V.interpolate_deriv_persp(fs, vis, ad, qd)
    want_d = perspref.deriv(tmp_path, q, pos9, uv_attr, T, v[0])
    same(words(d)[0], want_d, "derivative planes")
    pv = V.perspective(fs, vis, qd)
    same(words(pv)[0], perspref.forward(tmp_path, q, T, v[0]), "perspective buffer")
    uv = V.interpolate(fs, pv, ad)
    tex = mipref.make_tex(5, 64, 64, 3)
    n_levels = mipref.levels(tmp_path, 64, 64)
    out = V.texture_mip(fs, vis, dev(tex), uv, d, wrap=True)
    torch.cuda.synchronize()
    want = mipref.forward(tmp_path, tex, mipref.build(tmp_path, tex, n_levels), abi.TEX_WRAP, n_levels, T, v[0, 1], uv.cpu().numpy()[0], want_d)
    same(words(out)[0], want, "texture_mip over the perspective planes")
    l_p, f_p = mipref.lod(tmp_path, (64, 64), n_levels, want_d)
    lin = V.interpolate_deriv(fs, vis, ad).cpu().numpy()[0]
    l_s, f_s = mipref.lod(tmp_path, (64, 64), n_levels, lin)
    lam_p, lam_s = (l_p + f_p)[own], (l_s + f_s)[own]
    print(f"levels under the rule {lam_p.min():.2f} .. {lam_p.max():.2f}, under the screen-linear constants {lam_s.min():.2f} .. {lam_s.max():.2f}")
    assert lam_p.max() - lam_p.min() > 1.0, "the quad does not recede"
    assert (np.abs(lam_p - lam_s) > 0.25).mean() > 0.3
    fs.close()
