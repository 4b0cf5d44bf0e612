"""-m gpu: srz.visibility.background under autograd — the Function's gradients are the plain call's, needs_input_grad selects the
backward build, the chain antialias(fs, vis, shaded + background(fs, vis, env, view_rays(S)), pos) backpropagates to the environment,
the camera and the positions — and the pixel convention of view_rays pinned against the rasteriser."""
import numpy as np
import pytest
import torch

import backgroundref as br
import vgkit
from srz import abi
from srz import visibility as V
from support import ctx, scene_pair, visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

W = H = 64
SLOT = 2
EYE, CENTER, UP, FOVY = (0.4, -0.3, -2.5), (0.1, 0.2, 0.5), (0.05, 1.0, 0.1), 0.9


def dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


def scene(ctx):
    """one frame: a quad PARALLEL TO THE IMAGE PLANE, three units in front of the reference's camera (lookAtLH, perspectiveLH_NO), which
    covers the middle of the frame → (fs, vis, own [H, W], S [4, 4] float64, the quad's world vertices [4, 3], its triangle count)"""
    S = br.camera_matrix(EYE, CENTER, UP, FOVY, W, H)
    eye, f = np.float64(EYE), np.float64(CENTER) - np.float64(EYE)
    f /= np.linalg.norm(f)
    s = np.cross(np.float64(UP), f)
    s /= np.linalg.norm(s)
    u = np.cross(f, s)
    c = eye + 3.0 * f
    posn = np.float32([c - s - 0.8 * u, c + s - 0.8 * u, c + s + 0.8 * u, c - s + 0.8 * u])
    mvp = np.ascontiguousarray(S.T, np.float32).reshape(16)  # column-major: the model matrix is the identity
    faces = vgkit.oriented(posn, [(0, 1, 2), (0, 2, 3)], mvp)
    ident = np.eye(4, dtype=np.float32).reshape(16)
    sf, fr = scene_pair([(vgkit.verts8(posn), faces, abi.SHADER_NORMAL, -1, mvp, ident)], W, H, (0.0, 0.0, 1.0), [], 1.75, 0.5, ctx=ctx, slots=[SLOT])
    fs = ctx.frameset([sf])
    vis = visibility(fs)
    own = ((words(vis)[0, 1] & 0x7fffffff) - np.uint32(1)) < fr.n_tris
    assert 600 < own.sum() < 3000 and not own[0].any() and not own[:, 0].any()
    return fs, vis, own, S, posn, fr.n_tris


def test_the_function_is_the_plain_call_and_asks_for_what_is_needed(ctx, tmp_path, monkeypatch):
    import srz
    fs, vis, own, S, _, T = scene(ctx)
    calls = []
    real = srz.FrameSet.background_grad
    monkeypatch.setattr(srz.FrameSet, "background_grad", lambda self, *a, **k: (calls.append(a), real(self, *a, **k))[1])
    rng = np.random.default_rng(2)
    env, rays = dev(rng.uniform(0.1, 2.0, (6, 8, 8, 3))), V.view_rays(dev(S, np.float64))
    assert rays.shape == (1, 9) and rays.is_cuda and rays.dtype == torch.float32
    g = dev(rng.normal(0, 1, (1, 3, H, W)))
    v = words(vis)
    for where in ("nobody", "all"):
        wv = br.ALL if where == "all" else br.NOBODY
        want = br.forward(tmp_path, env.cpu().numpy(), T, v[0, 1], rays.cpu().numpy(), wv)
        acc = br.Grad((6, 8, 8, 3))
        row = br.grad(tmp_path, env.cpu().numpy(), T, v[0, 1], rays.cpu().numpy(), g.cpu().numpy()[0], acc, wv)[0]
        et, rt = env.clone().requires_grad_(True), rays.clone().requires_grad_(True)
        out = V.background(fs, vis, et, rt, where)
        assert np.array_equal(words(out.detach())[0], want.view(np.uint32))
        n0 = len(calls)
        (out * g).sum().backward()
        assert len(calls) == n0 + 1 and all(bool(p) for p in calls[-1][9:12])  # one launch: d_gtex, d_gray and d_work
        gtex, gray = V.background_grad(fs, vis, env, rays, g, where)
        assert torch.equal(rt.grad, gray) and np.array_equal(words(gray)[0], row.view(np.uint32))
        # cube.grad is a sum of float atomics: each launch lies within Grad.bound of the exact sums, so two lie within twice that
        for t in (et.grad, gtex):
            assert (np.abs(t.cpu().numpy().astype(np.float64) - acc.gtex) <= acc.bound()).all()
        # only one input needs a gradient: the launch asks for that output alone
        et = env.clone().requires_grad_(True)
        V.background(fs, vis, et, rays, where).sum().backward()
        assert [bool(p) for p in calls[-1][9:12]] == [True, False, False]
        rt = rays.clone().requires_grad_(True)
        (V.background(fs, vis, env, rt, where) * g).sum().backward()
        assert [bool(p) for p in calls[-1][9:12]] == [False, True, True] and torch.equal(rt.grad, gray)
        n0 = len(calls)
        assert not V.background(fs, vis, env, rays, where).requires_grad and len(calls) == n0
    # where="all" does not read the buffer: None will do
    assert torch.equal(V.background(fs, None, env, rays, "all"), V.background(fs, vis, env, rays, "all"))
    fs.close()


def test_the_chain_backpropagates_to_the_environment_the_camera_and_the_positions(ctx):
    fs, vis, own, S, posn, T = scene(ctx)
    rng = np.random.default_rng(3)
    env = dev(rng.uniform(0.1, 2.0, (6, 8, 8, 3))).requires_grad_(True)
    St = dev(S, np.float64).requires_grad_(True)
    pos = V.positions(fs, T).requires_grad_(True)
    attr = dev(rng.uniform(0, 1, (T, 3, 3)))
    target = dev(rng.uniform(0, 1, (1, 3, H, W)))
    shaded = V.interpolate_geo(fs, vis, attr, pos)
    bg = V.background(fs, vis, env, V.view_rays(St))
    m = torch.as_tensor(own).cuda()
    assert not bg[0][:, m].any() and not shaded[0][:, ~m].any() and bool((bg[0][:, ~m] > 0).all())
    img = V.antialias(fs, vis, shaded + bg, pos)
    assert not torch.equal(img, shaded + bg)  # the outline blends with the backdrop
    (img - target).square().sum().backward()
    torch.cuda.synchronize()
    for name, t in (("env", env), ("S", St), ("pos", pos)):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any()), name
    assert St.grad.dtype == torch.float64 and bool((St.grad[[0, 1, 3], :3] != 0).all()) and not St.grad[2].any() and not St.grad[:, 3].any()
    # the silhouette term sees the backdrop: against a black background the positions' gradient is another one
    pos0 = V.positions(fs, T).requires_grad_(True)
    (V.antialias(fs, vis, V.interpolate_geo(fs, vis, attr, pos0), pos0) - target).square().sum().backward()
    assert not torch.allclose(pos0.grad, pos.grad)
    fs.close()


def test_view_rays_pixel_convention_against_the_rasteriser(ctx):
    """the quad's world positions, interpolated at the pixels the rasteriser gave it, against the rays view_rays puts through the same
    integer pixels: the angle to P - eye stays below 1e-3 rad.  A pixel is 2 tan(FOVY / 2) / 64 = 1.5e-2 rad wide at the frame's
    centre, so a half-pixel offset or a flipped axis gives at least 7e-3 (and 1.5e-2 for a whole pixel); float32 interpolation over
    positions of magnitude 3 gives about 1e-5.  The quad is parallel to the image plane, so screen-linear barycentrics are the
    perspective-correct ones."""
    fs, vis, own, S, posn, T = scene(ctx)
    P = V.interpolate(fs, vis, V.corner_attr(fs, {SLOT: dev(posn)}, pos_tris=T))[0].cpu().numpy().astype(np.float64)  # [3, H, W]
    r = V.view_rays(torch.as_tensor(S)).numpy()[0].astype(np.float64)
    ys, xs = np.nonzero(own)
    d = r[0:3] + xs[:, None] * r[3:6] + ys[:, None] * r[6:9]
    b = P[:, own].T - np.float64(EYE)
    ang = np.arctan2(np.linalg.norm(np.cross(d, b), axis=1), (d * b).sum(1))
    print("pixel convention: max angle", ang.max(), "over", len(ang), "pixels")
    assert ang.max() < 1e-3
    half = r[0:3] + (xs[:, None] + 0.5) * r[3:6] + (ys[:, None] + 0.5) * r[6:9]
    flip = r[0:3] + xs[:, None] * r[3:6] + (H - 1 - ys[:, None]) * r[6:9]
    for other in (half, flip):
        a = np.arctan2(np.linalg.norm(np.cross(other, b), axis=1), (other * b).sum(1))
        assert np.median(a) > 7e-3  # (the threshold tells the conventions apart)
    fs.close()
