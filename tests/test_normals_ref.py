"""not-gpu: the reference of the vertex normals and the per-vertex attributes (tests/normalsref.py, tests/normals_ref.c) is itself held
to float64 evaluations: the normals to a numpy restatement and their backward to torch autograd on the CPU, both under rounding bounds
DERIVED in normalsref (gamma_n * sum |term| carried through the rule, not measured); the corner attributes to numpy fancy indexing bit
for bit and their gradient to a float64 scatter under gamma_n * sum |term|."""
import numpy as np
import pytest

import normalsref as nr
import vgkit

MESHES = {"fan": lambda: vgkit.fan(70, 2), "grid257": lambda: vgkit.grid(16, 16, 3, extra=1), "soup": lambda: nr.soup(1)}


@pytest.mark.parametrize("name", list(MESHES))
def test_normals_against_float64(tmp_path, name):
    pos, faces = MESHES[name]()
    L = nr.Lists(tmp_path, faces, len(pos))
    got, mask = nr.normals(tmp_path, L, pos, want_mask=True)
    e = nr.normals64(L, pos)
    assert np.array_equal(mask, e.len > 0) and mask.sum() >= len(pos) - 1 and not got[~mask].view(np.uint32).any()
    bound = nr.normals_bound(e)[mask]
    err = np.abs(got[mask].astype(np.float64) - e.n[mask]).max(1)
    print(f"{name}: {int(mask.sum())} normalised of {len(pos)}, max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}, "
          f"median bound {np.median(bound):.3e}")
    assert (err <= bound).all(), np.argwhere(err > bound)[:4].tolist()
    assert np.median(bound) < 1e-5, "the bound says nothing"
    # unit length: n = S r with r within gamma_6 of 1 / |S| (normalsref.normals_bound), one more rounding per component
    length = np.linalg.norm(got[mask].astype(np.float64), axis=1)
    assert (np.abs(length - 1.0) <= nr.gamma(7)).all(), np.abs(length - 1.0).max()


def test_normals_of_the_degenerate_cases_are_exact_zeros(tmp_path):
    pos, faces, ok = nr.edge_mesh()
    L = nr.Lists(tmp_path, faces, len(pos))
    got, mask = nr.normals(tmp_path, L, pos, want_mask=True)
    assert np.array_equal(mask, ok)
    assert not got[~ok].view(np.uint32).any(), "a vertex that is not normalised is not (+0, +0, +0)"
    assert np.isfinite(got).all() and (np.abs(np.linalg.norm(got[ok].astype(np.float64), axis=1) - 1.0) <= nr.gamma(7)).all()
    # a slot without faces, and two sets at once
    none = nr.Lists(tmp_path, np.zeros((0, 3), np.uint32), 5)
    assert not nr.normals(tmp_path, none, np.ones((2, 5, 3), np.float32)).view(np.uint32).any()
    # its backward: nothing passes through a vertex that is not normalised; gS = 0 there, and the only non-finite gpos belongs to the
    # face with the NaN position
    g = np.random.default_rng(131).uniform(-1, 1, pos.shape).astype(np.float32)
    gp = nr.normals_grad(tmp_path, L, pos, g)
    assert np.isfinite(gp[[0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 14, 15, 16, 17, 18]]).all() and not gp[3:8].any() and not gp[13:19].any()
    assert gp[0:3].any()


@pytest.mark.parametrize("name", list(MESHES))
def test_normals_grad_against_torch_autograd(tmp_path, name):
    import torch
    pos, faces = MESHES[name]()
    L = nr.Lists(tmp_path, faces, len(pos))
    g = np.random.default_rng([len(name), 137]).uniform(-1, 1, pos.shape).astype(np.float32)
    got = nr.normals_grad(tmp_path, L, pos, g)
    p = torch.tensor(pos.astype(np.float64), requires_grad=True)
    f = torch.as_tensor(L.f)
    N = torch.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]], dim=1)
    S = torch.zeros_like(p)
    for k in range(3):
        S = S.index_add(0, f[:, k], N)
    ln = S.norm(dim=1, keepdim=True)
    live = ln > 0
    n = torch.where(live, S / torch.where(live, ln, torch.ones_like(ln)), torch.zeros_like(S))
    (n * torch.as_tensor(g.astype(np.float64))).sum().backward()
    want = p.grad.numpy()
    bound = nr.grad_bound(nr.normals64(L, pos), g)
    err = np.abs(got.astype(np.float64) - want)
    fin = np.isfinite(bound)
    ratio = err[fin & (bound > 0)] / bound[fin & (bound > 0)]
    print(f"{name}: max |gpos| {np.abs(want).max():.3e}, max err {err.max():.3e}, max err / bound {ratio.max():.3f}, "
          f"median bound {np.median(bound[fin]):.3e}, finite bounds {int(fin.sum())} of {fin.size}")
    assert fin.mean() > 0.9 and (err[fin] <= bound[fin]).all(), np.argwhere(fin & (err > bound))[:4].tolist()
    assert np.median(bound[fin]) < 1e-4 * np.abs(want).max(), "the bound says nothing"
    # two sets in one call are the two calls
    two = nr.normals_grad(tmp_path, L, np.stack([pos, pos[::-1]]), np.stack([g, g]))
    assert np.array_equal(two[0].view(np.uint32), got.view(np.uint32))


def scene_frames(nf_a, nf_b):
    """three frames, (slot, face count) per draw: slot 3 drawn twice around slot 5; slot 5 alone; slot 5, then slot 3"""
    return [[(3, nf_a), (5, nf_b), (3, nf_a)], [(5, nf_b)], [(5, nf_b), (3, nf_a)]]


@pytest.mark.parametrize("n_ch", [1, 3, 64])
def test_corner_attributes_against_numpy(tmp_path, n_ch):
    rng = np.random.default_rng([n_ch, 139])
    (pa, fa), (pb, fb) = vgkit.fan(70, 2), vgkit.grid(3, 3, 9)
    A, B = nr.Lists(tmp_path, fa, len(pa)), nr.Lists(tmp_path, fb, len(pb))
    frames = scene_frames(len(fa), len(fb))
    T = 2 * len(fa) + len(fb) + 2
    for shared in (True, False):
        attr = rng.uniform(-1, 1, ((len(pa), n_ch) if shared else (3, len(pa), n_ch))).astype(np.float32)
        out = nr.corner_attr(tmp_path, frames, {3: A, 5: B}, {3: attr}, np.full((3, T, 3, n_ch), -7.25, np.float32))
        want = np.full((3, T, 3, n_ch), -7.25, np.float32)
        for f, draws in enumerate(frames):
            first = 0
            for slot, nf in draws:
                if slot == 3:
                    want[f, first:first + nf] = (attr if shared else attr[f])[np.asarray(fa, np.int64)]
                first += nf
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    # the gradient: a float64 scatter; every element is a sum of n float32 terms rounded once per add — gamma_n * sum |term|
    gout = rng.uniform(-1, 1, (3, T, 3, n_ch)).astype(np.float32)
    got = nr.corner_attr_grad(tmp_path, frames, A, 3, gout)
    want, mag, cnt = np.zeros(got.shape), np.zeros(got.shape), np.zeros(got.shape[:2])
    idx = np.asarray(fa, np.int64).reshape(-1)
    for f, draws in enumerate(frames):
        first = 0
        for slot, nf in draws:
            if slot == 3:
                rows = gout[f, first:first + nf].reshape(-1, n_ch).astype(np.float64)
                np.add.at(want[f], idx, rows), np.add.at(mag[f], idx, np.abs(rows)), np.add.at(cnt[f], idx, 1.0)
            first += nf
    bound = nr.gamma(cnt)[:, :, None] * mag
    err = np.abs(got.astype(np.float64) - want)
    print(f"n_ch {n_ch}: max n {int(cnt.max())}, max err {err.max():.3e}, max bound {bound.max():.3e}")
    assert (err <= bound).all() and not got[1].view(np.uint32).any() and cnt.max() == 140
    one = np.broadcast_to((cnt == 1)[:, :, None], got.shape)
    assert one.any() and np.array_equal(got[one], want[one].astype(np.float32))
