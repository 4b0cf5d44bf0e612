"""-m gpu: fitting a pose and a mesh under ONE live sceneset.  chainref.pose_scene's flat-coloured triangles are a mesh (vgkit.fit_model);
the target is the chain's image with the model translated by chainref.POSE_OFFSET through ndc_mvp.  Every step is srz_sceneset_update
(the matrix descent) or srz_mesh_update (the vertex descent), one visibility render, the autograd chain from scene_positions to the
loss 0.5 * sum (out - target)^2, and one backward: the set is never rebuilt.  The thresholds are the CPU references' own numbers for
the same loops (vgkit.FIT_*, held on the CPU by tests/test_vertex_grad_ref.py), not the device's."""
import numpy as np
import pytest
import torch

import chainref as cr
import vgkit
from srz import abi
from srz import visibility as V
from support import ctx, place, sceneset_update, vertex_stage, visibility  # noqa: F401

pytestmark = pytest.mark.gpu

IDENT = np.eye(4, dtype=np.float32).reshape(16)
UNIT = place(1.0, 1.0, 0.0, 0.0)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def scene_frame(p):
    return abi.SceneFrame(cr.W, cr.H, (0.0, 0.0, 1.0), np.zeros((0, 2, 3), np.float32),
                          [(0, abi.SHADER_NORMAL, -1, vgkit.fit_matrix(p), IDENT), (1, abi.SHADER_NORMAL, -1, UNIT, IDENT)], 1.0, 0.0, abi.FUSED_CLEAR)


class Fit:
    """the live set of one seed: slot 0 the model, slot 1 the backdrop"""

    def __init__(self, ctx, seed):
        self.ctx = ctx
        self.pos0, self.faces, attr = vgkit.fit_model(seed)
        self.attr = dev(attr)
        ctx.mesh_upload(0, vgkit.verts8(self.pos0), self.faces)
        ctx.mesh_upload(1, vgkit.verts8(vgkit.backdrop_mesh()[0]), vgkit.backdrop_mesh()[1])
        self.fs = ctx.frameset([scene_frame((0.0, 0.0))])
        self.handle = self.fs.h.value
        self.target = self.image(self.pos0, vgkit.FIT_W * np.float32(cr.POSE_OFFSET))[0].detach()

    def image(self, pos, p, silhouette=True):
        """the set moved to vertex positions pos and translation entries p — one srz_mesh_update, one srz_sceneset_update —, its
        visibility render and the chain -> (out [1, 3, rows, W], the verts and mvp leaves)"""
        V.mesh_update(self.ctx, 0, dev(vgkit.verts8(pos)))
        torch.cuda.synchronize()
        sceneset_update(self.ctx, self.fs, [scene_frame(p)])
        vis = visibility(self.fs)
        verts = dev(pos).requires_grad_(True)
        mvp = dev(np.stack([vgkit.fit_matrix(p), UNIT])[None]).requires_grad_(True)
        scr = V.scene_positions(self.fs, {0: verts}, mvp)
        out = V.antialias(self.fs, vis, V.interpolate_geo(self.fs, vis, self.attr, scr), scr if silhouette else None)
        return out, verts, mvp

    def grad_of(self, silhouette=True):
        def f(pos, p):
            out, verts, mvp = self.image(pos, p, silhouette)
            (0.5 * (out - self.target).square()).sum().backward()
            torch.cuda.synchronize()
            assert self.fs.h.value == self.handle  # (the one set made at the start)
            return verts.grad.cpu().numpy(), mvp.grad[0, 0].cpu().numpy().tolist() + [0.0, 0.0]
        return f

    def close(self):
        self.fs.close()


@pytest.mark.parametrize("kind", ["matrix", "verts"])
@pytest.mark.parametrize("seed", cr.POSE_SEEDS)
def test_fit_under_a_live_set(ctx, tmp_path, orc, seed, kind):
    """plain descent for chainref.POSE_STEPS steps on the two translation entries of the model's matrix, and on its vertices' x and y
    through srz_mesh_update.  With the full gradient the final error is below twice the CPU chain's (vgkit.FIT_MATRIX_BOUND; twice
    vgkit.FIT_VERTS_FINAL[seed]); the interior term alone — zero for flat colours, so gverts and gdraw are zeros — leaves it above 0.95
    of the start.  The target frame is the CPU chain's bit for bit."""
    fit = Fit(ctx, seed)
    t = vertex_stage(vgkit.verts8(fit.pos0), fit.faces, vgkit.fit_matrix(vgkit.FIT_W * np.float32(cr.POSE_OFFSET)), IDENT, 1.0, 0.0)
    P = np.concatenate([t["pos"], cr.BACKDROP[None]]).astype(np.float32)
    want = cr.loss_and_grad(tmp_path, orc, P, fit.attr.cpu().numpy(), np.zeros((3, cr.H, cr.W), np.float32), want_grad=False).out
    assert np.array_equal(fit.target[0].cpu().numpy().view(np.uint32), want.view(np.uint32)), "the target frame is not the CPU chain's"
    full = vgkit.fit_descend(kind, fit.grad_of(True), fit.pos0)
    inner = vgkit.fit_descend(kind, fit.grad_of(False), fit.pos0)
    recorded = vgkit.FIT_MATRIX_FINAL[seed] if kind == "matrix" else vgkit.FIT_VERTS_FINAL[seed]
    bound = vgkit.FIT_MATRIX_BOUND if kind == "matrix" else 2 * vgkit.FIT_VERTS_FINAL[seed]
    print(f"seed {seed} {kind}: error 1.0000 -> {full[-1]:.4f} on the device (CPU chain {recorded:.4f}, bound {bound:.4f}); interior term alone "
          f"-> {inner[-1]:.4f}")
    fit.close()
    assert inner[-1] > 0.95
    assert full[-1] < bound
