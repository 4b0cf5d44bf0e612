"""What srz.visibility refuses on the host, and in which words: ONE table, run without a device by tests/test_visibility_refusals.py
(the rows marked host=True, on meta tensors and a stub set) and whole by tests/test_gpu_visibility_refusals.py (tests/
test_gpu_light_refusals.py's scheme, one layer up).  A row is one call of a public function of srz.visibility: VALID's arguments of
that function — a call the function accepts — with the row's `fault` in their place, so the call has exactly one fault; it must raise
`exc` with exactly `text`.  Nothing reaches a kernel: every refusal is raised before a pointer leaves Python.

    R(fn, fault, exc, text, host, was)
      host  the row needs no device: a refusal that looks at no tensor, or the first tensor clause of its function (a meta tensor
            has the shape and dtype asked about; whatever comes after the first clause that names CUDA is out of its reach)
      was   None: the text is the one the layer has always had, pinned byte for byte.  Otherwise the row is a refusal that was
            missing before the checks were given one definition, and `was` says what the call did then: "AttributeError" (None
            where a tensor is required; depth, which slices its vis, "TypeError"), or "unchecked" — the tensor's address
            went to the library as it was, a host address or a buffer of another size; such a call was never made against a device, here or anywhere.

Not a test module: no test imports another, both import this."""
import collections
import traceback
import types

import numpy as np
import torch

from srz import abi
from srz import visibility as V

W = H = 64      # the plain set: two frames of 64 x 64 with N_TRIS triangles each (the refusal kits' set)
N_TRIS = 24
SLOT, N_VERTS, N_FACES = 3, 12, 12  # the scenesets' one mesh: vgkit.grid(3, 4, .)
FS, SFS, SFS2, CTX, VIS, VERTS8 = "<fs>", "<sceneset>", "<sceneset that draws the slot twice>", "<ctx>", "<vis>", "<verts8>"


class T:
    """a tensor of zeros the row is given, on the kit's device ("meta" without one) unless `dev` names another; strided: a
    non-contiguous view of that shape"""

    def __init__(self, *shape, dtype=torch.float32, dev=None, strided=False):
        self.shape, self.dtype, self.dev, self.strided = shape, dtype, dev, strided

    def make(self, device):
        if self.strided:
            return torch.zeros(*self.shape[:-1], 2 * self.shape[-1], dtype=self.dtype, device=self.dev or device)[..., ::2]
        return torch.zeros(*self.shape, dtype=self.dtype, device=self.dev or device)

    def __repr__(self):
        return "T" + repr(self.shape) + "".join(f",{k}={v}" for k, v in (("dtype", self.dtype), ("dev", self.dev), ("strided", self.strided))
                                                if v not in (torch.float32, None, False))


def P(n, **kw):
    """n planes of the set"""
    return T(2, n, H, W, **kw)


R = collections.namedtuple("R", "fn fault exc text host was", defaults=(False, None))

ATTR, POS, Q, CUBE, TEX = T(N_TRIS, 3, 5), T(2, N_TRIS, 3, 3), T(N_TRIS, 3), T(6, 4, 4, 3), T(8, 8, 3)
LIGHTS, V3 = T(3, 6), T(3)
# function -> the arguments of a call it accepts (keywords of its signature)
VALID = {
    "decode": dict(out=P(4)),
    "peel": dict(fs=FS, prev=VIS),
    "layers": dict(fs=FS, n=2),
    "composite": dict(colors=[P(3)], alphas=[P(1)]),
    "composite_layers": dict(fs=FS, layers=[VIS, VIS], colors=[P(3), P(3)], alphas=[P(1), 0.5], background=P(3)),
    "composite_grad": dict(fs=FS, layers=[VIS, VIS], colors=[P(3), P(3)], alphas=[P(1), 0.5], gout=P(3), background=P(3)),
    "gbuffer_planes": dict(what=abi.GB_ALL),
    "gbuffer_decode": dict(buf=P(9), what=abi.GB_ALL),
    "motion_planes": dict(what=abi.MV_ALL),
    "motion_decode": dict(buf=P(5), what=abi.MV_ALL),
    "interpolate": dict(fs=FS, vis=VIS, attr=ATTR),
    "interpolate_bary_grad": dict(fs=FS, vis=VIS, attr=ATTR, gout=P(5)),
    "position_grad": dict(fs=FS, vis=VIS, gbary=P(2), gz=P(1)),
    "interpolate_geo": dict(fs=FS, vis=VIS, attr=ATTR, pos=POS),
    "depth": dict(fs=FS, vis=VIS, pos=POS),
    "antialias_grad": dict(fs=FS, vis=VIS, color=P(3), gout=P(3)),
    "antialias": dict(fs=FS, vis=VIS, color=P(3), pos=POS),
    "texture_grad": dict(fs=FS, vis=VIS, tex=TEX, uv=P(2), gout=P(3)),
    "texture": dict(fs=FS, vis=VIS, tex=TEX, uv=P(2)),
    "texture_cube_grad": dict(fs=FS, vis=VIS, cube=CUBE, dirs=P(3), gout=P(3)),
    "texture_cube": dict(fs=FS, vis=VIS, cube=CUBE, dirs=P(3)),
    "view_rays": dict(screen_from_world=T(4, 4)),
    "background_grad": dict(fs=FS, vis=VIS, cube=CUBE, rays=T(1, 9), gout=P(3)),
    "background": dict(fs=FS, vis=VIS, cube=CUBE, rays=T(1, 9)),
    "shadow_grad": dict(fs=FS, vis=VIS, map=T(16, 16), sc=P(3), gout=P(1), bias=0.0, width=1.0),
    "shadow": dict(fs=FS, vis=VIS, map=T(16, 16), sc=P(3), bias=0.0, width=1.0),
    "light_params": dict(fs=FS, lights=LIGHTS, eye=V3, ka=V3, ks=V3),
    "light_grad": dict(fs=FS, vis=VIS, nrm=P(3), pos=P(3), kd=P(3), par=T(1, 27), p=5, gout=P(3)),
    "light": dict(fs=FS, vis=VIS, nrm=P(3), pos=P(3), kd=P(3), lights=LIGHTS, eye=V3, ka=V3, ks=V3, p=5),
    "microfacet_params": dict(fs=FS, lights=LIGHTS, eye=V3, amb=V3),
    "microfacet_grad": dict(fs=FS, vis=VIS, nrm=P(3), pos=P(3), base=P(3), mat=P(2), par=T(1, 24), gout=P(3)),
    "microfacet": dict(fs=FS, vis=VIS, nrm=P(3), pos=P(3), base=P(3), mat=P(2), lights=LIGHTS, eye=V3, amb=V3),
    "reflect_grad": dict(fs=FS, vis=VIS, nrm=P(3), pos=P(3), eye=V3, gout=P(4)),
    "reflect": dict(fs=FS, vis=VIS, nrm=P(3), pos=P(3), eye=V3),
    "brdf_table": dict(ctx_or_fs=FS, n=8, m=4),
    "ibl_grad": dict(fs=FS, vis=VIS, base=P(3), mat=P(2), nv=P(1), irr=P(3), spec=P(3), tab=T(8, 8, 2), gout=P(3)),
    "ibl": dict(fs=FS, vis=VIS, base=P(3), mat=P(2), nv=P(1), irr=P(3), spec=P(3), tab=T(8, 8, 2)),
    "normal_map_grad": dict(fs=FS, vis=VIS, nrm=P(3), tan=P(4), m=P(3), gout=P(3)),
    "normal_map": dict(fs=FS, vis=VIS, nrm=P(3), tan=P(4), m=P(3)),
    "interpolate_deriv": dict(fs=FS, vis=VIS, attr=T(N_TRIS, 3, 2)),
    "mip_build": dict(ctx_or_fs=FS, tex=TEX),
    "mip_views": dict(mip=T(63), tex_shape=(8, 8, 3)),
    "texture_mip_grad": dict(fs=FS, vis=VIS, tex=TEX, uv=P(2), uvd=P(4), gout=P(3)),
    "texture_mip": dict(fs=FS, vis=VIS, tex=TEX, uv=P(2), uvd=P(4)),
    "cube_mip_build": dict(ctx_or_fs=FS, cube=CUBE),
    "cube_mip_views": dict(mip=T(90), cube_shape=(6, 4, 4, 3)),
    "cube_level": dict(fs=FS, vis=VIS, dirs=P(3), dird=P(6), n=4, n_levels=3),
    "texture_cube_mip_grad": dict(fs=FS, vis=VIS, cube=CUBE, dirs=P(3), lam=P(1), gout=P(3)),
    "texture_cube_mip": dict(fs=FS, vis=VIS, cube=CUBE, dirs=P(3), lam=P(1)),
    "cube_prefilter": dict(ctx_or_fs=FS, cube=CUBE, n_out=4, kind=abi.PREFILTER_COSINE),
    "cube_prefilter_grad": dict(ctx_or_fs=FS, gdst=CUBE, den=T(6, 4, 4), n_src=4, kind=abi.PREFILTER_COSINE),
    "cube_prefilter_pyramid": dict(ctx_or_fs=FS, cube=CUBE, roughness=(0.5,)),
    "vertex_grad": dict(fs=SFS, mesh_id=SLOT, gpos=T(2, N_FACES, 3, 3)),
    "mesh_update": dict(ctx=CTX, mesh_id=SLOT, verts8=VERTS8),
    "scene_positions": dict(fs=SFS, meshes={SLOT: T(N_VERTS, 3)}, mvp=T(2, 1, 16), zmap=T(2, 1, 2)),
    "mesh_normals": dict(ctx=CTX, slot=SLOT, pos=T(N_VERTS, 3)),
    "mesh_tangents": dict(ctx=CTX, slot=SLOT, pos=T(N_VERTS, 3), uv=T(N_VERTS, 2)),
    "corner_attr": dict(fs=SFS, attrs={SLOT: T(N_VERTS, 3)}),
    "perspective": dict(fs=FS, vis=VIS, q=Q),
    "perspective_grad": dict(fs=FS, vis=VIS, q=Q, gbary_p=P(2)),
    "interpolate_persp": dict(fs=FS, vis=VIS, attr=ATTR, pos=POS, q=Q),
    "clip_q": dict(fs=SFS, meshes={SLOT: T(N_VERTS, 3)}, mvp=T(2, 1, 16)),
    "interpolate_deriv_persp": dict(fs=FS, vis=VIS, attr=T(N_TRIS, 3, 2), q=Q),
}

E = ValueError
NARROW = "(2, 3, 64, 32) torch.float32"       # what a three-plane tensor of half the width is said to be
VIS_WANT = ": expected a contiguous CUDA float32 tensor (2, 4, 64, 64), got "
PLANES = "must be a CUDA float32 tensor (2, {}, 64, 64), got "
P1, P2, P3, P4 = (PLANES.format(n) for n in (1, 2, 3, 4))
POS_WANT = ": pos must be float32 [n_frames, T, 3, 3], got (2, 24, 3, 2) torch.float32"
ATTR_WANT = "interpolate: attr must be a CUDA float32 tensor [T, 3, C] or [n_frames, T, 3, C], got "
TEX_WANT = "texture: tex must be a CUDA float32 tensor [H, W, C] or [n_frames, H, W, C], got "
CUBE_WANT = "texture_cube: cube must be a CUDA float32 tensor [6, N, N, C] or [n_frames, 6, N, N, C], got "
MAP_WANT = "shadow: map must be a float32 tensor [H, W], [n_frames, H, W] or [n_frames, 1, H, W], got "
A_CUBE = ": a cube is a CUDA float32 tensor [6, N, N, C] or [frames, 6, N, N, C], got (5, 4, 4, 3) torch.float32"
BAD_POS, BAD_CUBE = T(2, N_TRIS, 3, 2), T(5, 4, 4, 3)

ROWS = [
    # ---------------------------------------------------------------- the buffer itself, layers, compositing
    R("decode", dict(out=P(3)), E, "decode: expected a [..., 4, rows, W] tensor of 4-byte words, got (2, 3, 64, 64) torch.float32", True),
    R("decode", dict(out=T(2, 4, H, W, dtype=torch.float64)), E,
      "decode: expected a [..., 4, rows, W] tensor of 4-byte words, got (2, 4, 64, 64) torch.float64", True),
    R("peel", dict(prev=T(2, 4, H, 32)), E, "peel: prev" + VIS_WANT + "(2, 4, 64, 32) torch.float32", True),
    R("peel", dict(prev=P(4, dtype=torch.int32)), E, "peel: prev" + VIS_WANT + "(2, 4, 64, 64) torch.int32", True),
    R("peel", dict(prev=P(4, dev="cpu")), E, "peel: prev" + VIS_WANT + "(2, 4, 64, 64) torch.float32", True),
    R("peel", dict(prev=P(4, strided=True)), E, "peel: prev" + VIS_WANT + "(2, 4, 64, 64) torch.float32", True),
    R("peel", dict(out=P(3)), E, "peel: out" + VIS_WANT + "(2, 3, 64, 64) torch.float32"),
    R("peel", dict(out=P(4, dev="cpu")), E, "peel: out" + VIS_WANT + "(2, 4, 64, 64) torch.float32"),
    R("peel", dict(prev=None), E, "peel: prev" + VIS_WANT + "None", True, was="AttributeError"),
    R("layers", dict(n=0), E, "layers: n = 0, expected at least 1", True),
    R("composite", dict(colors=[]), E, "composite: 0 colour layers, 1 alpha layers", True),
    R("composite", dict(alphas=[P(1), P(1)]), E, "composite: 1 colour layers, 2 alpha layers", True),
    R("composite_layers", dict(colors=[P(3)]), E, "composite_layers: 2 layers, 1 colour buffers, 2 alphas", True),
    R("composite_layers", dict(layers=[], colors=[], alphas=[]), E, "composite_layers: 0 layers (1 .. 8), 0 colour buffers, 0 alphas", True),
    R("composite_layers", dict(layers=[VIS] * 9, colors=[P(3)] * 9, alphas=[0.5] * 9), E,
      "composite_layers: 9 layers (1 .. 8), 9 colour buffers, 9 alphas", True),
    R("composite_layers", dict(layers=[VIS, P(3)]), E, "composite_layers: layers[1]" + VIS_WANT + "(2, 3, 64, 64) torch.float32"),
    R("composite_layers", dict(layers=[P(4, dev="cpu"), VIS]), E, "composite_layers: layers[0]" + VIS_WANT + "(2, 4, 64, 64) torch.float32", True),
    R("composite_layers", dict(colors=[P(3), T(2, 3, H, 32)]), E, "composite_layers: colors[1] " + P3 + NARROW),
    R("composite_layers", dict(colors=[P(3, dev="cpu"), P(3)]), E, "composite_layers: colors[0] " + P3 + "(2, 3, 64, 64) torch.float32"),
    R("composite_layers", dict(colors=[P(65), P(65)], background=None), E,
      "composite_layers: colors[0] must be a CUDA float32 tensor (2, 65, 64, 64), got (2, 65, 64, 64) torch.float32"),
    R("composite_layers", dict(colors=[T(3, H, W), P(3)]), E,
      "composite_layers: colors[0] must be a CUDA float32 tensor (2, 0, 64, 64), got (3, 64, 64) torch.float32"),
    R("composite_layers", dict(alphas=[P(2), 0.5]), E,
      "composite_layers: alphas[0] must be a CUDA float32 tensor (2, 1, 64, 64) or a scalar, got (2, 2, 64, 64) torch.float32"),
    R("composite_layers", dict(background=P(4)), E, "composite_layers: background " + P3 + "(2, 4, 64, 64)"),
    R("composite_layers", dict(colors=[None, P(3)]), E, "composite_layers: colors[0] must be a CUDA float32 tensor (2, 0, 64, 64), got None",
      was="AttributeError"),
    R("composite_grad", dict(layers=[VIS]), E, "composite_layers: 1 layers (1 .. 8), 2 colour buffers, 2 alphas", True),
    R("composite_grad", dict(want_gcolor=[True]), E, "composite_grad: want_gcolor / want_galpha must be a bool or 2 bools"),
    R("composite_grad", dict(want_galpha=[True, False, True]), E, "composite_grad: want_gcolor / want_galpha must be a bool or 2 bools"),
    R("composite_grad", dict(background=None, want_gbg=True), E, "composite_grad: gbg without a background"),
    R("composite_grad", dict(background=None, want_gcolor=False, want_galpha=False), E, "composite_grad: no gradient is asked for"),
    R("composite_grad", dict(gout=P(4)), E, "composite_grad: gout " + P3 + "(2, 4, 64, 64) torch.float32"),
    R("composite_grad", dict(gout=P(3, dev="cpu")), E, "composite_grad: gout " + P3 + "(2, 3, 64, 64) torch.float32"),
    R("composite_grad", dict(gout=P(3), through=True), E, "composite_grad: gout " + P4 + "(2, 3, 64, 64) torch.float32"),
    R("composite_grad", dict(gout=None), E, "composite_grad: gout " + P3 + "None", was="AttributeError"),
    R("gbuffer_planes", dict(what=0), E, "gbuffer_planes: what = 0x0 names no group or an unknown one", True),
    R("gbuffer_planes", dict(what=0x10), E, "gbuffer_planes: what = 0x10 names no group or an unknown one", True),
    R("gbuffer_decode", dict(buf=P(8)), E, "gbuffer_decode: expected a [..., 9, rows, W] tensor of 4-byte words, got (2, 8, 64, 64) torch.float32", True),
    R("motion_planes", dict(what=0), E, "motion_planes: what = 0x0 names no group or an unknown one", True),
    R("motion_decode", dict(buf=P(4)), E, "motion_decode: expected a [..., 5, rows, W] tensor of 4-byte words, got (2, 4, 64, 64) torch.float32", True),
    # ---------------------------------------------------------------- interpolate, positions, depth, antialias
    R("interpolate", dict(attr=T(N_TRIS, 2, 5)), E, ATTR_WANT + "(24, 2, 5) torch.float32", True),
    R("interpolate", dict(attr=T(N_TRIS, 3, 5, dtype=torch.float64)), E, ATTR_WANT + "(24, 3, 5) torch.float64", True),
    R("interpolate", dict(attr=T(N_TRIS, 3, 5, dev="cpu")), E, ATTR_WANT + "(24, 3, 5) torch.float32", True),
    R("interpolate", dict(attr=T(3, N_TRIS, 3, 5)), E, "interpolate: attr has 3 frames, the set 2"),
    R("interpolate", dict(attr=None), E, ATTR_WANT + "None", True, was="AttributeError"),
    R("interpolate_bary_grad", dict(attr=T(5,)), E, ATTR_WANT + "(5,) torch.float32", True),
    R("interpolate_bary_grad", dict(gout=P(4)), E, "interpolate_bary_grad: gout must be float32 (2, 5, 64, 64), got (2, 4, 64, 64) torch.float32"),
    R("interpolate_bary_grad", dict(gout=P(5, dtype=torch.float64)), E,
      "interpolate_bary_grad: gout must be float32 (2, 5, 64, 64), got (2, 5, 64, 64) torch.float64"),
    R("position_grad", dict(gbary=None, gz=None), E, "position_grad: neither gbary nor gz is given", True),
    R("position_grad", dict(gbary=P(3)), E, "position_grad: gbary " + P2 + "(2, 3, 64, 64) torch.float32", True),
    R("position_grad", dict(gz=P(2)), E, "position_grad: gz " + P1 + "(2, 2, 64, 64) torch.float32"),
    R("position_grad", dict(gbary=None, gz=P(1, dev="cpu")), E, "position_grad: gz " + P1 + "(2, 1, 64, 64) torch.float32", True),
    R("position_grad", dict(fs=SFS), E, "position_grad: pos_tris must be given for a sceneset (at least every frame's triangle count)"),
    R("interpolate_geo", dict(attr=T(N_TRIS, 3)), E, ATTR_WANT + "(24, 3) torch.float32", True),
    R("interpolate_geo", dict(pos=BAD_POS), E, "interpolate_geo" + POS_WANT),
    R("interpolate_geo", dict(pos=T(3, N_TRIS, 3, 3)), E, "interpolate_geo: pos must be float32 [n_frames, T, 3, 3], got (3, 24, 3, 3) torch.float32"),
    R("depth", dict(pos=BAD_POS), E, "depth" + POS_WANT, True),
    R("depth", dict(pos=T(2, N_TRIS, 3, 3, dtype=torch.float64)), E, "depth: pos must be float32 [n_frames, T, 3, 3], got (2, 24, 3, 3) torch.float64", True),
    R("depth", dict(pos=None), E, "depth: pos must be float32 [n_frames, T, 3, 3], got None", True, was="AttributeError"),
    R("antialias_grad", dict(want_gin=False, want_gpos=False), E, "antialias_grad: neither gin nor gpos is asked for", True),
    R("antialias_grad", dict(color=T(2, 3, H, 32)), E,
      "antialias: color must be a CUDA float32 tensor [n_frames, C, rows, W] of the set, got " + NARROW, True),
    R("antialias_grad", dict(gout=T(3, H, W)), E,
      "antialias: gout must be a CUDA float32 tensor [n_frames, C, rows, W] of the set, got (3, 64, 64) torch.float32"),
    R("antialias_grad", dict(gout=P(3, dev="cpu")), E,
      "antialias: gout must be a CUDA float32 tensor [n_frames, C, rows, W] of the set, got (2, 3, 64, 64) torch.float32"),
    R("antialias_grad", dict(gout=P(4)), E, "antialias_grad: gout (2, 4, 64, 64) is not of color's shape (2, 3, 64, 64)"),
    R("antialias_grad", dict(fs=SFS), E, "position_grad: pos_tris must be given for a sceneset (at least every frame's triangle count)"),
    R("antialias", dict(color=P(65)), E, "antialias: color has 65 channels, 1 .. 64 are supported"),
    R("antialias", dict(color=P(0)), E, "antialias: color has 0 channels, 1 .. 64 are supported"),
    R("antialias", dict(color=P(3, dtype=torch.float16)), E,
      "antialias: color must be a CUDA float32 tensor [n_frames, C, rows, W] of the set, got (2, 3, 64, 64) torch.float16", True),
    R("antialias", dict(pos=BAD_POS), E, "antialias" + POS_WANT),
    R("antialias", dict(color=None), E, "antialias: color must be a CUDA float32 tensor [n_frames, C, rows, W] of the set, got None", True,
      was="AttributeError"),
    # ---------------------------------------------------------------- textures, cube maps, the background
    R("texture_grad", dict(want_gtex=False, want_guv=False), E, "texture_grad: neither gtex nor guv is asked for", True),
    R("texture_grad", dict(uv=P(3)), E, "texture: uv " + P2 + "(2, 3, 64, 64) torch.float32", True),
    R("texture_grad", dict(gout=P(2)), E, "texture_grad: gout must be float32 (2, 3, 64, 64), got (2, 2, 64, 64) torch.float32"),
    R("texture", dict(uv=P(2, dev="cpu")), E, "texture: uv " + P2 + "(2, 2, 64, 64) torch.float32", True),
    R("texture", dict(uv=None), E, "texture: uv " + P2 + "None", True, was="AttributeError"),
    R("texture", dict(tex=T(8, 3)), E, TEX_WANT + "(8, 3) torch.float32"),
    R("texture", dict(tex=T(8, 8, 3, dev="cpu")), E, TEX_WANT + "(8, 8, 3) torch.float32"),
    R("texture", dict(tex=None), E, TEX_WANT + "None", was="AttributeError"),
    R("texture", dict(tex=T(3, 8, 8, 3)), E, "texture: tex has 3 frames, the set 2"),
    R("texture", dict(tex=T(8, 8, 65)), E, "texture: tex is 8 x 8 texels of 65 channels; 1 .. 16384 and 1 .. 64 are supported"),
    R("texture", dict(tex=T(0, 8, 3)), E, "texture: tex is 8 x 0 texels of 3 channels; 1 .. 16384 and 1 .. 64 are supported"),
    R("texture_cube_grad", dict(want_gtex=False, want_gdir=False), E, "texture_cube_grad: neither gtex nor gdir is asked for", True),
    R("texture_cube_grad", dict(dirs=P(2)), E, "texture_cube: dirs " + P3 + "(2, 2, 64, 64) torch.float32", True),
    R("texture_cube_grad", dict(gout=P(3, dtype=torch.float64)), E,
      "texture_cube_grad: gout must be float32 (2, 3, 64, 64), got (2, 3, 64, 64) torch.float64"),
    R("texture_cube", dict(dirs=None), E, "texture_cube: dirs " + P3 + "None", True, was="AttributeError"),
    R("texture_cube", dict(cube=BAD_CUBE), E, CUBE_WANT + "(5, 4, 4, 3) torch.float32"),
    R("texture_cube", dict(cube=T(6, 4, 5, 3)), E, CUBE_WANT + "(6, 4, 5, 3) torch.float32"),
    R("texture_cube", dict(cube=None), E, CUBE_WANT + "None", was="AttributeError"),
    R("texture_cube", dict(cube=T(3, 6, 4, 4, 3)), E, "texture_cube: cube has 3 frames, the set 2"),
    R("texture_cube", dict(cube=T(6, 4, 4, 65)), E, "texture_cube: faces of 4 x 4 texels, 65 channels; 1 .. 16384 and 1 .. 64 are supported"),
    R("view_rays", dict(screen_from_world=T(4, 3)), E, "view_rays: screen_from_world must be [4, 4] or [n_frames, 4, 4], got (4, 3)", True),
    R("view_rays", dict(front=0), E, "view_rays: front must be +1 or -1, got 0", True),
    R("background", dict(where="some"), E, "background: where must be 'nobody' or 'all', got 'some'", True),
    R("background", dict(cube=BAD_CUBE), E, CUBE_WANT + "(5, 4, 4, 3) torch.float32", True),
    R("background", dict(rays=T(3, 9)), E, "background: rays must be a CUDA float32 tensor [1 or 2, 9], got (3, 9) torch.float32"),
    R("background", dict(rays=T(1, 8)), E, "background: rays must be a CUDA float32 tensor [1 or 2, 9], got (1, 8) torch.float32"),
    R("background", dict(rays=None), E, "background: rays must be a CUDA float32 tensor [1 or 2, 9], got None", was="AttributeError"),
    R("background", dict(vis=None), E, "background: vis may be None only with where='all'"),
    R("background_grad", dict(want_gtex=False, want_gray=False), E, "background_grad: neither gtex nor gray is asked for", True),
    R("background_grad", dict(gout=P(4)), E, "background_grad: gout must be float32 (2, 3, 64, 64), got (2, 4, 64, 64) torch.float32"),
    # ---------------------------------------------------------------- shadow, light, microfacet
    R("shadow", dict(width=-1.0), E, "shadow: bias and width must be finite and width >= 0, got bias 0.0, width -1.0", True),
    R("shadow", dict(bias=float("nan")), E, "shadow: bias and width must be finite and width >= 0, got bias nan, width 1.0", True),
    R("shadow", dict(map=T(4,)), E, MAP_WANT + "(4,) torch.float32", True),
    R("shadow", dict(map=T(2, 3, 16, 16)), E, MAP_WANT + "(2, 3, 16, 16) torch.float32", True),
    R("shadow", dict(map=T(16, 16, dtype=torch.float64)), E, MAP_WANT + "(16, 16) torch.float64", True),
    R("shadow", dict(map=None), E, MAP_WANT + "None", True, was="AttributeError"),
    R("shadow", dict(map=T(3, 16, 16)), E, "shadow: map has 3 frames, the set 2", True),
    R("shadow", dict(map=T(0, 16)), E, "shadow: map is 16 x 0 texels; 1 .. 16384 are supported", True),
    R("shadow", dict(map=T(16, 16, dev="cpu")), E, "shadow: map must be on the device, got cpu", True),
    R("shadow", dict(sc=P(2)), E, "shadow: sc must be a float32 tensor (2, 3, 64, 64), got (2, 2, 64, 64) torch.float32"),
    R("shadow", dict(sc=None), E, "shadow: sc must be a float32 tensor (2, 3, 64, 64), got None", was="AttributeError"),
    R("shadow", dict(sc=P(3, dev="cpu")), E, "shadow: sc must be on the device, got cpu"),
    R("shadow_grad", dict(want_gmap=False, want_gsc=False), E, "shadow_grad: neither gmap nor gsc is asked for", True),
    R("shadow_grad", dict(width=float("inf")), E, "shadow: bias and width must be finite and width >= 0, got bias 0.0, width inf", True),
    R("shadow_grad", dict(gout=P(3)), E, "shadow_grad: gout must be float32 (2, 1, 64, 64), got (2, 3, 64, 64) torch.float32"),
    R("light_params", dict(lights=T(3, 5)), E, "light: lights must be [L, 6] or [n_frames, L, 6] with 1 <= L <= 8, got (3, 5)", True),
    R("light_params", dict(lights=T(9, 6)), E, "light: lights must be [L, 6] or [n_frames, L, 6] with 1 <= L <= 8, got (9, 6)", True),
    R("light_params", dict(lights=None), E, "light: lights must be [L, 6] or [n_frames, L, 6] with 1 <= L <= 8, got None", True, was="AttributeError"),
    R("light_params", dict(eye=T(4)), E, "light: eye must be [3] or [n_frames, 3], got (4,)", True),
    R("light_params", dict(ks=T(2, 3, 3)), E, "light: ks must be [3] or [n_frames, 3], got (2, 3, 3)", True),
    R("light_params", dict(ka=None), E, "light: ka must be [3] or [n_frames, 3], got None", True, was="AttributeError"),
    R("light_params", dict(eye=T(3, 3)), E, "light: eye has 3 frames, the set 2", True),
    R("light_params", dict(lights=T(3, 3, 6)), E, "light: lights has 3 frames, the set 2", True),
    R("light", dict(lights=T(0, 6)), E, "light: lights must be [L, 6] or [n_frames, L, 6] with 1 <= L <= 8, got (0, 6)", True),
    R("light", dict(nrm=T(2, 3, H, 32)), E, "light: nrm " + P3 + NARROW, True),
    R("light", dict(pos=P(3, dev="cpu")), E, "light: pos " + P3 + "(2, 3, 64, 64) torch.float32"),
    R("light", dict(kd=P(2)), E, "light: kd " + P3 + "(2, 2, 64, 64) torch.float32"),
    R("light", dict(nrm=None), E, "light: nrm " + P3 + "None", True, was="AttributeError"),
    R("light", dict(p=0), E, "light: p must be an integer in 1 .. 256, got 0"),
    R("light", dict(p=2.5), E, "light: p must be an integer in 1 .. 256, got 2.5"),
    R("light_grad", dict(want_gnrm=False, want_gpos=False, want_gkd=False, want_gpar=False), E, "light_grad: no gradient is asked for", True),
    R("light_grad", dict(kd=None, want_gnrm=False, want_gpos=False, want_gpar=False), E, "light_grad: no gradient is asked for", True),
    R("light_grad", dict(par=T(1, 26)), E, "light: par must be a CUDA float32 tensor [1 or n_frames, 9 + 6 L], got (1, 26) torch.float32"),
    R("light_grad", dict(par=T(27,)), E, "light: par must be a CUDA float32 tensor [1 or n_frames, 9 + 6 L], got (27,) torch.float32"),
    R("light_grad", dict(par=None), E, "light: par must be a CUDA float32 tensor [1 or n_frames, 9 + 6 L], got None", was="AttributeError"),
    R("light_grad", dict(par=T(3, 27)), E, "light: par of 3 frames and 3 lights; 1 or 2 frames and 1 .. 8 lights are supported"),
    R("light_grad", dict(par=T(1, 63)), E, "light: par of 1 frames and 9 lights; 1 or 2 frames and 1 .. 8 lights are supported"),
    R("light_grad", dict(p=257), E, "light: p must be an integer in 1 .. 256, got 257"),
    R("light_grad", dict(gout=P(4)), E, "light_grad: gout must be float32 (2, 3, 64, 64), got (2, 4, 64, 64) torch.float32"),
    R("microfacet_params", dict(lights=T(3, 5)), E, "microfacet: lights must be [L, 6] or [n_frames, L, 6] with 1 <= L <= 8, got (3, 5)", True),
    R("microfacet_params", dict(amb=T(4)), E, "microfacet: amb must be [3] or [n_frames, 3], got (4,)", True),
    R("microfacet_params", dict(eye=T(3, 3)), E, "microfacet: eye has 3 frames, the set 2", True),
    R("microfacet", dict(nrm=T(2, 3, H, 32)), E, "microfacet: nrm " + P3 + "((2, 3, 64, 32), torch.float32)", True),
    R("microfacet", dict(pos=P(3, dtype=torch.float64)), E, "microfacet: pos " + P3 + "((2, 3, 64, 64), torch.float64)"),
    R("microfacet", dict(base=P(3, dev="cpu")), E, "microfacet: base " + P3 + "((2, 3, 64, 64), torch.float32)"),
    R("microfacet", dict(mat=P(3)), E, "microfacet: mat " + P2 + "((2, 3, 64, 64), torch.float32)"),
    R("microfacet", dict(mat=None), E, "microfacet: mat " + P2 + "None"),
    R("microfacet_grad", dict(want_gnrm=False, want_gpos=False, want_gbase=False, want_gmat=False, want_gpar=False), E,
      "microfacet_grad: no gradient is asked for", True),
    R("microfacet_grad", dict(par=T(1, 23)), E, "microfacet: par must be a CUDA float32 tensor [1 or n_frames, 6 + 6 L], got (1, 23) torch.float32"),
    R("microfacet_grad", dict(par=T(3, 24)), E, "microfacet: par of 3 frames and 3 lights; 1 or 2 frames and 1 .. 8 lights are supported"),
    R("microfacet_grad", dict(gout=P(2)), E, "microfacet_grad: gout must be float32 (2, 3, 64, 64), got (2, 2, 64, 64) torch.float32"),
    # ---------------------------------------------------------------- reflect, ibl, normal_map
    R("reflect_grad", dict(want_gnrm=False, want_gpos=False), E, "reflect_grad: no gradient is asked for", True),
    R("reflect_grad", dict(gout=P(3)), E, "reflect_grad: gout " + P4 + "((2, 3, 64, 64), torch.float32)"),
    R("reflect_grad", dict(gout=None), E, "reflect_grad: gout " + P4 + "None"),
    R("reflect", dict(nrm=P(3, dev="cpu")), E, "reflect: nrm " + P3 + "((2, 3, 64, 64), torch.float32)", True),
    R("reflect", dict(pos=None), E, "reflect: pos " + P3 + "None"),
    R("reflect", dict(eye=T(4)), E, "reflect: eye must be a CUDA float32 tensor [3] or [1 or 2, 3], got (4,) torch.float32"),
    R("reflect", dict(eye=T(3, 3)), E, "reflect: eye must be a CUDA float32 tensor [3] or [1 or 2, 3], got (3, 3) torch.float32"),
    R("reflect", dict(eye=T(3, dev="cpu")), E, "reflect: eye must be a CUDA float32 tensor [3] or [1 or 2, 3], got (3,) torch.float32"),
    R("reflect", dict(eye=None), E, "reflect: eye must be a CUDA float32 tensor [3] or [1 or 2, 3], got None", was="AttributeError"),
    R("brdf_table", dict(n=1), E, "brdf_table: 2 <= n <= 64 and 1 <= m <= 256, got n 1, m 4", True),
    R("brdf_table", dict(m=257), E, "brdf_table: 2 <= n <= 64 and 1 <= m <= 256, got n 8, m 257", True),
    R("brdf_table", dict(device="cpu"), E, "brdf_table: tab must be on the device, got cpu", True, was="unchecked"),
    R("ibl_grad", dict(want_gbase=False, want_gmat=False, want_gnv=False, want_girr=False, want_gspec=False, want_gtab=False), E,
      "ibl_grad: no gradient is asked for", True),
    R("ibl_grad", dict(gout=P(3, dev="cpu")), E, "ibl_grad: gout " + P3 + "((2, 3, 64, 64), torch.float32)"),
    R("ibl", dict(base=P(2)), E, "ibl: base " + P3 + "((2, 2, 64, 64), torch.float32)", True),
    R("ibl", dict(mat=None), E, "ibl: mat " + P2 + "None"),
    R("ibl", dict(nv=P(2)), E, "ibl: nv " + P1 + "((2, 2, 64, 64), torch.float32)"),
    R("ibl", dict(spec=T(2, 3, H, 32)), E, "ibl: spec " + P3 + "((2, 3, 64, 32), torch.float32)"),
    R("ibl", dict(tab=T(8, 4, 2)), E, "ibl: tab must be a CUDA float32 tensor [n, n, 2] with 2 <= n <= 64, got ((8, 4, 2), torch.float32)"),
    R("ibl", dict(tab=None), E, "ibl: tab must be a CUDA float32 tensor [n, n, 2] with 2 <= n <= 64, got None"),
    R("normal_map_grad", dict(want_gnrm=False, want_gtan=False, want_gm=False), E, "normal_map_grad: no gradient is asked for", True),
    R("normal_map_grad", dict(gout=P(4)), E, "normal_map_grad: gout must be float32 (2, 3, 64, 64), got (2, 4, 64, 64) torch.float32"),
    R("normal_map", dict(nrm=P(4)), E, "normal_map: nrm " + P3 + "(2, 4, 64, 64) torch.float32", True),
    R("normal_map", dict(tan=P(3)), E, "normal_map: tan " + P4 + "(2, 3, 64, 64) torch.float32"),
    R("normal_map", dict(m=P(3, dev="cpu")), E, "normal_map: m " + P3 + "(2, 3, 64, 64) torch.float32"),
    R("normal_map", dict(m=None), E, "normal_map: m " + P3 + "None", was="AttributeError"),
    # ---------------------------------------------------------------- derivatives and mip pyramids
    R("interpolate_deriv", dict(attr=T(N_TRIS, 3, 33)), E, "interpolate_deriv: 33 channels; at most 32 are supported"),
    R("interpolate_deriv", dict(attr=T(N_TRIS, 2, 2)), E, ATTR_WANT + "(24, 2, 2) torch.float32", True),
    R("mip_views", dict(n_levels=9), E, "mip: a 8 x 8 texture has 4 levels, 9 asked for", True),
    R("mip_views", dict(n_levels=0), E, "mip: a 8 x 8 texture has 4 levels, 0 asked for", True),
    R("mip_build", dict(tex=T(8, 3)), E, "mip_build: tex must be a CUDA float32 tensor [H, W, C] or [frames, H, W, C], got (8, 3) torch.float32", True),
    R("mip_build", dict(tex=T(8, 8, 3, dev="cpu")), E,
      "mip_build: tex must be a CUDA float32 tensor [H, W, C] or [frames, H, W, C], got (8, 8, 3) torch.float32", True),
    R("mip_build", dict(n_levels=5), E, "mip: a 8 x 8 texture has 4 levels, 5 asked for"),
    R("texture_mip_grad", dict(want_gtex=False, want_guv=False), E, "texture_mip_grad: neither gtex nor guv is asked for", True),
    R("texture_mip_grad", dict(gout=P(4)), E, "texture_mip_grad: gout must be float32 (2, 3, 64, 64), got (2, 4, 64, 64) torch.float32"),
    R("texture_mip_grad", dict(mip=T(62)), E, "texture_mip_grad: mip must be a flat CUDA float32 tensor of 63 elements (mip_build's layout)",
      was="unchecked"),
    R("texture_mip_grad", dict(mip=T(63, dev="cpu")), E, "texture_mip_grad: mip must be a flat CUDA float32 tensor of 63 elements (mip_build's layout)",
      was="unchecked"),
    R("texture_mip", dict(uv=P(3)), E, "texture: uv " + P2 + "(2, 3, 64, 64) torch.float32", True),
    R("texture_mip", dict(n_levels=5), E, "mip: a 8 x 8 texture has 4 levels, 5 asked for"),
    R("texture_mip", dict(uvd=P(3)), E, "texture_mip: uvd must be a CUDA float32 tensor (2, 4, 64, 64)"),
    R("texture_mip", dict(uvd=None), E, "texture_mip: uvd must be a CUDA float32 tensor (2, 4, 64, 64)"),
    R("cube_mip_views", dict(cube_shape=(6, 4, 2, 3)), E, "cube_mip: a cube is [6, N, N, C] or [frames, 6, N, N, C], got (6, 4, 2, 3)", True),
    R("cube_mip_views", dict(n_levels=9), E, "cube_mip: a cube of 4 x 4 faces has 3 levels, 9 asked for", True),
    R("cube_mip_build", dict(cube=T(6, 4, 4, 3, dtype=torch.float64)), E,
      "cube_mip_build: cube must be a CUDA float32 tensor, got (6, 4, 4, 3) torch.float64", True),
    R("cube_mip_build", dict(cube=T(6, 4, 4, 3, dev="cpu")), E, "cube_mip_build: cube must be a CUDA float32 tensor, got (6, 4, 4, 3) torch.float32", True),
    R("cube_mip_build", dict(cube=BAD_CUBE), E, "cube_mip: a cube is [6, N, N, C] or [frames, 6, N, N, C], got (5, 4, 4, 3)"),
    R("cube_level", dict(dirs=P(2)), E, "texture_cube: dirs " + P3 + "(2, 2, 64, 64) torch.float32", True),
    R("cube_level", dict(dird=P(3)), E, "cube_level: dird must be a CUDA float32 tensor (2, 6, 64, 64), got (2, 3, 64, 64) torch.float32"),
    R("cube_level", dict(dird=None), E, "cube_level: dird must be a CUDA float32 tensor (2, 6, 64, 64), got None", was="AttributeError"),
    R("texture_cube_mip_grad", dict(want_gtex=False, want_gdir=False, want_glam=False), E, "texture_cube_mip_grad: no gradient is asked for", True),
    R("texture_cube_mip_grad", dict(n_levels=4), E, "cube_mip: a cube of 4 x 4 faces has 3 levels, 4 asked for"),
    R("texture_cube_mip_grad", dict(gout=P(2)), E, "texture_cube_mip_grad: gout must be float32 (2, 3, 64, 64), got (2, 2, 64, 64) torch.float32"),
    R("texture_cube_mip_grad", dict(mip=T(91)), E, "texture_cube_mip: mip must be a flat CUDA float32 tensor of 90 elements (cube_mip_build's layout)"),
    R("texture_cube_mip", dict(dirs=P(3, dtype=torch.float16)), E, "texture_cube: dirs " + P3 + "(2, 3, 64, 64) torch.float16", True),
    R("texture_cube_mip", dict(lam=P(2)), E, "texture_cube_mip: lam must be a CUDA float32 tensor (2, 1, 64, 64)"),
    R("texture_cube_mip", dict(lam=None), E, "texture_cube_mip: lam must be a CUDA float32 tensor (2, 1, 64, 64)"),
    R("texture_cube_mip", dict(mip=T(89)), E, "texture_cube_mip: mip must be a flat CUDA float32 tensor of 90 elements (cube_mip_build's layout)"),
    R("texture_cube_mip", dict(mip=T(90, dev="cpu")), E, "texture_cube_mip: mip must be a flat CUDA float32 tensor of 90 elements (cube_mip_build's layout)"),
    R("cube_prefilter", dict(cube=BAD_CUBE), E, "cube_prefilter" + A_CUBE, True),
    R("cube_prefilter_pyramid", dict(cube=BAD_CUBE), E, "cube_prefilter_pyramid" + A_CUBE, True),
    R("cube_prefilter_grad", dict(gdst=BAD_CUBE), E, "cube_prefilter_grad" + A_CUBE, True),
    R("cube_prefilter_grad", dict(den=T(6, 4, 3)), E, "cube_prefilter_grad: den must be a CUDA float32 tensor (6, 4, 4), got (6, 4, 3) torch.float32"),
    R("cube_prefilter_grad", dict(out=T(6, 4, 4, 2)), E, "cube_prefilter_grad: out must be a contiguous float32 tensor (6, 4, 4, 3)"),
    R("cube_prefilter_grad", dict(out=T(6, 4, 4, 3, strided=True)), E, "cube_prefilter_grad: out must be a contiguous float32 tensor (6, 4, 4, 3)"),
    R("cube_prefilter_grad", dict(out=T(6, 4, 4, 3, dev="cpu")), E, "cube_prefilter_grad: out must be on the device, got cpu", was="unchecked"),
    # ---------------------------------------------------------------- the scenesets: vertex stage, normals, per-vertex attributes
    R("vertex_grad", dict(want_gverts=False, want_gdraw=False), E, "vertex_grad: neither gverts nor gdraw is asked for", True),
    R("vertex_grad", dict(gpos=T(2, N_FACES, 3, 2)), E,
      "vertex_grad: gpos must be a CUDA float32 tensor [n_frames, T, 3, 3], got (2, 12, 3, 2) torch.float32", True),
    R("vertex_grad", dict(gpos=T(2, N_FACES, 3, 3, dev="cpu")), E,
      "vertex_grad: gpos must be a CUDA float32 tensor [n_frames, T, 3, 3], got (2, 12, 3, 3) torch.float32", True),
    R("vertex_grad", dict(fs=FS), E, "the set is not a sceneset"),
    R("vertex_grad", dict(gdraw=T(2, 2, 18)), E, "vertex_grad: gdraw must be a contiguous float32 tensor (2, 1, 18)"),
    R("vertex_grad", dict(gdraw=T(2, 1, 18, dev="cpu")), E, "vertex_grad: gdraw must be on the device, got cpu", was="unchecked"),
    R("mesh_update", dict(verts8=T(N_VERTS, 7)), E, "mesh_update: verts8 must be a CUDA float32 tensor [V, 8], got (12, 7) torch.float32", True),
    R("scene_positions", dict(fs=FS), E, "the set is not a sceneset", True),
    R("scene_positions", dict(meshes={SLOT: T(11, 3)}), E, "scene_positions: mesh 3 must be float32 [12, 3] or [2, 12, 3], got (11, 3) torch.float32", True),
    R("scene_positions", dict(meshes={SLOT: T(3, N_VERTS, 3)}), E,
      "scene_positions: mesh 3 must be float32 [12, 3] or [2, 12, 3], got (3, 12, 3) torch.float32", True),
    R("scene_positions", dict(mvp=T(2, 1, 15)), E, "scene_positions: mvp must be float32 (2, 1, 16), got (2, 1, 15) torch.float32", True),
    R("scene_positions", dict(zmap=T(2, 2, 2)), E, "scene_positions: zmap must be float32 (2, 1, 2), got (2, 2, 2) torch.float32", True),
    R("mesh_normals", dict(pos=T(11, 3)), E,
      "mesh_normals: pos must be a CUDA float32 tensor [12, 3] or [B, 12, 3] (B <= 65535), got (11, 3) torch.float32", True),
    R("mesh_tangents", dict(pos=T(N_VERTS, 3, dev="cpu")), E,
      "mesh_normals: pos must be a CUDA float32 tensor [12, 3] or [B, 12, 3] (B <= 65535), got (12, 3) torch.float32", True),
    R("mesh_tangents", dict(uv=T(N_VERTS, 3)), E, "mesh_tangents: uv must be a CUDA float32 tensor [12, 2], got (12, 3) torch.float32"),
    R("corner_attr", dict(attrs={}), E, "corner_attr: no attributes given", True),
    R("corner_attr", dict(attrs={SLOT: T(11, 3)}), E,
      "corner_attr: slot 3 must be a CUDA float32 tensor [12, C] or [2, 12, C] with one C in 1..64 for every slot, got (11, 3) torch.float32", True),
    R("corner_attr", dict(attrs={SLOT: T(N_VERTS, 65)}), E,
      "corner_attr: slot 3 must be a CUDA float32 tensor [12, C] or [2, 12, C] with one C in 1..64 for every slot, got (12, 65) torch.float32", True),
    # ---------------------------------------------------------------- perspective-correct interpolation
    R("perspective", dict(vis=P(3)), E, "perspective: vis" + VIS_WANT + "(2, 3, 64, 64) torch.float32", True),
    R("perspective", dict(q=T(N_TRIS, 2)), E, "perspective: q must be a CUDA float32 tensor [T, 3] or [n_frames, T, 3], got (24, 2) torch.float32"),
    R("perspective", dict(q=None), E, "perspective: q must be a CUDA float32 tensor [T, 3] or [n_frames, T, 3], got None", was="AttributeError"),
    R("perspective", dict(q=T(3, N_TRIS, 3)), E, "perspective: q has 3 frames, the set 2"),
    R("perspective", dict(out=P(4, strided=True)), E, "perspective: out" + VIS_WANT + "(2, 4, 64, 64) torch.float32"),
    R("perspective_grad", dict(want_gbary=False, want_gq=False), E, "perspective_grad: neither gbary nor gq is asked for", True),
    R("perspective_grad", dict(vis=P(4, dev="cpu")), E, "perspective_grad: vis" + VIS_WANT + "(2, 4, 64, 64) torch.float32", True),
    R("perspective_grad", dict(q=T(N_TRIS, 3, dtype=torch.float64)), E,
      "perspective_grad: q must be a CUDA float32 tensor [T, 3] or [n_frames, T, 3], got (24, 3) torch.float64"),
    R("perspective_grad", dict(q=T(5, N_TRIS, 3)), E, "perspective_grad: q has 5 frames, the set 2"),
    R("perspective_grad", dict(gbary_p=P(3)), E, "perspective_grad: gbary_p " + P2 + "(2, 3, 64, 64) torch.float32"),
    R("interpolate_persp", dict(attr=T(N_TRIS, 3, 5, dtype=torch.int32)), E, ATTR_WANT + "(24, 3, 5) torch.int32", True),
    R("interpolate_persp", dict(pos=BAD_POS), E, "interpolate_persp" + POS_WANT),
    R("interpolate_persp", dict(vis=T(2, 4, H, 32)), E, "perspective: vis" + VIS_WANT + "(2, 4, 64, 32) torch.float32"),
    R("interpolate_persp", dict(q=T(N_TRIS,)), E, "perspective: q must be a CUDA float32 tensor [T, 3] or [n_frames, T, 3], got (24,) torch.float32"),
    R("clip_q", dict(fs=FS), E, "the set is not a sceneset", True),
    R("clip_q", dict(mvp=T(2, 1, 15)), E, "clip_q: mvp must be float32 (2, 1, 16), got (2, 1, 15) torch.float32", True),
    R("clip_q", dict(meshes={SLOT: T(11, 3)}), E, "clip_q: mesh 3 must be float32 [12, 3] or [2, 12, 3], got (11, 3) torch.float32", True),
    R("clip_q", dict(fs=SFS2, mvp=T(2, 2, 16)), E, "clip_q: frame 1 draws mesh slot 3 2 times; lay q out per draw instead", True),
    R("interpolate_deriv_persp", dict(vis=P(4, dtype=torch.int32)), E, "interpolate_deriv_persp: vis" + VIS_WANT + "(2, 4, 64, 64) torch.int32", True),
    R("interpolate_deriv_persp", dict(attr=T(N_TRIS, 3, 33)), E, "interpolate_deriv_persp: 33 channels; at most 32 are supported"),
    R("interpolate_deriv_persp", dict(q=T(N_TRIS, 4)), E,
      "interpolate_deriv_persp: q must be a CUDA float32 tensor [T, 3] or [n_frames, T, 3], got (24, 4) torch.float32"),
    # ---------------------------------------------------------------- None where a tensor is required, beside the rows above
    R("mesh_normals", dict(pos=None), E, "mesh_normals: pos must be a CUDA float32 tensor [12, 3] or [B, 12, 3] (B <= 65535), got None", True,
      was="AttributeError"),
    R("mesh_update", dict(verts8=None), E, "mesh_update: verts8 must be a CUDA float32 tensor [V, 8], got None", True, was="AttributeError"),
    R("mip_build", dict(tex=None), E, "mip_build: tex must be a CUDA float32 tensor [H, W, C] or [frames, H, W, C], got None", True, was="AttributeError"),
    R("cube_mip_build", dict(cube=None), E, "cube_mip_build: cube must be a CUDA float32 tensor, got None", True, was="AttributeError"),
    R("cube_prefilter", dict(cube=None), E, "cube_prefilter: a cube is a CUDA float32 tensor [6, N, N, C] or [frames, 6, N, N, C], got None", True,
      was="AttributeError"),
    R("cube_prefilter_grad", dict(den=None), E, "cube_prefilter_grad: den must be a CUDA float32 tensor (6, 4, 4), got None", was="AttributeError"),
    R("vertex_grad", dict(gpos=None), E, "vertex_grad: gpos must be a CUDA float32 tensor [n_frames, T, 3, 3], got None", True, was="AttributeError"),
]

# the functions whose `vis` went to the library as it was: each now refuses a host tensor, a buffer of another set's shape, a
# strided view and None in _vis_arg's words, after every other check of the call
VIS_FUNCTIONS = ("interpolate", "interpolate_bary_grad", "position_grad", "interpolate_geo", "depth", "antialias_grad", "antialias", "texture_grad",
                 "texture", "texture_cube_grad", "texture_cube", "background_grad", "background", "shadow_grad", "shadow", "light_grad", "light",
                 "microfacet_grad", "microfacet", "reflect_grad", "reflect", "ibl_grad", "ibl", "normal_map_grad", "normal_map", "interpolate_deriv",
                 "texture_mip_grad", "texture_mip", "cube_level", "texture_cube_mip_grad", "texture_cube_mip")
for _fn in VIS_FUNCTIONS:
    _host = _fn == "depth"  # (its one other argument is the never-read handle, which may live anywhere)
    ROWS += [R(_fn, dict(vis=P(4, dev="cpu")), E, _fn + ": vis" + VIS_WANT + "(2, 4, 64, 64) torch.float32", _host, "unchecked"),
             R(_fn, dict(vis=T(2, 4, H, 32)), E, _fn + ": vis" + VIS_WANT + "(2, 4, 64, 32) torch.float32", _host, "unchecked"),
             R(_fn, dict(vis=P(4, strided=True)), E, _fn + ": vis" + VIS_WANT + "(2, 4, 64, 64) torch.float32", _host, "unchecked")]
    if _fn not in ("background_grad", "background"):  # (there None is an argument: the one refusal above, or where="all")
        ROWS.append(R(_fn, dict(vis=None), E, _fn + ": vis" + VIS_WANT + "None", _host, "TypeError" if _host else "AttributeError"))

# the *_grad functions whose `gout` was checked for shape and dtype alone: (function, its planes)
GOUT_FUNCTIONS = (("interpolate_bary_grad", 5), ("texture_grad", 3), ("texture_cube_grad", 3), ("background_grad", 3), ("shadow_grad", 1), ("light_grad", 3),
                  ("microfacet_grad", 3), ("normal_map_grad", 3), ("texture_mip_grad", 3), ("texture_cube_mip_grad", 3))
for _fn, _n in GOUT_FUNCTIONS:
    ROWS += [R(_fn, dict(gout=P(_n, dev="cpu")), E, _fn + ": gout must be on the device, got cpu", was="unchecked"),
             R(_fn, dict(gout=None), E, f"{_fn}: gout must be float32 (2, {_n}, 64, 64), got None", was="AttributeError")]


def row_id(row):
    return row.fn + ":" + ",".join(f"{k}={v!r}" for k, v in row.fault.items()).replace(" ", "")


assert len({row_id(r) for r in ROWS}) == len(ROWS)
assert all(set(r.fault) <= set(V.__dict__[r.fn].__code__.co_varnames[:V.__dict__[r.fn].__code__.co_argcount]) for r in ROWS)


# ------------------------------------------------------------------------------------------------------ the kits
def scene_frames():
    """the frames of the two scenesets, and the mesh: SFS draws the mesh once per frame, SFS2 twice in its frame 1"""
    import vgkit
    pos, faces = vgkit.grid(3, 4, 5)
    m = vgkit.perspective(50.0, 46.0, 5.0, 6.0)
    faces = vgkit.oriented(pos, faces, m)
    assert pos.shape == (N_VERTS, 3) and faces.shape == (N_FACES, 3)
    ident = np.eye(4, dtype=np.float32).reshape(16)
    draw = (SLOT, abi.SHADER_NORMAL, -1, m, ident)
    frames = lambda counts: [abi.SceneFrame(W, H, (0.0, 0.0, 1.0), [], [draw] * n, 1.0, 0.0, abi.FUSED_CLEAR) for n in counts]  # noqa: E731
    return frames((1, 1)), frames((1, 2)), vgkit.verts8(pos), faces


def stub_kit():
    """what the wrappers ask of a set before anything reaches the library (tests/test_shadow_host.py's stub, and out_shape, frames and
    the context's mesh sizes), with meta tensors: no device, no library call"""
    once, twice, verts8, _ = scene_frames()
    ctx = types.SimpleNamespace(mesh_sizes={SLOT: (N_VERTS, N_FACES)})

    class Set:
        n_frames, out_shape = 2, (2, 4, H, W)

        def __init__(self, frames):
            self.frames, self.ctx = frames, ctx

        def interpolate_shape(self, c):
            return (2, c, H, W)
    plain = Set([types.SimpleNamespace(n_tris=N_TRIS)] * 2)
    return types.SimpleNamespace(device="meta", named={FS: plain, SFS: Set(once), SFS2: Set(twice), CTX: ctx, VIS: torch.zeros(plain.out_shape, device="meta"),
                                                       VERTS8: torch.zeros(N_VERTS, 8, device="meta")})


def build(spec, kit):
    if isinstance(spec, T):
        return spec.make(kit.device)
    if isinstance(spec, str) and spec in kit.named:
        return kit.named[spec]
    if isinstance(spec, (list, tuple)):
        return type(spec)(build(s, kit) for s in spec)
    if isinstance(spec, dict):
        return {k: build(s, kit) for k, s in spec.items()}
    return spec


def call(kit, fn, fault):
    """one call of srz.visibility.<fn> with VALID's arguments, those of `fault` in their place -> (its result, None), or (None, the
    exception it raised)"""
    args = dict(VALID[fn])
    args.update(fault)
    try:
        return getattr(V, fn)(**{k: build(v, kit) for k, v in args.items()}), None
    except Exception as e:  # noqa: BLE001 (the caller asserts which)
        return None, e


def raised_at(e):
    """the line of the innermost frame of the traceback that lies in srz/visibility.py"""
    lines = [f.lineno for f in traceback.extract_tb(e.__traceback__) if f.filename == V.__file__]
    return lines[-1] if lines else None


def check(kit, row):
    """the row's call is refused with the row's exception and, for a ValueError, exactly its text -> the line that raised"""
    _, e = call(kit, row.fn, row.fault)
    assert type(e) is row.exc, (row_id(row), repr(e))
    if row.text is not None:
        assert str(e) == row.text, row_id(row)
    return raised_at(e)
