"""The visibility buffer's test reference, built on the unchanged CPU oracle (tests/vis_ref.c holds the arithmetic).

Every triangle of a frame gets a flat unit normal of its own (a greedy pick from a Fibonacci sphere: any two triangles whose boxes
overlap differ by >= SEP levels of 255 in some channel); the oracle renders that frame with SHADER_NORMAL, whose colour is
(n + 1) / 2 on the 0..255 scale (floored for S pixels), and each pixel the oracle changed is decoded to the one triangle that
contains it in its box and matches its colour within TOL.  Culling reads positions only, so visibility is that of the original
frame; alpha, beta and the per-class z of that owner come from vis_ref.c."""
import ctypes as C

import numpy as np

from srz import abi
from support import frame_positions, ref_lib

SEP, TOL, N_CAND = 4.0, 1.5, 16384
vp = C.c_void_p
SIGNATURES = {"vr_boxes": (None, [vp, C.c_int, C.c_int, C.c_int, vp]),
              "vr_assign": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_double, vp]),
              "vr_decode": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_double, vp, vp, vp, vp, vp]),
              "vr_bary": (None, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp])}


def lib(tmpdir):
    return ref_lib("vis_ref", tmpdir, SIGNATURES)


def _p(a):
    return a.ctypes.data


def fibonacci(n):
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    v = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)
    return v / np.linalg.norm(v, axis=1, keepdims=True).astype(np.float32)


def levels(n):
    return (n.astype(np.float64) + 1.0) * 0.5 * 255.0


class Reference:
    """recolour(frame) → the frame with flat normals (shaders kept: what the GPU renders) and its NORMAL-shaded twin (the oracle's)."""

    def __init__(self, tmpdir, frame):
        L = lib(tmpdir)
        self.W, self.H = frame.width, frame.height
        self.sizes = [len(t) for t in frame.tris]
        self.pos = frame_positions(frame)
        n = len(self.pos)
        self.box = np.zeros((max(n, 1), 4), np.int32)
        L.vr_boxes(_p(self.pos), n, self.W, self.H, _p(self.box))
        cand = fibonacci(N_CAND)
        choice = np.zeros(max(n, 1), np.int32)
        clev = np.ascontiguousarray(levels(cand))  # (held: the call gets a bare address)
        failed = L.vr_assign(_p(self.box), n, self.W, self.H, _p(clev), N_CAND, SEP, _p(choice))
        assert failed == 0, f"{failed} triangles found no normal {SEP} levels apart from their neighbours"
        self.nrm = cand[choice[:n]]
        self.tlev = np.ascontiguousarray(levels(self.nrm)) if n else np.zeros((1, 3))
        gpu_b, orc_b, k = [], [], 0
        for (t, b) in zip(frame.tris, range(len(frame.tris))):
            t2 = t.copy()
            t2["nrm"] = self.nrm[k:k + len(t)][:, None, :]
            k += len(t)
            sh, tex = int(frame._batches[b].shader), int(frame._batches[b].tex_id)
            gpu_b.append((sh, tex, t2))
            orc_b.append((abi.SHADER_NORMAL, -1, t2))
        kw = dict(ka=tuple(frame.c.ka), ks=tuple(frame.c.ks), p=frame.c.p, kh=frame.c.kh, kn=frame.c.kn)
        lights = frame.lights.view(np.float32).reshape(-1, 2, 3)
        self.gpu_frame = abi.Frame(self.W, self.H, tuple(frame.c.eye), lights, gpu_b, frame.c.flags, **kw)
        self.orc_frame = abi.Frame(self.W, self.H, tuple(frame.c.eye), lights, orc_b, frame.c.flags, **kw)
        self.unified = bool(frame.c.flags & abi.UNIFIED)
        self.L = L

    def expected(self, orc, planes_init=None, unified=None):
        """(words [4,H,W] uint32 of the visibility buffer, oracle planes, ambiguous pixels, per-class z [H,W])"""
        W, H = self.W, self.H
        init = planes_init if planes_init is not None else orc.new_planes(W, H)
        planes = tuple(np.array(p, np.float32, copy=True) for p in init)
        rc, out, _ = orc.draw(self.orc_frame, planes, want_stats=False)
        assert rc == 0
        fused = bool(self.orc_frame.c.flags & abi.FUSED_CLEAR)
        changed = np.zeros((H, W), bool)
        for a, b in zip(out, init):
            changed |= np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b, np.float32).view(np.uint32)
        if fused:  # the clear changed every pixel: owned = nobody's clear value left behind
            changed = ~((out[0] == np.inf) & (out[1] == 0) & (out[2] == 0) & (out[3] == 0))
        owner = np.zeros((H, W), np.int32)
        owned = np.ascontiguousarray(changed, np.uint8)
        c = [np.ascontiguousarray(x, np.float32) for x in out[1:]]
        n = len(self.pos)
        amb = self.L.vr_decode(_p(self.box), n, W, H, _p(self.tlev), TOL, _p(owned), _p(c[0]), _p(c[1]), _p(c[2]), _p(owner))
        cls = np.zeros((H, W), np.uint8)
        al, be, zz = (np.zeros((H, W), np.float32) for _ in range(3))
        uni = self.unified if unified is None else unified
        self.L.vr_bary(_p(self.pos), _p(self.box), W, H, int(uni), _p(owner), _p(cls), _p(al), _p(be), _p(zz))
        words = np.zeros((4, H, W), np.uint32)
        words[0] = np.ascontiguousarray(out[0], np.float32).view(np.uint32)
        own = owner >= 0
        words[1] = np.where(own, (owner.astype(np.int64) + 1) | (cls.astype(np.int64) << 31), 0).astype(np.uint32)
        words[2] = np.where(own, al.view(np.uint32), 0)
        words[3] = np.where(own, be.view(np.uint32), 0)
        if not fused:  # accumulate: what the oracle did not change keeps its incoming words
            for p in range(1, 4):
                words[p] = np.where(changed, words[p], np.ascontiguousarray(init[p], np.float32).view(np.uint32))
        return words, out, int(amb), zz, own
