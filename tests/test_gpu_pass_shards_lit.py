"""-m gpu: the shading passes over a visibility buffer on band shards — tests/test_gpu_pass_shards.py's two frame sizes and three
layouts (tests/shardkit.py) under light, microfacet, reflect, ibl, normal_map and background, forward and backward.  Per pass and
geometry (shardkit.hold_pass): the unsharded call against the pass's own reference (lightref, microfacetref, iblref, tangentref,
backgroundref on the device's visibility words) — planes word for word, float-atomic sums within the reference's gamma_n * sum |term|
—, then every rank on its rows of the whole-frame inputs, NaN in every float plane outside its bands and the sentinel in every output
there: the owned rows are the whole frame's word for word, the padding is untouched, with and without SRZ_FUSED_CLEAR.

The summed outputs.  gtab of ibl_grad and gtex of background_grad are float-atomic: a rank is held to the reference on the whole frame
with the other ranks' rows taken out of the pass — an owner pass: their ids written to nobody; background with SRZ_BG_NOBODY: a valid
owner written there; with SRZ_BG_ALL: +0 in gout there, where the reference still counts those rows' adds of +-0, so that bound has the
whole frame's n —, the ranks of worlds 3 and 5 together to the whole frame's reference, after
walkkit.teeth has shown from the reference alone that a band's share of an element is above four times its bound.  gpar of light_grad
and microfacet_grad and gray of background_grad are reduced in a fixed tree (include/srz.h): a rank's tiles in local order are the
frame's tiles of its bands in frame order and a tile without a contributing pixel adds +0, so the reference's tree over the whole
frame with the other ranks' rows taken out gives the rank's row bit for bit, per-frame and shared blocks alike; the rank without a
band writes +0 into the trees and leaves the atomic sums at shardkit.ACC_FILL, which they start from there.

background is the pass whose value is a function of the frame's row: with the shard-local row in its ray, every other test in the tree
passes.  Its tests assert from srz.parallel that rows at a local band >= 1 whose band is not lb * world + rank are among those
compared."""
import numpy as np
import pytest
import torch

import backgroundref as br
import cuberef
import iblref
import lightref
import microfacetref
import shardkit
import tangentref
from shardkit import GEOMETRIES, hold_pass, mask_rows, owner_pass
from srz import abi
from support import SENTINEL, ctx, filled, stream, words  # noqa: F401
from walkkit import dev

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
N_LIGHTS, P = 3, 5
TABLE = 8
CUBE_N = 4
BG_C = 3
RY_ALL = 0.04  # SRZ_BG_ALL: the scale of a block's ry


@pytest.fixture(scope="module")
def geos(ctx):
    yield from shardkit.make_geos(ctx)


def fl(fused):
    return F if fused else 0


def pre(g, k):
    return np.full((k, g.H, g.W), SENTINEL, np.uint32)


def done(**outs):
    torch.cuda.synchronize()
    return {k: words(t) for k, t in outs.items()}


def nobody_nan(g, a):
    a = np.ascontiguousarray(a, np.float32)
    a[np.broadcast_to(~g.own[:, None], a.shape)] = np.nan
    return a


def tree(tmp, terms):
    """srz_frameset_light_grad's fixed tree (tests/background_ref.c's br_tree, nine entries at a time) over per-pixel terms [K, H, W]
    that are 0 where a pixel does not contribute: adding +-0 changes no partial sum, each starts from +0"""
    K = len(terms)
    every = np.ones(terms.shape[1:], np.uint8)
    padded = np.zeros((-(-K // 9) * 9,) + terms.shape[1:], np.float32)
    padded[:K] = terms
    return np.concatenate([br.tree(tmp, padded[j:j + 9], every) for j in range(0, len(padded), 9)])[:K]


def fold(tmp, rows):
    """[n, K] float32 rows summed in frame order from +0: a shared block's frames"""
    rows = np.ascontiguousarray(rows, np.float32)
    K = rows.shape[1]
    padded = np.zeros((len(rows), -(-K // 9) * 9), np.float32)
    padded[:, :K] = rows
    return np.concatenate([br.fold(tmp, np.ascontiguousarray(padded[:, j:j + 9])) for j in range(0, padded.shape[1], 9)])[:K]


# ------------------------------------------------------------------------------------------------------ light and microfacet
class Lit:
    """light or microfacet: the planes each reads, its calls and its reference's (tests/test_gpu_pass_walk_lit.py's, on a Shard)"""

    def __init__(self, name):
        self.name, self.ref = name, lightref if name == "light" else microfacetref
        self.K = self.ref.par_len(N_LIGHTS)
        self.tail = (P,) if name == "light" else ()

    def inputs(self, g):
        """nrm, pos, kd — or nrm, pos, base, mat — [n, k, H, W] float32, NaN at nobody's pixels, and gout [n, 3, H, W]"""
        def make(g):
            per = [self.ref.make_planes(40 + i, (g.H, g.W)) for i in range(g.n)]
            cols = [nobody_nan(g, np.stack([p[k] for p in per])) for k in range(len(per[0]))]
            return cols[:-1], cols[-1]
        return g.memo(("lit", self.name), make)

    def pars(self):
        return {"": self.ref.make_params(19, N_LIGHTS, frames=shardkit.N_FRAMES), " shared": self.ref.make_params(23, N_LIGHTS)[None]}

    def forward(self, S, ins, par, fused):
        out, pt = S.out(3), dev(par)
        getattr(S.fs, self.name)(S.vis_in.data_ptr(), *(t.data_ptr() for t in ins), pt.data_ptr(), N_LIGHTS, len(par), *self.tail, out.data_ptr(),
                                 S.fs.interpolate_bytes(3), fl(fused), stream())
        return out

    def backward(self, S, ins, par, g, fused):
        outs = [S.out(t.shape[1]) for t in ins]
        pt, gpar = dev(par), filled((len(par), self.K))
        nbytes = S.fs.light_work_bytes(N_LIGHTS) if self.name == "light" else S.fs.microfacet_work_bytes(N_LIGHTS)
        work = filled((nbytes // 4 + 1,))
        getattr(S.fs, self.name + "_grad")(S.vis_in.data_ptr(), *(t.data_ptr() for t in ins), pt.data_ptr(), N_LIGHTS, len(par), *self.tail,
                                           g.data_ptr(), *(o.data_ptr() for o in outs), gpar.data_ptr(), work.data_ptr(), nbytes, fl(fused), stream())
        return outs, gpar


def run_lit(kind):
    lit = Lit(kind)

    def run(tmp, g, S, fused):
        ins = [S.dev(a) for a in lit.inputs(g)[0]]
        return done(**{"out" + k: lit.forward(S, ins, par, fused) for k, par in lit.pars().items()}), {}
    return run


def ref_lit(kind):
    lit = Lit(kind)

    def ref(tmp, g, v, fused):
        ins = lit.inputs(g)[0]
        return {"out" + k: np.stack([lit.ref.forward(tmp, g.n_tris[i], v[i, 1], *(a[i] for a in ins), par[i % len(par)], *lit.tail, fused, pre(g, 3))
                                     for i in range(g.n)]) for k, par in lit.pars().items()}, {}
    return ref


PLANES = {"light": ("gnrm", "gpos", "gkd"), "microfacet": ("gnrm", "gpos", "gbase", "gmat")}


def run_lit_grad(kind):
    lit = Lit(kind)

    def run(tmp, g, S, fused):
        planes, go = lit.inputs(g)
        ins, gd = [S.dev(a) for a in planes], S.dev(go)
        p, s = {}, {}
        for k, par in lit.pars().items():
            outs, gpar = lit.backward(S, ins, par, gd, fused)
            p.update(done(**{name + k: o for name, o in zip(PLANES[kind], outs)}))
            s["gpar" + k] = words(gpar).view(np.float32)
        return p, s
    return run


def ref_lit_grad(kind):
    lit = Lit(kind)

    def ref(tmp, g, v, fused):
        planes, go = lit.inputs(g)
        p, s = {}, {}
        for k, par in lit.pars().items():
            res = [lit.ref.grad(tmp, g.n_tris[i], v[i, 1], *(a[i] for a in planes), par[i % len(par)], *lit.tail, go[i], None, fused, pre(g, 3),
                                want_terms=True) for i in range(g.n)]
            for j, name in enumerate(PLANES[kind]):
                p[name + k] = np.stack([r[j] for r in res])
            rows = np.stack([tree(tmp, r[-1]) for r in res])
            s["gpar" + k] = (rows if len(par) > 1 else fold(tmp, rows)[None], None, None, 0)
        return p, s
    return ref


# ------------------------------------------------------------------------------------------------------ reflect, ibl, normal_map
def reflect_of(g):
    def make(g):
        per = [iblref.reflect_planes(50 + i, (g.H, g.W)) for i in range(g.n)]
        return [nobody_nan(g, np.stack([p[k] for p in per])) for k in range(3)], iblref.make_eye(25, g.n)
    return g.memo("reflect", make)


def run_reflect(tmp, g, S, fused):
    (nrm, pos, _), eye = reflect_of(g)
    n, p, e, out = S.dev(nrm), S.dev(pos), dev(eye), S.out(4)
    S.fs.reflect(S.vis_in.data_ptr(), n.data_ptr(), p.data_ptr(), e.data_ptr(), len(eye), out.data_ptr(), S.fs.interpolate_bytes(4), fl(fused), stream())
    return done(out=out), {}


def ref_reflect(tmp, g, v, fused):
    (nrm, pos, _), eye = reflect_of(g)
    return {"out": np.stack([iblref.reflect(tmp, g.n_tris[i], v[i, 1], nrm[i], pos[i], eye[i], fused, pre(g, 4)) for i in range(g.n)])}, {}


def run_reflect_grad(tmp, g, S, fused):
    (nrm, pos, go), eye = reflect_of(g)
    n, p, gd, e, gn, gp = S.dev(nrm), S.dev(pos), S.dev(go), dev(eye), S.out(3), S.out(3)
    S.fs.reflect_grad(S.vis_in.data_ptr(), n.data_ptr(), p.data_ptr(), e.data_ptr(), len(eye), gd.data_ptr(), gn.data_ptr(), gp.data_ptr(), fl(fused),
                      stream())
    return done(gnrm=gn, gpos=gp), {}


def ref_reflect_grad(tmp, g, v, fused):
    (nrm, pos, go), eye = reflect_of(g)
    res = [iblref.reflect_grad(tmp, g.n_tris[i], v[i, 1], nrm[i], pos[i], eye[i], go[i], fused, pre(g, 3)) for i in range(g.n)]
    return {"gnrm": np.stack([r[0] for r in res]), "gpos": np.stack([r[1] for r in res])}, {}


def ibl_of(g):
    """(the table, [base, mat, nv, irr, spec], gout)"""
    def make(g):
        per = [iblref.ibl_planes(60 + i, (g.H, g.W), TABLE) for i in range(g.n)]
        cols = [nobody_nan(g, np.stack([p[k] for p in per])) for k in range(6)]
        return iblref.smooth_table(TABLE), cols[:5], cols[5]
    return g.memo("ibl", make)


def run_ibl(tmp, g, S, fused):
    tab, planes, _ = ibl_of(g)
    ins, tt, out = [S.dev(a) for a in planes], dev(tab), S.out(3)
    S.fs.ibl(S.vis_in.data_ptr(), *(t.data_ptr() for t in ins), tt.data_ptr(), TABLE, out.data_ptr(), S.fs.interpolate_bytes(3), fl(fused), stream())
    return done(out=out), {}


def ref_ibl(tmp, g, v, fused):
    tab, planes, _ = ibl_of(g)
    return {"out": np.stack([iblref.ibl(tmp, g.n_tris[i], v[i, 1], *(a[i] for a in planes), tab, fused, pre(g, 3)) for i in range(g.n)])}, {}


IBL_PLANES = ("gbase", "gmat", "gnv", "girr", "gspec")


def run_ibl_grad(tmp, g, S, fused):
    tab, planes, go = ibl_of(g)
    ins, tt, gd = [S.dev(a) for a in planes], dev(tab), S.dev(go)
    outs, gtab = [S.out(a.shape[1]) for a in planes], S.acc(tt.shape)
    S.fs.ibl_grad(S.vis_in.data_ptr(), *(t.data_ptr() for t in ins), tt.data_ptr(), TABLE, gd.data_ptr(), *(o.data_ptr() for o in outs),
                  gtab.data_ptr(), fl(fused), stream())
    return done(**dict(zip(IBL_PLANES, outs))), {"gtab": gtab.cpu().numpy()}


def ref_ibl_grad(tmp, g, v, fused):
    tab, planes, go = ibl_of(g)
    acc = iblref.TabGrad(TABLE)
    res = [iblref.ibl_grad(tmp, g.n_tris[i], v[i, 1], *(a[i] for a in planes), tab, go[i], acc, fused, pre(g, 3)) for i in range(g.n)]
    p = {name: np.stack([r[j] for r in res]) for j, name in enumerate(IBL_PLANES)}
    return p, {"gtab": (acc.gsum, acc.gabs, acc.count, 1)}  # (extra 1: the add into the caller's word, tests/test_gpu_ibl.py's)


def tangent_of(g):
    def make(g):
        per = [tangentref.make_planes(70 + i, (g.H, g.W)) for i in range(g.n)]
        return [nobody_nan(g, np.stack([p[k] for p in per])) for k in range(4)]
    return g.memo("tangent", make)


def run_normal_map(tmp, g, S, fused):
    n, t, m, out = *(S.dev(a) for a in tangent_of(g)[:3]), S.out(3)
    S.fs.normal_map(S.vis_in.data_ptr(), n.data_ptr(), t.data_ptr(), m.data_ptr(), out.data_ptr(), S.fs.interpolate_bytes(3), fl(fused), stream())
    return done(out=out), {}


def ref_normal_map(tmp, g, v, fused):
    nrm, tan, m, _ = tangent_of(g)
    return {"out": np.stack([tangentref.nm_forward(tmp, g.n_tris[i], v[i, 1], nrm[i], tan[i], m[i], fused, SENTINEL) for i in range(g.n)])}, {}


def run_normal_map_grad(tmp, g, S, fused):
    n, t, m, gd = (S.dev(a) for a in tangent_of(g))
    outs = [S.out(k) for k in (3, 4, 3)]
    S.fs.normal_map_grad(S.vis_in.data_ptr(), n.data_ptr(), t.data_ptr(), m.data_ptr(), gd.data_ptr(), *(o.data_ptr() for o in outs), fl(fused),
                         stream())
    return done(gnrm=outs[0], gtan=outs[1], gm=outs[2]), {}


def ref_normal_map_grad(tmp, g, v, fused):
    nrm, tan, m, go = tangent_of(g)
    res = [tangentref.nm_grad(tmp, g.n_tris[i], v[i, 1], nrm[i], tan[i], m[i], go[i], fused, SENTINEL) for i in range(g.n)]
    return {name: np.stack([r[j] for r in res]) for j, name in enumerate(("gnrm", "gtan", "gm"))}, {}


# ------------------------------------------------------------------------------------------------------ background
def bg_of(g, where, shared):
    """(cube [n or 1, 6, N, N, C], ray blocks [n or 1, 9], gout [n, C, H, W]: NaN at the owned pixels under SRZ_BG_NOBODY, which never
    reads them)"""
    def make(g):
        cube = cuberef.make_cube(31, CUBE_N, BG_C, frames=1 if shared else g.n)
        rays = np.stack([br.camera_block(g.W, g.H, i, 1.6) for i in range(1 if shared else g.n)])
        if where == br.ALL:  # every pixel adds: the rays turn slowly from row to row, so that every band reaches every touched texel
            rays[:, 6:9] *= np.float32(RY_ALL)
        go = g.planes(32 + where, BG_C, 2.0, nan=g.own if where == br.NOBODY else None)
        return np.ascontiguousarray(cube.reshape((-1,) + cube.shape[-4:])), rays, go
    return g.memo(("background", where, shared), make)


def run_background(where, shared):
    def run(tmp, g, S, fused):
        cube, rays, _ = bg_of(g, where, shared)
        t, r, out = dev(cube), dev(rays), S.out(BG_C)
        S.fs.background(S.vis_in.data_ptr(), r.data_ptr(), len(rays), t.data_ptr(), CUBE_N, BG_C, len(cube), where, out.data_ptr(),
                        S.fs.interpolate_bytes(BG_C), fl(fused), stream())
        return done(out=out), {}
    return run


def bg_ids(g, rows, where):
    """the id planes the reference runs on for the rows `rows` alone: SRZ_BG_NOBODY: a valid owner written into the other rows;
    SRZ_BG_ALL: no ids (the other rows leave through gout)"""
    return None if where == br.ALL else mask_rows(g.v, rows, keep=1)[:, 1]


def ref_background(where, shared):
    def ref(tmp, g, rows, fused):
        cube, rays, _ = bg_of(g, where, shared)
        ids = bg_ids(g, rows, where)
        return {"out": np.stack([br.forward(tmp, cube[i % len(cube)], g.n_tris[i], None if ids is None else ids[i], rays[i % len(rays)], where, fused,
                                            pre(g, BG_C), shape=(g.H, g.W)) for i in range(g.n)])}, {}
    return ref


def run_background_grad(where, shared):
    def run(tmp, g, S, fused):
        cube, rays, go = bg_of(g, where, shared)
        t, r, gd = dev(cube), dev(rays), S.dev(go)
        gt, gr = S.acc(t.shape), filled((len(rays), 9))
        wb = S.fs.background_work_bytes()
        work = filled((wb // 4 + 1,))
        S.fs.background_grad(S.vis_in.data_ptr(), r.data_ptr(), len(rays), gd.data_ptr(), t.data_ptr(), CUBE_N, BG_C, len(cube), where, gt.data_ptr(),
                             gr.data_ptr(), work.data_ptr(), wb, fl(fused), stream())
        torch.cuda.synchronize()
        return {}, {"gtex": gt.cpu().numpy(), "gray": words(gr).view(np.float32)}
    return run


def ref_background_grad(where, shared):
    def ref(tmp, g, rows, fused):
        cube, rays, go = bg_of(g, where, shared)
        ids = bg_ids(g, rows, where)
        if where == br.ALL:  # +0 in gout at the other ranks' rows (the texels are finite): every term from there is a zero
            go = go.copy()
            go[:, :, ~rows] = 0.0
        accs = [br.Grad(cube.shape[-4:]) for _ in cube]
        out = [br.grad(tmp, cube[i % len(cube)], g.n_tris[i], None if ids is None else ids[i], rays[i % len(rays)], go[i], accs[i % len(cube)], where,
                       shape=(g.H, g.W))[0] for i in range(g.n)]
        gray = np.stack(out) if len(rays) > 1 else br.fold(tmp, np.stack(out))[None]
        return {}, {"gray": (gray, None, None, 0),
                    "gtex": (np.stack([a.gtex for a in accs]), np.stack([a.gabs for a in accs]), np.stack([a.count for a in accs])[..., None], 0)}
    return ref


BOTH = (False, True)
PASSES = {"light": (run_lit("light"), owner_pass(ref_lit("light")), BOTH),
          "light_grad": (run_lit_grad("light"), owner_pass(ref_lit_grad("light")), BOTH),
          "microfacet": (run_lit("microfacet"), owner_pass(ref_lit("microfacet")), BOTH),
          "microfacet_grad": (run_lit_grad("microfacet"), owner_pass(ref_lit_grad("microfacet")), BOTH),
          "reflect": (run_reflect, owner_pass(ref_reflect), BOTH), "reflect_grad": (run_reflect_grad, owner_pass(ref_reflect_grad), BOTH),
          "ibl": (run_ibl, owner_pass(ref_ibl), BOTH), "ibl_grad": (run_ibl_grad, owner_pass(ref_ibl_grad), BOTH),
          "normal_map": (run_normal_map, owner_pass(ref_normal_map), BOTH),
          "normal_map_grad": (run_normal_map_grad, owner_pass(ref_normal_map_grad), BOTH)}
for _where, _w in ((br.NOBODY, "nobody"), (br.ALL, "all")):
    for _shared, _s in ((False, "per-frame"), (True, "shared")):
        PASSES[f"background {_w} {_s}"] = (run_background(_where, _shared), ref_background(_where, _shared), BOTH)
        PASSES[f"background_grad {_w} {_s}"] = (run_background_grad(_where, _shared), ref_background_grad(_where, _shared), BOTH[:1])
ROTATED = ((3, 0), (3, 1), (3, 2), (5, 1), (5, 2))  # the ranks with a local band >= 1 that is not band lb * world + rank


@pytest.mark.parametrize("geo", list(GEOMETRIES))
@pytest.mark.parametrize("name", list(PASSES))
def test_every_shard_gives_the_whole_frames_words(geos, tmp_path, name, geo):
    run, ref, fused_options = PASSES[name]
    g = geos(geo)
    if name.startswith("background"):  # the point of this one: y is the frame's row — rows the rotation moves are among those compared
        assert all(shardkit.rotated_rows(g.H, r, w) > 0 and g.shard(w, r).late.sum() >= shardkit.rotated_rows(g.H, r, w) for (w, r) in ROTATED)
    hold_pass(tmp_path, g, name, run, ref, fused_options)
