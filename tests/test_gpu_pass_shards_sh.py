"""-m gpu: the SH9 pixel pass on band shards — srz_frameset_sh and srz_frameset_sh_grad on tests/shardkit.py's two geometries and three
layouts (worlds 3, 5 and ranks 6 and 7 of world 8: the ragged band alone, and the rank without a band), on which a rank's local band
`lb` is not band `lb * world + rank`.  The planes (out, gnrm) go through shardkit.hold_pass: the unsharded call against
tests/shref.py on every row, then every shard's owned rows against the whole frame's word for word, every padding word untouched
(check_planes), with and without SRZ_FUSED_CLEAR, per-frame and shared coefficients.  gsh is reduced in srz_frameset_light_grad's
fixed tree: a rank's tiles in local order are the frame's tiles of its bands in frame order and a tile without a lit pixel adds +0,
so every rank's rows are held BIT FOR BIT to the tree (tests/background_ref.c's br_tree, nine entries — one channel — at a time)
over the reference's float32 terms of the rank's rows, and within Grad.bound of its double sums; the rank without a band writes +0
in every entry; the ranks of worlds 3 and 5 together lie within the whole frame's bound (check_rank_sum), after walkkit.teeth has
shown from the reference alone that a band's share of an entry is above four times that bound."""
import numpy as np
import pytest
import torch

import backgroundref as br
import shardkit
import shref
from shardkit import GEOMETRIES, band_masks, band_shares, check_rank_sum, hold_pass, mask_rows, masked_ids, owner_pass
from srz import abi
from support import SENTINEL, ctx, filled, stream, words  # noqa: F401
from walkkit import check_bound, dev, same, teeth

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
N_CH = 3
KIND = shref.IRRADIANCE


@pytest.fixture(scope="module")
def geos(ctx):
    yield from shardkit.make_geos(ctx)


def fl(fused):
    return F if fused else 0


def pre(g, k):
    return np.full((k, g.H, g.W), SENTINEL, np.uint32)


def inputs(g):
    """(nrm [n, 3, H, W], gout [n, C, H, W]) float32, NaN at nobody's pixels"""
    def make(g):
        per = [shref.make_planes(50 + i, (g.H, g.W), N_CH) for i in range(g.n)]
        out = []
        for k in range(2):
            a = np.stack([p[k] for p in per])
            a[np.broadcast_to(~g.own[:, None], a.shape)] = np.nan
            out.append(a)
        return out
    return g.memo("sh", make)


def coefficients():
    return {"": shref.make_sh(51, N_CH, frames=shardkit.N_FRAMES), " shared": shref.make_sh(52, N_CH)[None]}


def backward(S, nrm, sh, gd, fused, want_nrm=True):
    gn = S.out(3) if want_nrm else None
    st, gsh = dev(sh), filled((len(sh), 9, N_CH))
    nbytes = S.fs.sh_work_bytes(N_CH)
    work = filled((nbytes // 4 + 1,))
    S.fs.sh_grad(S.vis_in.data_ptr(), nrm.data_ptr(), st.data_ptr(), N_CH, len(sh), KIND, gd.data_ptr(), None if gn is None else gn.data_ptr(),
                 gsh.data_ptr(), work.data_ptr(), nbytes, fl(fused), stream())
    torch.cuda.synchronize()
    return gn, words(gsh).view(np.float32)


def run_sh(tmp, g, S, fused):
    nrm = S.dev(inputs(g)[0])
    outs = {}
    for k, sh in coefficients().items():
        out, st = S.out(N_CH), dev(sh)
        S.fs.sh(S.vis_in.data_ptr(), nrm.data_ptr(), st.data_ptr(), N_CH, len(sh), KIND, out.data_ptr(), S.fs.interpolate_bytes(N_CH), fl(fused),
                stream())
        outs["out" + k] = out
    torch.cuda.synchronize()
    return {k: words(t) for k, t in outs.items()}, {}


def ref_sh(tmp, g, v, fused):
    nw = inputs(g)[0]
    return {"out" + k: np.stack([shref.forward(tmp, g.n_tris[i], v[i, 1], nw[i], sh[i % len(sh)], KIND, fused, pre(g, N_CH)) for i in range(g.n)])
            for k, sh in coefficients().items()}, {}


def run_sh_grad(tmp, g, S, fused):
    nw, go = inputs(g)
    nrm, gd = S.dev(nw), S.dev(go)
    return {"gnrm" + k: words(backward(S, nrm, sh, gd, fused)[0]) for k, sh in coefficients().items()}, {}


def ref_sh_grad(tmp, g, v, fused):
    nw, go = inputs(g)
    return {"gnrm" + k: np.stack([shref.grad(tmp, g.n_tris[i], v[i, 1], nw[i], sh[i % len(sh)], KIND, go[i], None, fused, pre(g, 3)) for i in range(g.n)])
            for k, sh in coefficients().items()}, {}


PASSES = {"sh": (run_sh, owner_pass(ref_sh)), "sh_grad": (run_sh_grad, owner_pass(ref_sh_grad))}


@pytest.mark.parametrize("geo", list(GEOMETRIES))
@pytest.mark.parametrize("name", list(PASSES))
def test_every_shard_gives_the_whole_frames_words(geos, tmp_path, name, geo):
    run, ref = PASSES[name]
    hold_pass(tmp_path, geos(geo), name, run, ref, (False, True))


def ref_gsh(tmp, g, v, sh):
    """on the visibility words v: (the rows [sh frames, 9, C] float32 in the fixed tree, one Grad per row)"""
    nw, go = inputs(g)
    shared = len(sh) == 1
    accs = [shref.Grad(N_CH) for _ in range(1 if shared else g.n)]
    rows = []
    for i in range(g.n):
        _, terms = shref.grad(tmp, g.n_tris[i], v[i, 1], nw[i], sh[i % len(sh)], KIND, go[i], accs[0 if shared else i], want_terms=True)
        every = np.ones((g.H, g.W), np.uint8)  # (a term is 0 where the pixel does not contribute: adding +-0 changes no partial sum)
        rows.append(np.stack([br.tree(tmp, terms[:, c], every) for c in range(N_CH)], 1))
    rows = np.stack(rows)
    if shared:
        rows = np.stack([br.fold(tmp, np.ascontiguousarray(rows[:, :, c])) for c in range(N_CH)], 1)[None]
    return rows, accs


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_gsh_on_every_shard(geos, tmp_path, geo):
    g = geos(geo)
    nw, go = inputs(g)
    stack = lambda accs, k: np.stack([getattr(a, k) for a in accs])  # noqa: E731
    for k, sh in coefficients().items():
        what = f"gsh{k}, {g.name}"
        # the anchor: the unsharded call against the tree and the double sums on every row
        want, accs = ref_gsh(tmp_path, g, g.v, sh)
        _, got = backward(g.whole, g.whole.dev(nw), sh, g.whole.dev(go), False, want_nrm=False)
        same(got, want, what + ": the whole frame against the reference's tree")
        gsum, gabs, cnt = (stack(accs, key) for key in ("gsum", "gabs", "count"))
        extra = g.n - 1 if len(sh) == 1 else 0  # (shared: the frames' rows are added too)
        check_bound(got, gsum, gabs, cnt, what + ", whole frame", extra)
        per_band = [stack(ref_gsh(tmp_path, g, mask_rows(g.v, m), sh)[1], "gabs") for m in band_masks(g.H)]
        teeth(band_shares(gabs.shape, per_band), gabs, cnt, what, single=False)
        parts = {}
        for S in g.shards():
            _, part = backward(S, S.dev(nw), sh, S.dev(go), False, want_nrm=False)
            if not S.rows:  # the rank without a band: written, +0 in every entry
                assert not part.view(np.uint32).any(), f"{what}: {S} wrote something but +0"
                continue
            mine, maccs = ref_gsh(tmp_path, g, masked_ids(g.v, S), sh)
            same(part, mine, f"{what}, {S}: against the reference's tree on the rank's rows")
            assert mine.any()
            check_bound(part, stack(maccs, "gsum"), stack(maccs, "gabs"), stack(maccs, "count"), f"{what}, {S}", extra)
            parts.setdefault(S.world, []).append(part)
        for w in shardkit.SUM_WORLDS:
            assert len(parts[w]) == w
            check_rank_sum(parts[w], gsum, gabs, cnt, f"{what}, world {w}", extra)
