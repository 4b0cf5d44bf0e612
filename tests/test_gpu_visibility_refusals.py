"""-m gpu: EVERY row of tests/visrefusals.py with CUDA tensors on real sets — what srz.visibility refuses, and in which words.  Each
call has exactly one fault and is refused on the host: no row reaches a kernel.  The only launches are the table's valid calls, made
once each on the 64 x 64 set, and the last test holds the table to the source: every `raise ValueError` of srz/visibility.py is the
innermost frame of some row, so a pass that adds a refusal without pinning it fails here."""
import types

import pytest
import torch

import srz
import visrefusals as X
from srz import abi
from srz import visibility as V
from support import frame, soup, stream

pytestmark = pytest.mark.gpu

# `raise ValueError` statements no argument can reach, by their line's text (at most 3: more would be dead checks, to be removed)
UNREACHED = ()


@pytest.fixture(scope="module")
def kit():
    """the plain set (two frames of 64 x 64 with 24 triangles), its visibility buffer, and the two scenesets over one 12-face mesh"""
    tris = soup(3, X.N_TRIS, X.W, X.H, (10.0, 20.0, 30.0))
    ctx = srz.Context(0)
    once, twice, verts8, faces = X.scene_frames()
    ctx.mesh_upload(X.SLOT, verts8, faces)
    sets = [ctx.frameset([frame(tris, X.W, X.H), frame(tris[::-1].copy(), X.W, X.H)]), ctx.frameset(once), ctx.frameset(twice)]
    vis = torch.zeros(sets[0].out_shape, dtype=torch.float32, device="cuda")
    sets[0].render_visibility(vis.data_ptr(), sets[0].out_bytes, abi.FUSED_CLEAR, stream())
    torch.cuda.synchronize()
    assert tuple(vis.shape) == (2, 4, X.H, X.W) and all(tuple(s.out_shape) == tuple(vis.shape) for s in sets)
    yield types.SimpleNamespace(device="cuda", named={X.FS: sets[0], X.SFS: sets[1], X.SFS2: sets[2], X.CTX: ctx, X.VIS: vis,
                                                      X.VERTS8: torch.as_tensor(verts8).cuda()})
    for s in sets:
        s.close()
    ctx.close()


@pytest.mark.parametrize("row", X.ROWS, ids=X.row_id)
def test_refusal(kit, row):
    before = kit.named[X.VIS].clone()
    assert X.check(kit, row) is not None
    torch.cuda.synchronize()
    assert torch.equal(kit.named[X.VIS].view(torch.int32), before.view(torch.int32))


def test_the_valid_calls_are_accepted(kit):
    """VALID's arguments are a call every function accepts: each refusal above is due to the one argument its row changes"""
    for fn in X.VALID:
        _, e = X.call(kit, fn, {})
        assert e is None, (fn, repr(e))
    for fn, fault in (("background", dict(vis=None, where="all")), ("light", dict(kd=None)), ("antialias", dict(pos=None)),
                      ("texture_mip", dict(uvd=None, n_levels=1)), ("texture_cube_mip", dict(lam=None, n_levels=1)),
                      ("position_grad", dict(gbary=None)), ("composite_layers", dict(background=None))):
        _, e = X.call(kit, fn, fault)
        assert e is None, (fn, fault, repr(e))
    torch.cuda.synchronize()


def test_every_refusal_of_the_layer_is_pinned(kit):
    """completeness, asserted: every line of srz/visibility.py that starts a `raise ValueError` statement is where some row's
    exception was raised"""
    source = open(V.__file__).read().splitlines()
    sites = {n for n, line in enumerate(source, 1) if line.lstrip().startswith("raise ValueError")}
    hit = {X.check(kit, row) for row in X.ROWS}
    assert hit <= sites, sorted(hit - sites)
    left = sorted(source[n - 1].strip() for n in sites - hit)
    assert len(UNREACHED) <= 3 and left == sorted(UNREACHED), left
