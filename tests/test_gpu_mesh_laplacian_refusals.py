"""-m gpu: every SRZ_E_INVALID of srz_mesh_laplacian and srz_mesh_laplacian_grad (the list of include/srz.h) — nothing launched, the
outputs keep the sentinel, srz_last_error names the function — and the errors of srz.visibility.mesh_laplacian / mesh_solve."""
import numpy as np
import pytest
import torch

import srz
import vgkit
from srz import abi
from srz import visibility as V
from support import SENTINEL, ctx, filled, stream, words  # noqa: F401

pytestmark = pytest.mark.gpu

SLOT = 9
U, G, K = abi.LAP_UMBRELLA, abi.LAP_GRAPH, abi.LAP_COTAN


def refused(fn_name, fn, *untouched):
    """fn() raises SRZ_E_INVALID naming fn_name; every tensor of `untouched` still holds the sentinel"""
    with pytest.raises(srz.SrzError) as e:
        fn()
    assert e.value.code == abi.SRZ_E_INVALID and fn_name + ":" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for t in untouched:
        assert (words(t) == SENTINEL).all(), fn_name + ": an output was written"


@pytest.mark.parametrize("name", ["srz_mesh_laplacian", "srz_mesh_laplacian_grad"])
def test_refusals(ctx, name):
    pos, faces = vgkit.fan(70, 2)
    ctx.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    nv = len(pos)
    grad = name.endswith("_grad")
    call = ctx.mesh_laplacian_grad if grad else ctx.mesh_laplacian
    raw = getattr(srz.lib(), name)
    vp = srz.C.c_void_p
    xin = torch.zeros((2 * nv * 8,), dtype=torch.float32, device="cuda")
    wp = torch.as_tensor(pos).cuda()
    out = filled((2 * nv * 8,))
    x, w, o, s = xin.data_ptr(), wp.data_ptr(), out.data_ptr(), stream()
    assert raw(None, SLOT, vp(x), 3, 3, 1, G, vp(w), 3, vp(o), 3, None) == abi.SRZ_E_INVALID            # no context
    for slot in (-1, 256, 200):                                                                        # a bad id, an empty slot
        refused(name, lambda slot=slot: call(slot, x, 3, 3, 1, G, w, 3, o, 3, s), out)
    for n_sets in (0, 65536):
        refused(name, lambda n_sets=n_sets: call(SLOT, x, 3, 3, n_sets, G, w, 3, o, 3, s), out)
    for n_ch in (0, 65):
        refused(name, lambda n_ch=n_ch: call(SLOT, x, 80, n_ch, 1, G, w, 3, o, 80, s), out)
    refused(name, lambda: call(SLOT, x, 4, 5, 1, G, w, 3, o, 5, s), out)                                # a stride below n_ch
    refused(name, lambda: call(SLOT, x, 5, 5, 1, G, w, 3, o, 4, s), out)
    for kind in (U, G, K):
        refused(name, lambda kind=kind: call(SLOT, x, 3, 3, 1, kind, w, 2, o, 3, s), out)              # a wpos_stride below 3
    for kind in (-1, 3, 1 << 20):                                                                      # an unknown kind
        refused(name, lambda kind=kind: call(SLOT, x, 3, 3, 1, kind, w, 3, o, 3, s), out)
    if grad:                                                                                           # the backward has no null form
        refused(name, lambda: call(SLOT, None, 8, 3, 1, G, w, 3, o, 3, s), out)
    else:                                                                                              # the slot's own positions: 3 channels, 1 set
        refused(name, lambda: call(SLOT, None, 8, 4, 1, G, w, 3, o, 4, s), out)
        refused(name, lambda: call(SLOT, None, 8, 2, 1, G, w, 3, o, 3, s), out)
        refused(name, lambda: call(SLOT, None, 8, 3, 2, G, w, 3, o, 3, s), out)
    refused(name, lambda: call(SLOT, x, 3, 3, 1, G, w, 3, None, 3, s), out)                             # a null output
    for bad in ((x + 2, w, o), (x, w + 2, o), (x, w, o + 2), (x + 1, w, o)):                            # a misaligned pointer
        refused(name, lambda bad=bad: call(SLOT, bad[0], 3, 3, 1, K, bad[1], 3, bad[2], 3, s), out)
    span = 4 * (2 * nv * 3)
    for kind in (U, G, K):                                                                             # the output's span meets the input's
        refused(name, lambda kind=kind: call(SLOT, o, 3, 3, 2, kind, w, 3, o, 3, s), out)              # in place
        refused(name, lambda kind=kind: call(SLOT, o, 3, 3, 2, kind, w, 3, o + span - 4, 3, s), out)    # by one float
        refused(name, lambda kind=kind: call(SLOT, o + span - 4, 3, 3, 2, kind, w, 3, o, 3, s), out)
        refused(name, lambda kind=kind: call(SLOT, o, 8, 3, 2, kind, w, 3, o + 12, 8, s), out)          # no record form
    wspan = 4 * (nv * 3)
    refused(name, lambda: call(SLOT, x, 3, 3, 1, K, o + wspan - 4, 3, o, 3, s), out)                    # COTAN: the output meets wpos
    refused(name, lambda: call(SLOT, x, 3, 3, 1, K, o, 3, o + wspan - 4, 3, s), out)
    # what is NOT refused: spans that end where the other begins; wpos inside the output when the kind does not read it
    both = torch.zeros((2 * span // 4,), dtype=torch.float32, device="cuda")
    b = both.data_ptr()
    for kind in (U, G, K):
        call(SLOT, b, 3, 3, 2, kind, w, 3, b + span, 3, s)
        call(SLOT, b + span, 3, 3, 2, kind, w, 3, b, 3, s)
    wo = torch.as_tensor(np.tile(pos, (2, 1))).cuda()
    for kind in (U, G):
        call(SLOT, x, 3, 3, 2, kind, wo.data_ptr(), 3, wo.data_ptr(), 3, s)
    ctx.sync()


def test_the_torch_layers_own_errors(ctx):
    pos, faces = vgkit.fan(70, 2)
    ctx.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    nv = len(pos)
    x = torch.zeros((nv, 3), dtype=torch.float32, device="cuda")
    for fn in (lambda t, **kw: V.mesh_laplacian(ctx, SLOT, t, **kw), lambda t, **kw: V.mesh_solve(ctx, SLOT, t, 1.0, **kw)):
        for bad in (None, x.cpu(), x.double(), x[:-1], x.reshape(-1), x.reshape(1, 1, nv, 3), torch.zeros((nv, 65), device="cuda"),
                    torch.zeros((nv, 0), device="cuda"), torch.zeros((0, nv, 3), device="cuda")):
            with pytest.raises(ValueError):
                fn(bad)
        for wpos in (x.cpu(), x.double(), x[:-1], x[None], torch.zeros((nv, 4), device="cuda")):
            with pytest.raises(ValueError, match="wpos must be a CUDA float32 tensor"):
                fn(x, kind="cotan", wpos=wpos)
    for kind in ("uniform", 2, None):  # a kind that is none: the library's to refuse
        with pytest.raises(srz.SrzError, match="srz_mesh_laplacian: unknown kind") as e:
            V.mesh_laplacian(ctx, SLOT, x, kind)
        assert e.value.code == abi.SRZ_E_INVALID
    for kind in ("umbrella", "uniform", 2, None):  # the solve needs a symmetric operator
        with pytest.raises(NotImplementedError, match="symmetric"):
            V.mesh_solve(ctx, SLOT, x, 1.0, kind=kind)
    assert V.mesh_solve(ctx, SLOT, x, 1.0, iters=0).shape == x.shape
