"""-m gpu: every SRZ_E_INVALID of srz_mesh_edges and srz_mesh_edges_grad (the lists of include/srz.h) — nothing launched, the outputs
keep the sentinel, srz_last_error names the function — and what is NOT refused: spans that adjoin, a null d_work under LENGTH."""
import pytest
import torch

import srz
import vgkit
from srz import abi
from support import SENTINEL, ctx, filled, stream, words  # noqa: F401

pytestmark = pytest.mark.gpu

SLOT = 9
N, LEN, DIH = abi.EDGE_COUNT, abi.EDGE_LENGTH, abi.EDGE_DIHEDRAL


def refused(fn_name, fn, *untouched):
    """fn() raises SRZ_E_INVALID naming fn_name; every tensor of `untouched` still holds the sentinel"""
    with pytest.raises(srz.SrzError) as e:
        fn()
    assert e.value.code == abi.SRZ_E_INVALID and fn_name + ":" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for t in untouched:
        assert (words(t) == SENTINEL).all(), fn_name + ": an output was written"


def mesh(c):
    pos, faces = vgkit.fan(70, 2)
    c.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    return len(pos), len(faces)


def test_forward_refusals(ctx):
    name, call = "srz_mesh_edges", ctx.mesh_edges
    nv, nf = mesh(ctx)
    vp = srz.C.c_void_p
    pin = torch.zeros((2 * nv * 8,), dtype=torch.float32, device="cuda")
    out = filled((2 * nf * 8,))
    p, o, s = pin.data_ptr(), out.data_ptr(), stream()
    assert srz.lib().srz_mesh_edges(None, SLOT, vp(p), 3, 1, LEN, vp(o), 3, None) == abi.SRZ_E_INVALID  # no context
    for slot in (-1, 256, 200):                                                                        # a bad id, an empty slot
        refused(name, lambda slot=slot: call(slot, p, 3, 1, LEN, o, 3, s), out)
    for n_sets in (0, 65536):
        refused(name, lambda n_sets=n_sets: call(SLOT, p, 3, n_sets, LEN, o, 3, s), out)
    refused(name, lambda: call(SLOT, None, 8, 2, LEN, o, 3, s), out)                                    # the slot's own positions are one set
    refused(name, lambda: call(SLOT, p, 2, 1, LEN, o, 3, s), out)                                       # pos_stride below 3
    for kind in (-1, 3, 1 << 20):                                                                      # an unknown kind
        refused(name, lambda kind=kind: call(SLOT, p, 3, 1, kind, o, 3, s), out)
    refused(name, lambda: call(SLOT, p, 3, 2, N, o, 3, s), out)                                         # COUNT with n_sets != 1
    for kind in (N, LEN, DIH):
        refused(name, lambda kind=kind: call(SLOT, p, 3, 1, kind, None, 3, s), out)                    # a null output
        refused(name, lambda kind=kind: call(SLOT, p, 3, 1, kind, o, 2, s), out)                       # out_stride below 3
        for bad in ((p + 2, o), (p, o + 2), (p + 1, o)):                                               # a misaligned pointer
            refused(name, lambda kind=kind, bad=bad: call(SLOT, bad[0], 3, 1, kind, bad[1], 3, s), out)
        pspan = 4 * (nv * 3)
        refused(name, lambda kind=kind: call(SLOT, o, 3, 1, kind, o, 3, s), out)                       # the output's span meets the positions'
        refused(name, lambda kind=kind: call(SLOT, o, 3, 1, kind, o + pspan - 4, 3, s), out)           # by one float
        refused(name, lambda kind=kind: call(SLOT, o + 4 * (nf * 3) - 4, 3, 1, kind, o, 3, s), out)
    # what is NOT refused: spans that end where the other begins, either way round; the null form
    both = torch.zeros((nv * 3 + nf * 3,), dtype=torch.float32, device="cuda")
    b = both.data_ptr()
    for kind in (N, LEN, DIH):
        call(SLOT, b, 3, 1, kind, b + 4 * nv * 3, 3, s)
        call(SLOT, b + 4 * nf * 3, 3, 1, kind, b, 3, s)
        call(SLOT, None, 8, 1, kind, b, 3, s)
    ctx.sync()


def test_backward_refusals(ctx):
    name, call = "srz_mesh_edges_grad", ctx.mesh_edges_grad
    nv, nf = mesh(ctx)
    vp = srz.C.c_void_p
    pin = torch.zeros((2 * nv * 8,), dtype=torch.float32, device="cuda")
    gin = torch.zeros((2 * nf * 8,), dtype=torch.float32, device="cuda")
    work, gpos = filled((2 * nf * 3 + 8,)), filled((2 * nv * 3 + 8,))
    p, g, w, o, s = pin.data_ptr(), gin.data_ptr(), work.data_ptr(), gpos.data_ptr(), stream()
    outs = (work, gpos)
    assert srz.lib().srz_mesh_edges_grad(None, SLOT, vp(p), 3, 1, LEN, vp(g), 3, vp(w), vp(o), None) == abi.SRZ_E_INVALID
    for slot in (-1, 256, 200):
        refused(name, lambda slot=slot: call(slot, p, 3, 1, LEN, g, 3, w, o, s), *outs)
    for n_sets in (0, 65536):
        refused(name, lambda n_sets=n_sets: call(SLOT, p, 3, n_sets, LEN, g, 3, w, o, s), *outs)
    refused(name, lambda: call(SLOT, None, 8, 2, LEN, g, 3, w, o, s), *outs)
    refused(name, lambda: call(SLOT, p, 2, 1, LEN, g, 3, w, o, s), *outs)
    for kind in (-1, 3, 1 << 20):                                                                      # an unknown kind
        refused(name, lambda kind=kind: call(SLOT, p, 3, 1, kind, g, 3, w, o, s), *outs)
    for n_sets in (1, 2):                                                                              # COUNT has no backward
        refused(name, lambda n_sets=n_sets: call(SLOT, p, 3, n_sets, N, g, 3, w, o, s), *outs)
    refused(name, lambda: call(SLOT, p, 3, 1, DIH, g, 3, None, o, s), *outs)                            # a null d_work under DIHEDRAL
    for kind in (LEN, DIH):
        refused(name, lambda kind=kind: call(SLOT, p, 3, 1, kind, None, 3, w, o, s), *outs)            # a null d_gout, a null d_gpos
        refused(name, lambda kind=kind: call(SLOT, p, 3, 1, kind, g, 3, w, None, s), *outs)
        refused(name, lambda kind=kind: call(SLOT, p, 3, 1, kind, g, 2, w, o, s), *outs)               # gout_stride below 3
        for bad in ((p + 2, g, w, o), (p, g + 2, w, o), (p, g, w + 2, o), (p, g, w, o + 1)):           # a misaligned pointer
            refused(name, lambda kind=kind, bad=bad: call(SLOT, bad[0], 3, 1, kind, bad[1], 3, bad[2], bad[3], s), *outs)
        pspan, gspan = 4 * (nv * 3), 4 * (nf * 3)
        refused(name, lambda kind=kind: call(SLOT, o, 3, 1, kind, g, 3, w, o, s), *outs)               # gpos meets the positions
        refused(name, lambda kind=kind: call(SLOT, o + pspan - 4, 3, 1, kind, g, 3, w, o, s), *outs)
        refused(name, lambda kind=kind: call(SLOT, p, 3, 1, kind, o + pspan - 4, 3, w, o, s), *outs)   # gpos meets gout
        refused(name, lambda kind=kind: call(SLOT, p, 3, 1, kind, o, 3, w, o + gspan - 4, s), *outs)
    refused(name, lambda: call(SLOT, w, 3, 1, DIH, g, 3, w, o, s), *outs)                               # DIHEDRAL: the workspace meets the positions,
    refused(name, lambda: call(SLOT, p, 3, 1, DIH, w + gspan - 4, 3, w, o, s), *outs)                   # gout,
    refused(name, lambda: call(SLOT, p, 3, 1, DIH, g, 3, o + pspan - 4, o, s), *outs)                   # and gpos
    refused(name, lambda: call(SLOT, p, 3, 1, DIH, g, 3, o, o, s), *outs)
    # what is NOT refused: adjoining spans; a null d_work under LENGTH, and one LENGTH never touches wherever it points
    ring = torch.zeros((nv * 3 + nf * 3 + nf * 3 + nv * 3,), dtype=torch.float32, device="cuda")
    r = ring.data_ptr()
    r_g, r_w, r_o = r + 4 * nv * 3, r + 4 * (nv * 3 + nf * 3), r + 4 * (nv * 3 + 2 * nf * 3)
    for kind in (LEN, DIH):
        call(SLOT, r, 3, 1, kind, r_g, 3, r_w, r_o, s)
    call(SLOT, p, 3, 1, LEN, g, 3, None, o, s)
    call(SLOT, p, 3, 1, LEN, g, 3, p, o, s)
    call(SLOT, None, 8, 1, DIH, g, 3, w, o, s)
    ctx.sync()
    assert (words(work)[nf * 3:] == SENTINEL).all() and (words(gpos)[nv * 3:] == SENTINEL).all()
