"""-m gpu: what srz_frameset_microfacet and _microfacet_grad refuse, and in which words.  One call per row of CASES: every argument is
valid but the one the row names, so the call has exactly one fault; it must return SRZ_E_INVALID, leave the row's text — which names
the argument — in srz_last_error, and touch no buffer.  Nothing reaches a kernel: every call is refused on the host.
(tests/test_gpu_light_refusals.py's scheme; the words are srz_frameset_light's where the case is.)"""
import types

import pytest
import torch

import srz
from srz import abi
from support import frame, soup, stream

pytestmark = pytest.mark.gpu

F, E = abi.FUSED_CLEAR, abi.SRZ_E_INVALID
SENTINEL = 0x5eed5eed
T, W, H, L = 24, 64, 64, 3        # triangles per frame, frame size, lights
PLANES4 = 2 * 4 * H * W * 4       # bytes of a visibility buffer of the two-frame set = the largest buffer any call here names
PLANES3 = 2 * 3 * H * W * 4       # bytes of every three-plane buffer
PLANES2 = 2 * 2 * H * W * 4       # bytes of the material and of its gradient
PAR = abi.microfacet_par(L) * 4   # bytes of one parameter frame
WORK = 2 * (4 + 1) * PAR          # srz_frameset_microfacet_work_bytes of the set: two frames of four tiles, and a row per frame
WRONG_SHARD = "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)"
ONLY_FUSED = "only SRZ_FUSED_CLEAR is accepted in flags"
N_LIGHTS, PAR_FRAMES = "n_lights must be 1 .. SRZ_LIGHT_MAX", "par_frames must be 1 or the set's frame count"
FWD_16 = "the plane buffers (d_vis, d_nrm, d_pos, d_base, d_mat, d_out) must be 16-byte aligned"
BWD_16 = "the plane buffers (d_vis, d_nrm, d_pos, d_base, d_mat, d_gout, d_gnrm, d_gpos, d_gbase, d_gmat) must be 16-byte aligned"
BWD_4 = "d_par, d_gpar and d_work must be 4-byte aligned"
FWD_NAMES = " (d_out against d_vis, d_nrm, d_pos, d_base, d_mat, d_par)"
BWD_NAMES = " (d_gnrm, d_gpos, d_gbase, d_gmat, d_gpar, d_work against d_vis, d_nrm, d_pos, d_base, d_mat, d_par, d_gout)"
OUT_IN, OUT_OUT = "an output overlaps an input", "two outputs overlap"
NONE_ASKED = "none of d_gnrm, d_gpos, d_gbase, d_gmat, d_gpar is asked for"
WORK_SHORT = "work_bytes is below srz_frameset_microfacet_work_bytes"

# entry point -> its arguments after (ctx, fs), in order, each with the value of a valid call.  (name, offset): the address of a
# buffer of the kit plus `offset` bytes — vis: a visibility buffer; nrm, pos, base, mat, g, par: inputs of PLANES4 bytes (par: its
# first two parameter frames are read); o1 .. o6: sentinel-filled outputs of PLANES4 + 256 bytes.
ENTRIES = {
    "microfacet": dict(vis=("vis", 0), nrm=("nrm", 0), pos=("pos", 0), base=("base", 0), mat=("mat", 0), par=("par", 0), n_lights=L,
                       par_frames=1, out=("o1", 0), out_bytes=PLANES3, flags=F),
    "microfacet_grad": dict(vis=("vis", 0), nrm=("nrm", 0), pos=("pos", 0), base=("base", 0), mat=("mat", 0), par=("par", 0), n_lights=L,
                            par_frames=1, gout=("g", 0), gnrm=("o1", 0), gpos=("o2", 0), gbase=("o3", 0), gmat=("o6", 0), gpar=("o4", 0),
                            work=("o5", 0), work_bytes=WORK, flags=F),
}

# (entry point, the faulty argument(s), text after "srz_frameset_<entry point>"; WRONG_SHARD stands alone; None: no text is set)
CASES = [
    ("microfacet", dict(ctx=None), None),
    ("microfacet", dict(fs=None), ": null frameset"),
    ("microfacet", dict(vis=None), ": null d_vis"),
    ("microfacet", dict(nrm=None), ": null d_nrm"),
    ("microfacet", dict(pos=None), ": null d_pos"),
    ("microfacet", dict(mat=None), ": null d_mat"),
    ("microfacet", dict(par=None), ": null d_par"),
    ("microfacet", dict(out=None), ": null d_out"),
    ("microfacet", dict(n_lights=0), ": " + N_LIGHTS),
    ("microfacet", dict(n_lights=abi.LIGHT_MAX + 1), ": " + N_LIGHTS),
    ("microfacet", dict(n_lights=0xffffffff), ": " + N_LIGHTS),
    ("microfacet", dict(par_frames=0), ": " + PAR_FRAMES),
    ("microfacet", dict(par_frames=3), ": " + PAR_FRAMES),
    ("microfacet", dict(out_bytes=PLANES3 - 1), ": out_bytes is too small for d_out"),
    ("microfacet", dict(flags=abi.UNIFIED), ": " + ONLY_FUSED),
    ("microfacet", dict(flags=F | abi.ORDERED_RASTER), ": " + ONLY_FUSED),
    ("microfacet", dict(vis=("vis", 4)), ": " + FWD_16),
    ("microfacet", dict(nrm=("nrm", 8)), ": " + FWD_16),
    ("microfacet", dict(pos=("pos", 4)), ": " + FWD_16),
    ("microfacet", dict(base=("base", 12)), ": " + FWD_16),
    ("microfacet", dict(mat=("mat", 8)), ": " + FWD_16),
    ("microfacet", dict(out=("o1", 4)), ": " + FWD_16),
    ("microfacet", dict(par=("par", 2)), ": d_par must be 4-byte aligned"),
    ("microfacet", dict(out=("vis", 64)), FWD_NAMES + ": " + OUT_IN),
    ("microfacet", dict(out=("nrm", 0)), FWD_NAMES + ": " + OUT_IN),
    ("microfacet", dict(out=("pos", 16)), FWD_NAMES + ": " + OUT_IN),
    ("microfacet", dict(out=("base", 0)), FWD_NAMES + ": " + OUT_IN),
    ("microfacet", dict(out=("mat", 0)), FWD_NAMES + ": " + OUT_IN),
    ("microfacet", dict(mat=("o1", PLANES3 - 16)), FWD_NAMES + ": " + OUT_IN),
    ("microfacet", dict(nrm=("o1", PLANES3 - 16)), FWD_NAMES + ": " + OUT_IN),
    ("microfacet", dict(par=("o1", 4)), FWD_NAMES + ": " + OUT_IN),
    ("microfacet", dict(ctx="sharded"), WRONG_SHARD),

    ("microfacet_grad", dict(ctx=None), None),
    ("microfacet_grad", dict(fs=None), ": null frameset"),
    ("microfacet_grad", dict(vis=None), ": null d_vis"),
    ("microfacet_grad", dict(nrm=None), ": null d_nrm"),
    ("microfacet_grad", dict(pos=None), ": null d_pos"),
    ("microfacet_grad", dict(mat=None), ": null d_mat"),
    ("microfacet_grad", dict(par=None), ": null d_par"),
    ("microfacet_grad", dict(gout=None), ": null d_gout"),
    ("microfacet_grad", dict(gnrm=None, gpos=None, gbase=None, gmat=None, gpar=None), ": " + NONE_ASKED),
    ("microfacet_grad", dict(base=None), ": d_gbase needs d_base"),
    ("microfacet_grad", dict(work=None), ": d_gpar needs d_work"),
    ("microfacet_grad", dict(work_bytes=WORK - 1), ": " + WORK_SHORT),
    ("microfacet_grad", dict(work_bytes=0), ": " + WORK_SHORT),
    ("microfacet_grad", dict(n_lights=0), ": " + N_LIGHTS),
    ("microfacet_grad", dict(n_lights=abi.LIGHT_MAX + 1), ": " + N_LIGHTS),
    ("microfacet_grad", dict(par_frames=0), ": " + PAR_FRAMES),
    ("microfacet_grad", dict(par_frames=3), ": " + PAR_FRAMES),
    ("microfacet_grad", dict(flags=16), ": " + ONLY_FUSED),
    ("microfacet_grad", dict(vis=("vis", 4)), ": " + BWD_16),
    ("microfacet_grad", dict(nrm=("nrm", 4)), ": " + BWD_16),
    ("microfacet_grad", dict(pos=("pos", 8)), ": " + BWD_16),
    ("microfacet_grad", dict(base=("base", 4)), ": " + BWD_16),
    ("microfacet_grad", dict(mat=("mat", 4)), ": " + BWD_16),
    ("microfacet_grad", dict(gout=("g", 8)), ": " + BWD_16),
    ("microfacet_grad", dict(gnrm=("o1", 4)), ": " + BWD_16),
    ("microfacet_grad", dict(gpos=("o2", 8)), ": " + BWD_16),
    ("microfacet_grad", dict(gbase=("o3", 4)), ": " + BWD_16),
    ("microfacet_grad", dict(gmat=("o6", 12)), ": " + BWD_16),
    ("microfacet_grad", dict(par=("par", 2)), ": " + BWD_4),
    ("microfacet_grad", dict(gpar=("o4", 2)), ": " + BWD_4),
    ("microfacet_grad", dict(work=("o5", 1)), ": " + BWD_4),
    ("microfacet_grad", dict(gnrm=("vis", 16)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(gnrm=("nrm", 0)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(gpos=("pos", PLANES3 - 16)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(gbase=("base", 0)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(gmat=("mat", PLANES2 - 16)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(gmat=("g", 0)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(gpos=("g", 0)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(gpar=("par", 4)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(gpar=("g", 4)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(work=("vis", 4)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(work=("mat", 4)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(gout=("o1", 16)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(mat=("o6", PLANES2 - 16)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(par=("o4", PAR - 4)), BWD_NAMES + ": " + OUT_IN),
    ("microfacet_grad", dict(gpos=("o1", PLANES3 - 16)), BWD_NAMES + ": " + OUT_OUT),
    ("microfacet_grad", dict(gbase=("o2", 16)), BWD_NAMES + ": " + OUT_OUT),
    ("microfacet_grad", dict(gmat=("o3", PLANES3 - 16)), BWD_NAMES + ": " + OUT_OUT),
    ("microfacet_grad", dict(gpar=("o6", PLANES2 - 4)), BWD_NAMES + ": " + OUT_OUT),
    ("microfacet_grad", dict(work=("o4", PAR - 4)), BWD_NAMES + ": " + OUT_OUT),
    ("microfacet_grad", dict(work=("o3", 4)), BWD_NAMES + ": " + OUT_OUT),
    ("microfacet_grad", dict(ctx="sharded"), WRONG_SHARD),
]


def case_id(case):
    entry, fault, _ = case
    return entry + ":" + ",".join(f"{k}={'+'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in fault.items())


assert len({case_id(c) for c in CASES}) == len(CASES)


@pytest.fixture(scope="module")
def kit():
    """the contexts, the set and the buffers every case draws its arguments from"""
    tris = soup(3, T, W, H, (10.0, 20.0, 30.0))
    main, sharded = srz.Context(0), srz.Context(0, 0, 2)
    k = types.SimpleNamespace(ctx={"main": main, "sharded": sharded})
    k.fs = {"main": main.frameset([frame(tris, W, H), frame(tris[::-1].copy(), W, H)])}
    fs = k.fs["main"]
    vis = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    assert vis.numel() * 4 == PLANES4 == fs.out_bytes and fs.interpolate_bytes(3) == PLANES3 and fs.interpolate_bytes(2) == PLANES2
    assert fs.microfacet_work_bytes(L) == WORK and fs.microfacet_work_bytes(0) == 0 and fs.microfacet_work_bytes(9) == 0
    fs.render_visibility(vis.data_ptr(), PLANES4, F, stream())
    torch.cuda.synchronize()
    ones = lambda n: torch.ones(n, dtype=torch.float32, device="cuda")  # noqa: E731
    k.buf = {"vis": vis, "nrm": ones(PLANES4 // 4), "pos": ones(PLANES4 // 4) * 0.25, "base": ones(PLANES4 // 4), "mat": ones(PLANES4 // 4) * 0.5,
             "g": ones(PLANES4 // 4), "par": ones(PLANES4 // 4) * 3.0}
    for name in ("o1", "o2", "o3", "o4", "o5", "o6"):
        k.buf[name] = torch.full((PLANES4 // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    k.before = {name: t.clone() for name, t in k.buf.items()}
    yield k
    for fs in k.fs.values():
        fs.close()
    main.close(), sharded.close()


def call(kit, entry, fault):
    """one call of srz_frameset_<entry> with ENTRIES' arguments, those of `fault` in their place -> (return code, the ctx handle passed)"""
    args = dict(ctx="main", fs="main", **ENTRIES[entry])
    assert set(fault) <= set(args), (entry, fault)
    args.update(fault)
    h = kit.ctx[args.pop("ctx")].h if args["ctx"] is not None else args.pop("ctx")
    fs = kit.fs[args.pop("fs")].h if args["fs"] is not None else args.pop("fs")
    values = [kit.buf[v[0]].data_ptr() + v[1] if isinstance(v, tuple) else v for v in args.values()]
    return getattr(srz.lib(), "srz_frameset_" + entry)(h, fs, *values, None), h


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_refusal(kit, case):
    entry, fault, text = case
    L_ = srz.lib()
    # every context's text is first set to another refusal's, so that a stale text cannot stand in for the one expected
    marker = "srz_frameset_render: null frameset / output"
    for c in kit.ctx.values():
        assert L_.srz_frameset_render(c.h, None, None, 0, 0, None) == E and L_.srz_last_error(c.h).decode() == marker
    created = L_.srz_last_error(None)
    rc, h = call(kit, entry, fault)
    assert rc == E, (rc, L_.srz_last_error(h))
    if text is None:  # (no context to leave a text in: nobody's text changes)
        assert h is None and L_.srz_last_error(None) == created
        assert all(L_.srz_last_error(c.h).decode() == marker for c in kit.ctx.values())
    else:
        assert L_.srz_last_error(h).decode() == (text if text is WRONG_SHARD else f"srz_frameset_{entry}{text}")
    torch.cuda.synchronize()
    for name, t in kit.buf.items():
        assert torch.equal(t, kit.before[name]), f"{name} was written"


def test_the_valid_calls_are_accepted(kit):
    """ENTRIES' arguments are a valid call of both entry points, and so are the calls that leave out what may be left out: the
    refusals above are each due to the one argument their row changes"""
    for entry, fault in (("microfacet", {}), ("microfacet", dict(base=None)), ("microfacet", dict(par_frames=2)),
                         ("microfacet", dict(n_lights=1)), ("microfacet", dict(n_lights=abi.LIGHT_MAX)),
                         ("microfacet_grad", {}), ("microfacet_grad", dict(base=None, gbase=None)), ("microfacet_grad", dict(par_frames=2)),
                         ("microfacet_grad", dict(gpar=None, work=None, work_bytes=0)),
                         ("microfacet_grad", dict(gnrm=None, gpos=None, gbase=None, gmat=None)),
                         ("microfacet_grad", dict(gnrm=None, gpos=None, gbase=None, gpar=None, work=None, work_bytes=0)),
                         ("microfacet_grad", dict(gpar=None, work=("par", 2), work_bytes=0))):  # (without d_gpar, d_work is not looked at)
        rc, h = call(kit, entry, fault)
        assert rc == 0, (entry, fault, srz.lib().srz_last_error(h))
    torch.cuda.synchronize()
    for name in ("o1", "o2", "o3", "o4", "o6"):
        assert not torch.equal(kit.buf[name], kit.before[name]), name
    for name, t in kit.buf.items():  # (the outputs are written now: the sentinels go back for whatever runs next)
        t.copy_(kit.before[name])
