"""-m gpu: what the eight passes over a visibility buffer refuse, and in which words (srz_frameset_shade_visibility, _gbuffer, _motion,
_interpolate, _interpolate_grad, _position_grad, _antialias, _antialias_grad).  One call per row of CASES: every argument is valid but
the one the row names, so the call has exactly one fault; it must return the row's code, leave the row's text in srz_last_error and
touch no buffer.  The texts are the ones the entry points had before their argument checks were gathered into one place: a change of
a word here is a change of the interface.  Nothing reaches a kernel: every call is refused on the host."""
import types

import pytest
import torch

import srz
from srz import abi
from support import frame, soup, stream

pytestmark = pytest.mark.gpu

F, E = abi.FUSED_CLEAR, abi.SRZ_E_INVALID
SENTINEL = 0x5eed5eed
T, C, W, H = 24, 3, 64, 64  # triangles per frame, channels, frame size
PLANES4 = 2 * 4 * H * W * 4  # bytes of a visibility buffer of the two-frame sets = the largest buffer any call here names
GPOS = 2 * T * 9 * 4         # bytes of a position gradient
WRONG_SHARD = "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)"
ONLY_FUSED = "only SRZ_FUSED_CLEAR is accepted in flags"
N_CH = "n_ch must be 1 .. SRZ_ATTR_MAX_CH"
OUT_IN, OUT_OUT = "an output overlaps an input", "the two outputs overlap"
PLANES_16 = "the plane buffers must be 16-byte aligned"

# entry point -> its arguments after (ctx, fs), in order, each with the value of a valid call.  (name, offset): the address of a
# buffer of the kit plus `offset` bytes — vis: a visibility buffer; a, b: inputs of PLANES4 bytes; attr: [T][3][C] attributes;
# o1, o2: sentinel-filled outputs of PLANES4 + 256 bytes.
ENTRIES = {
    "shade_visibility": dict(vis=("vis", 0), out=("o1", 0), out_bytes=PLANES4, flags=F),
    "gbuffer": dict(vis=("vis", 0), out=("o1", 0), out_bytes=2 * 3 * H * W * 4, what=abi.GB_NORMAL, flags=F),
    "motion": dict(vis=("vis", 0), out=("o1", 0), out_bytes=2 * 2 * H * W * 4, what=abi.MV_FLOW, delta=1, flags=F),
    "interpolate": dict(vis=("vis", 0), attr=("attr", 0), n_ch=C, attr_frames=1, attr_tris=T, out=("o1", 0), out_bytes=2 * C * H * W * 4, flags=F),
    "interpolate_grad": dict(vis=("vis", 0), gout=("a", 0), attr=("attr", 0), n_ch=C, attr_frames=1, attr_tris=T, gattr=("o2", 0),
                             gbary=("o1", 0), flags=F),
    "position_grad": dict(vis=("vis", 0), gbary=("a", 0), gz=("b", 0), pos_tris=T, gpos=("o2", 0), gpix=("o1", 0), flags=F),
    "antialias": dict(vis=("vis", 0), cin=("a", 0), n_ch=C, out=("o1", 0), out_bytes=2 * C * H * W * 4, flags=F),
    "antialias_grad": dict(vis=("vis", 0), cin=("a", 0), gout=("b", 0), n_ch=C, gin=("o1", 0), pos_tris=T, gpos=("o2", 0), flags=F),
}

# (entry point, the faulty argument(s), code, text after "srz_frameset_<entry point>: "; WRONG_SHARD stands alone; None: no text is set).
# ctx: None, or "sharded" = a context under srz_set_shard(0, 2); fs: None, "uneven" = a set whose frames have 24 and 20 triangles,
# "sharded" = a set made under the sharded context.
CASES = [
    ("shade_visibility", dict(ctx=None), E, None),
    ("shade_visibility", dict(fs=None), E, "null frameset / visibility buffer / output"),
    ("shade_visibility", dict(vis=None), E, "null frameset / visibility buffer / output"),
    ("shade_visibility", dict(out=None), E, "null frameset / visibility buffer / output"),
    ("shade_visibility", dict(out_bytes=PLANES4 - 1), E, "output buffer too small"),
    ("shade_visibility", dict(vis=("vis", 4)), E, "buffers must be 16-byte aligned"),
    ("shade_visibility", dict(out=("o1", 8)), E, "buffers must be 16-byte aligned"),
    ("shade_visibility", dict(out=("vis", 64)), E, "visibility buffer and output overlap partly"),
    ("shade_visibility", dict(vis=("o1", 16)), E, "visibility buffer and output overlap partly"),
    ("shade_visibility", dict(ctx="sharded"), E, WRONG_SHARD),

    ("gbuffer", dict(ctx=None), E, None),
    ("gbuffer", dict(fs=None), E, "null frameset / visibility buffer / output"),
    ("gbuffer", dict(vis=None), E, "null frameset / visibility buffer / output"),
    ("gbuffer", dict(out=None), E, "null frameset / visibility buffer / output"),
    ("gbuffer", dict(what=0), E, "`what` names no group or an unknown one"),
    ("gbuffer", dict(what=16), E, "`what` names no group or an unknown one"),
    ("gbuffer", dict(flags=abi.UNIFIED), E, ONLY_FUSED),
    ("gbuffer", dict(out_bytes=2 * 3 * H * W * 4 - 1), E, "output buffer too small"),
    ("gbuffer", dict(vis=("vis", 8)), E, "buffers must be 16-byte aligned"),
    ("gbuffer", dict(out=("o1", 4)), E, "buffers must be 16-byte aligned"),
    ("gbuffer", dict(out=("vis", 0)), E, "the output overlaps the visibility buffer"),
    ("gbuffer", dict(out=("vis", PLANES4 - 16)), E, "the output overlaps the visibility buffer"),
    ("gbuffer", dict(ctx="sharded"), E, WRONG_SHARD),

    ("motion", dict(ctx=None), E, None),
    ("motion", dict(fs=None), E, "null frameset / visibility buffer / output"),
    ("motion", dict(vis=None), E, "null frameset / visibility buffer / output"),
    ("motion", dict(out=None), E, "null frameset / visibility buffer / output"),
    ("motion", dict(what=0), E, "`what` names no group or an unknown one"),
    ("motion", dict(what=8), E, "`what` names no group or an unknown one"),
    ("motion", dict(flags=F | abi.ORDERED_RASTER), E, ONLY_FUSED),
    ("motion", dict(ctx="sharded", fs="sharded", what=abi.MV_TARGET), E,
     "SRZ_MV_TARGET needs the whole frame on this ctx (the target row may belong to another rank)"),
    ("motion", dict(out_bytes=2 * 2 * H * W * 4 - 1), E, "output buffer too small"),
    ("motion", dict(vis=("vis", 4)), E, "buffers must be 16-byte aligned"),
    ("motion", dict(out=("o1", 12)), E, "buffers must be 16-byte aligned"),
    ("motion", dict(out=("vis", 0)), E, "the output overlaps the visibility buffer"),
    ("motion", dict(vis=("o1", 64)), E, "the output overlaps the visibility buffer"),
    ("motion", dict(fs="uneven"), E, "frames 0 and 1 differ in triangle count"),
    ("motion", dict(fs="uneven", delta=-1), E, "frames 1 and 0 differ in triangle count"),
    ("motion", dict(ctx="sharded"), E, WRONG_SHARD),

    ("interpolate", dict(ctx=None), E, None),
    ("interpolate", dict(fs=None), E, "null frameset / visibility buffer / attributes / output"),
    ("interpolate", dict(vis=None), E, "null frameset / visibility buffer / attributes / output"),
    ("interpolate", dict(attr=None), E, "null frameset / visibility buffer / attributes / output"),
    ("interpolate", dict(out=None), E, "null frameset / visibility buffer / attributes / output"),
    ("interpolate", dict(n_ch=0), E, N_CH),
    ("interpolate", dict(n_ch=65), E, N_CH),
    ("interpolate", dict(flags=abi.NO_Z_READBACK), E, ONLY_FUSED),
    ("interpolate", dict(attr_frames=3), E, "attr_frames must be 1 or the set's frame count"),
    ("interpolate", dict(attr_frames=0), E, "attr_frames must be 1 or the set's frame count"),
    ("interpolate", dict(attr_tris=T - 1), E, "attr_tris is below a frame's triangle count"),
    ("interpolate", dict(out_bytes=2 * C * H * W * 4 - 1), E, "output buffer too small"),
    ("interpolate", dict(vis=("vis", 8)), E, "buffers must be 16-byte aligned"),
    ("interpolate", dict(out=("o1", 4)), E, "buffers must be 16-byte aligned"),
    ("interpolate", dict(attr=("attr", 2)), E, "the attributes must be 4-byte aligned"),
    ("interpolate", dict(out=("vis", 32)), E, "the output overlaps the visibility buffer or the attributes"),
    ("interpolate", dict(out=("attr", 0)), E, "the output overlaps the visibility buffer or the attributes"),
    ("interpolate", dict(attr=("o1", 4)), E, "the output overlaps the visibility buffer or the attributes"),
    ("interpolate", dict(ctx="sharded"), E, WRONG_SHARD),

    ("interpolate_grad", dict(ctx=None), E, None),
    ("interpolate_grad", dict(fs=None), E, "null frameset / visibility buffer / output gradient"),
    ("interpolate_grad", dict(vis=None), E, "null frameset / visibility buffer / output gradient"),
    ("interpolate_grad", dict(gout=None), E, "null frameset / visibility buffer / output gradient"),
    ("interpolate_grad", dict(gattr=None, gbary=None), E, "neither d_gattr nor d_gbary is asked for"),
    ("interpolate_grad", dict(attr=None), E, "d_gbary needs the attributes"),
    ("interpolate_grad", dict(n_ch=0), E, N_CH),
    ("interpolate_grad", dict(flags=16), E, ONLY_FUSED),
    ("interpolate_grad", dict(attr_frames=3), E, "attr_frames must be 1 or the set's frame count"),
    ("interpolate_grad", dict(attr_tris=T - 1), E, "attr_tris is below a frame's triangle count"),
    ("interpolate_grad", dict(vis=("vis", 4)), E, PLANES_16),
    ("interpolate_grad", dict(gout=("a", 8)), E, PLANES_16),
    ("interpolate_grad", dict(gbary=("o1", 4)), E, PLANES_16),
    ("interpolate_grad", dict(attr=("attr", 2)), E, "attributes and their gradient must be 4-byte aligned"),
    ("interpolate_grad", dict(gattr=("o2", 2)), E, "attributes and their gradient must be 4-byte aligned"),
    ("interpolate_grad", dict(gattr=("vis", 4)), E, OUT_IN),
    ("interpolate_grad", dict(gattr=("a", 4)), E, OUT_IN),
    ("interpolate_grad", dict(gattr=("attr", 4)), E, OUT_IN),
    ("interpolate_grad", dict(gbary=("vis", 16)), E, OUT_IN),
    ("interpolate_grad", dict(gbary=("a", 2 * C * H * W * 4 - 16)), E, OUT_IN),
    ("interpolate_grad", dict(gbary=("attr", 0)), E, OUT_IN),
    ("interpolate_grad", dict(gout=("o1", 16)), E, OUT_IN),
    ("interpolate_grad", dict(gattr=("o1", 2 * 2 * H * W * 4 - 4)), E, OUT_OUT),
    ("interpolate_grad", dict(gbary=("o2", 16)), E, OUT_OUT),
    ("interpolate_grad", dict(ctx="sharded"), E, WRONG_SHARD),

    ("position_grad", dict(ctx=None), E, None),
    ("position_grad", dict(fs=None), E, "null frameset / visibility buffer"),
    ("position_grad", dict(vis=None), E, "null frameset / visibility buffer"),
    ("position_grad", dict(gbary=None, gz=None), E, "neither d_gbary nor d_gz is given"),
    ("position_grad", dict(gpos=None, gpix=None), E, "neither d_gpos nor d_gpix is asked for"),
    ("position_grad", dict(flags=abi.UNIFIED), E, ONLY_FUSED),
    ("position_grad", dict(pos_tris=T - 1), E, "pos_tris is below a frame's triangle count"),
    ("position_grad", dict(vis=("vis", 4)), E, PLANES_16),
    ("position_grad", dict(gbary=("a", 4)), E, PLANES_16),
    ("position_grad", dict(gz=("b", 8)), E, PLANES_16),
    ("position_grad", dict(gpix=("o1", 4)), E, PLANES_16),
    ("position_grad", dict(gpos=("o2", 2)), E, "the position gradient must be 4-byte aligned"),
    ("position_grad", dict(gpos=("vis", 4)), E, OUT_IN),
    ("position_grad", dict(gpos=("a", 4)), E, OUT_IN),
    ("position_grad", dict(gpos=("b", 4)), E, OUT_IN),
    ("position_grad", dict(gpix=("vis", 16)), E, OUT_IN),
    ("position_grad", dict(gpix=("a", 16)), E, OUT_IN),
    ("position_grad", dict(gpix=("b", H * W * 4 * 2 - 16)), E, OUT_IN),
    ("position_grad", dict(gz=("o2", GPOS - 16)), E, OUT_IN),
    ("position_grad", dict(gpos=("o1", 2 * 2 * H * W * 4 - 4)), E, OUT_OUT),
    ("position_grad", dict(gpix=("o2", 16)), E, OUT_OUT),
    ("position_grad", dict(ctx="sharded"), E, WRONG_SHARD),

    ("antialias", dict(ctx=None), E, None),
    ("antialias", dict(fs=None), E, "null frameset / visibility buffer / input / output"),
    ("antialias", dict(vis=None), E, "null frameset / visibility buffer / input / output"),
    ("antialias", dict(cin=None), E, "null frameset / visibility buffer / input / output"),
    ("antialias", dict(out=None), E, "null frameset / visibility buffer / input / output"),
    ("antialias", dict(n_ch=0), E, N_CH),
    ("antialias", dict(n_ch=65), E, N_CH),
    ("antialias", dict(flags=F | abi.UNIFIED), E, ONLY_FUSED),
    ("antialias", dict(ctx="sharded", fs="sharded"), E,
     "needs the whole frame on this ctx (a vertical pair across a band edge needs another rank's rows)"),
    ("antialias", dict(out_bytes=2 * C * H * W * 4 - 1), E, "output buffer too small"),
    ("antialias", dict(vis=("vis", 4)), E, "buffers must be 16-byte aligned"),
    ("antialias", dict(cin=("a", 8)), E, "buffers must be 16-byte aligned"),
    ("antialias", dict(out=("o1", 4)), E, "buffers must be 16-byte aligned"),
    ("antialias", dict(out=("vis", 64)), E, "the output overlaps the visibility buffer or the input (the pass reads neighbours: not in place)"),
    ("antialias", dict(out=("a", 0)), E, "the output overlaps the visibility buffer or the input (the pass reads neighbours: not in place)"),
    ("antialias", dict(cin=("o1", 16)), E, "the output overlaps the visibility buffer or the input (the pass reads neighbours: not in place)"),
    ("antialias", dict(ctx="sharded"), E, WRONG_SHARD),

    ("antialias_grad", dict(ctx=None), E, None),
    ("antialias_grad", dict(fs=None), E, "null frameset / visibility buffer / input / output gradient"),
    ("antialias_grad", dict(vis=None), E, "null frameset / visibility buffer / input / output gradient"),
    ("antialias_grad", dict(cin=None), E, "null frameset / visibility buffer / input / output gradient"),
    ("antialias_grad", dict(gout=None), E, "null frameset / visibility buffer / input / output gradient"),
    ("antialias_grad", dict(gin=None, gpos=None), E, "neither d_gin nor d_gpos is asked for"),
    ("antialias_grad", dict(n_ch=65), E, N_CH),
    ("antialias_grad", dict(flags=abi.ORDERED_RASTER), E, ONLY_FUSED),
    ("antialias_grad", dict(ctx="sharded", fs="sharded"), E,
     "needs the whole frame on this ctx (a vertical pair across a band edge needs another rank's rows)"),
    ("antialias_grad", dict(pos_tris=T - 1), E, "pos_tris is below a frame's triangle count"),
    ("antialias_grad", dict(vis=("vis", 4)), E, PLANES_16),
    ("antialias_grad", dict(cin=("a", 4)), E, PLANES_16),
    ("antialias_grad", dict(gout=("b", 8)), E, PLANES_16),
    ("antialias_grad", dict(gin=("o1", 4)), E, PLANES_16),
    ("antialias_grad", dict(gpos=("o2", 2)), E, "the position gradient must be 4-byte aligned"),
    ("antialias_grad", dict(gin=("vis", 16)), E, OUT_IN),
    ("antialias_grad", dict(gin=("a", 16)), E, OUT_IN),
    ("antialias_grad", dict(gin=("b", 2 * C * H * W * 4 - 16)), E, OUT_IN),
    ("antialias_grad", dict(gpos=("vis", 4)), E, OUT_IN),
    ("antialias_grad", dict(gpos=("a", 4)), E, OUT_IN),
    ("antialias_grad", dict(gpos=("b", 4)), E, OUT_IN),
    ("antialias_grad", dict(cin=("o2", GPOS - 16)), E, OUT_IN),
    ("antialias_grad", dict(gpos=("o1", 2 * C * H * W * 4 - 4)), E, OUT_OUT),
    ("antialias_grad", dict(gin=("o2", 16)), E, OUT_OUT),
    ("antialias_grad", dict(ctx="sharded"), E, WRONG_SHARD),
]


def case_id(case):
    entry, fault, _, _ = case
    return entry + ":" + ",".join(f"{k}={'+'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in fault.items())


assert len({case_id(c) for c in CASES}) == len(CASES)


@pytest.fixture(scope="module")
def kit():
    """the contexts, sets and buffers every case draws its arguments from"""
    tris = soup(3, T, W, H, (10.0, 20.0, 30.0))
    main, sharded = srz.Context(0), srz.Context(0, 0, 2)
    k = types.SimpleNamespace(ctx={"main": main, "sharded": sharded})
    k.fs = {"main": main.frameset([frame(tris, W, H), frame(tris[::-1].copy(), W, H)]),
            "uneven": main.frameset([frame(tris, W, H), frame(tris[:T - 4], W, H)]),
            "sharded": sharded.frameset([frame(tris, W, H), frame(tris, W, H)])}
    vis = torch.zeros(k.fs["main"].out_shape, dtype=torch.float32, device="cuda")
    assert vis.numel() * 4 == PLANES4 == k.fs["main"].out_bytes
    k.fs["main"].render_visibility(vis.data_ptr(), PLANES4, F, stream())
    torch.cuda.synchronize()
    k.buf = {"vis": vis, "a": torch.zeros(PLANES4 // 4, dtype=torch.int32, device="cuda"),
             "b": torch.zeros(PLANES4 // 4, dtype=torch.int32, device="cuda"),
             "attr": torch.zeros(T * 3 * C, dtype=torch.int32, device="cuda"),
             "o1": torch.full((PLANES4 // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda"),
             "o2": torch.full((PLANES4 // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda")}
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
    entry, fault, code, text = case
    L = srz.lib()
    # every context's text is first set to another refusal's, so that a stale text cannot stand in for the one expected
    marker = "srz_frameset_render: null frameset / output"
    for c in kit.ctx.values():
        assert L.srz_frameset_render(c.h, None, None, 0, 0, None) == E and L.srz_last_error(c.h).decode() == marker
    created = L.srz_last_error(None)
    rc, h = call(kit, entry, fault)
    assert rc == code, (rc, L.srz_last_error(h))
    if text is None:  # (no context to leave a text in: nobody's text changes)
        assert h is None and L.srz_last_error(None) == created
        assert all(L.srz_last_error(c.h).decode() == marker for c in kit.ctx.values())
    else:
        assert L.srz_last_error(h).decode() == (text if text is WRONG_SHARD else f"srz_frameset_{entry}: {text}")
    torch.cuda.synchronize()
    for name, t in kit.buf.items():
        assert torch.equal(t, kit.before[name]), f"{name} was written"


def test_the_valid_calls_are_accepted(kit):
    """ENTRIES' arguments are a valid call of every entry point: the refusals above are each due to the one argument their row changes"""
    for entry in ENTRIES:
        rc, h = call(kit, entry, {})
        assert rc == 0, (entry, srz.lib().srz_last_error(h))
    torch.cuda.synchronize()
    for name, t in kit.buf.items():  # (the outputs are written now: the sentinels go back for whatever runs next)
        t.copy_(kit.before[name])
