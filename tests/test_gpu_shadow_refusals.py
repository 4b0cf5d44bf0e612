"""-m gpu: what srz_frameset_shadow and _shadow_grad refuse, and in which words.  One call per row of CASES: every argument is valid
but the one the row names, so the call has exactly one fault; it must return SRZ_E_INVALID, leave the row's text — which names the
argument — in srz_last_error, and touch no buffer.  Nothing reaches a kernel: every call is refused on the host.
(tests/test_gpu_cube_refusals.py's scheme.)"""
import types

import pytest
import torch

import srz
from srz import abi
from support import frame, soup, stream

pytestmark = pytest.mark.gpu

F, E = abi.FUSED_CLEAR, abi.SRZ_E_INVALID
SENTINEL = 0x5eed5eed
T, W, H, MW, MH = 24, 64, 64, 8, 6  # triangles per frame, frame size, map size
PLANES4 = 2 * 4 * H * W * 4  # bytes of a visibility buffer of the two-frame set = the largest buffer any call here names
PLANES3 = 2 * 3 * H * W * 4  # bytes of the coordinate planes and of d_gsc
PLANES1 = 2 * 1 * H * W * 4  # bytes of d_out and d_gout
MAP = MW * MH * 4            # bytes of one map
NAN, INF = float("nan"), float("inf")
WRONG_SHARD = "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)"
ONLY_FUSED = "only SRZ_FUSED_CLEAR is accepted in flags"
MAP_SIZE, MAP_FRAMES = "map_w and map_h must be 1 .. SRZ_TEX_MAX_SIZE", "map_frames must be 1 or the set's frame count"
FINITE, NEGATIVE = "bias and width must be finite", "width must be >= 0 (0: the hard test)"
FWD_16, FWD_OVER = "the plane buffers (d_vis, d_sc, d_out) must be 16-byte aligned", "d_out overlaps d_vis, d_sc or d_map"
BWD_16 = "the plane buffers (d_vis, d_sc, d_gout, d_gsc) must be 16-byte aligned"
BWD_4 = "d_map and d_gmap must be 4-byte aligned"
BWD_NAMES = " (d_gmap, d_gsc against d_vis, d_sc, d_gout, d_map)"
OUT_IN, OUT_OUT = "an output overlaps an input", "the two outputs overlap"

# entry point -> its arguments after (ctx, fs), in order, each with the value of a valid call.  (name, offset): the address of a
# buffer of the kit plus `offset` bytes — vis: a visibility buffer; sc, g: inputs of PLANES4 bytes; map: two maps; o1, o2:
# sentinel-filled outputs of PLANES4 + 256 bytes.
ENTRIES = {
    "shadow": dict(vis=("vis", 0), sc=("sc", 0), map=("map", 0), map_w=MW, map_h=MH, map_frames=1, bias=0.25, width=1.0, out=("o1", 0),
                   out_bytes=PLANES1, flags=F),
    "shadow_grad": dict(vis=("vis", 0), sc=("sc", 0), gout=("g", 0), map=("map", 0), map_w=MW, map_h=MH, map_frames=1, bias=0.25, width=1.0,
                        gmap=("o2", 0), gsc=("o1", 0), flags=F),
}

# (entry point, the faulty argument(s), text after "srz_frameset_<entry point>"; WRONG_SHARD stands alone; None: no text is set)
CASES = [
    ("shadow", dict(ctx=None), None),
    ("shadow", dict(fs=None), ": null frameset"),
    ("shadow", dict(vis=None), ": null d_vis"),
    ("shadow", dict(sc=None), ": null d_sc"),
    ("shadow", dict(map=None), ": null d_map"),
    ("shadow", dict(out=None), ": null d_out"),
    ("shadow", dict(map_w=0), ": " + MAP_SIZE),
    ("shadow", dict(map_h=0), ": " + MAP_SIZE),
    ("shadow", dict(map_w=abi.TEX_MAX_SIZE + 1), ": " + MAP_SIZE),
    ("shadow", dict(map_h=abi.TEX_MAX_SIZE + 1), ": " + MAP_SIZE),
    ("shadow", dict(map_frames=0), ": " + MAP_FRAMES),
    ("shadow", dict(map_frames=3), ": " + MAP_FRAMES),
    ("shadow", dict(bias=NAN), ": " + FINITE),
    ("shadow", dict(bias=INF), ": " + FINITE),
    ("shadow", dict(bias=-INF), ": " + FINITE),
    ("shadow", dict(width=NAN), ": " + FINITE),
    ("shadow", dict(width=INF), ": " + FINITE),
    ("shadow", dict(width=-INF), ": " + FINITE),
    ("shadow", dict(width=-1.0), ": " + NEGATIVE),
    ("shadow", dict(width=-1e-40), ": " + NEGATIVE),
    ("shadow", dict(out_bytes=PLANES1 - 1), ": out_bytes is too small for d_out"),
    ("shadow", dict(flags=abi.UNIFIED), ": " + ONLY_FUSED),
    ("shadow", dict(flags=F | abi.ORDERED_RASTER), ": " + ONLY_FUSED),
    ("shadow", dict(vis=("vis", 4)), ": " + FWD_16),
    ("shadow", dict(sc=("sc", 8)), ": " + FWD_16),
    ("shadow", dict(out=("o1", 4)), ": " + FWD_16),
    ("shadow", dict(map=("map", 2)), ": d_map must be 4-byte aligned"),
    ("shadow", dict(out=("vis", 64)), ": " + FWD_OVER),
    ("shadow", dict(out=("sc", 0)), ": " + FWD_OVER),
    ("shadow", dict(out=("map", 0)), ": " + FWD_OVER),
    ("shadow", dict(sc=("o1", PLANES1 - 16)), ": " + FWD_OVER),
    ("shadow", dict(map=("o1", 4)), ": " + FWD_OVER),
    ("shadow", dict(ctx="sharded"), WRONG_SHARD),

    ("shadow_grad", dict(ctx=None), None),
    ("shadow_grad", dict(fs=None), ": null frameset"),
    ("shadow_grad", dict(vis=None), ": null d_vis"),
    ("shadow_grad", dict(sc=None), ": null d_sc"),
    ("shadow_grad", dict(gout=None), ": null d_gout"),
    ("shadow_grad", dict(map=None), ": null d_map"),
    ("shadow_grad", dict(gmap=None, gsc=None), ": neither d_gmap nor d_gsc is asked for"),
    ("shadow_grad", dict(map_w=0), ": " + MAP_SIZE),
    ("shadow_grad", dict(map_h=abi.TEX_MAX_SIZE + 1), ": " + MAP_SIZE),
    ("shadow_grad", dict(map_frames=0), ": " + MAP_FRAMES),
    ("shadow_grad", dict(map_frames=3), ": " + MAP_FRAMES),
    ("shadow_grad", dict(bias=NAN), ": " + FINITE),
    ("shadow_grad", dict(bias=-INF), ": " + FINITE),
    ("shadow_grad", dict(width=NAN), ": " + FINITE),
    ("shadow_grad", dict(width=INF), ": " + FINITE),
    ("shadow_grad", dict(width=-0.5), ": " + NEGATIVE),
    ("shadow_grad", dict(flags=16), ": " + ONLY_FUSED),
    ("shadow_grad", dict(flags=F | abi.UNIFIED), ": " + ONLY_FUSED),
    ("shadow_grad", dict(vis=("vis", 4)), ": " + BWD_16),
    ("shadow_grad", dict(sc=("sc", 4)), ": " + BWD_16),
    ("shadow_grad", dict(gout=("g", 8)), ": " + BWD_16),
    ("shadow_grad", dict(gsc=("o1", 4)), ": " + BWD_16),
    ("shadow_grad", dict(map=("map", 2)), ": " + BWD_4),
    ("shadow_grad", dict(gmap=("o2", 2)), ": " + BWD_4),
    ("shadow_grad", dict(gmap=("vis", 4)), BWD_NAMES + ": " + OUT_IN),
    ("shadow_grad", dict(gmap=("sc", 4)), BWD_NAMES + ": " + OUT_IN),
    ("shadow_grad", dict(gmap=("g", 4)), BWD_NAMES + ": " + OUT_IN),
    ("shadow_grad", dict(gmap=("map", MAP - 4)), BWD_NAMES + ": " + OUT_IN),
    ("shadow_grad", dict(gsc=("vis", 16)), BWD_NAMES + ": " + OUT_IN),
    ("shadow_grad", dict(gsc=("sc", PLANES3 - 16)), BWD_NAMES + ": " + OUT_IN),
    ("shadow_grad", dict(gsc=("g", 0)), BWD_NAMES + ": " + OUT_IN),
    ("shadow_grad", dict(gsc=("map", 0)), BWD_NAMES + ": " + OUT_IN),
    ("shadow_grad", dict(gout=("o1", 16)), BWD_NAMES + ": " + OUT_IN),
    ("shadow_grad", dict(gmap=("o1", PLANES3 - 4)), BWD_NAMES + ": " + OUT_OUT),
    ("shadow_grad", dict(gsc=("o2", 16)), BWD_NAMES + ": " + OUT_OUT),
    ("shadow_grad", dict(ctx="sharded"), WRONG_SHARD),
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
    vis = torch.zeros(k.fs["main"].out_shape, dtype=torch.float32, device="cuda")
    assert vis.numel() * 4 == PLANES4 == k.fs["main"].out_bytes and k.fs["main"].interpolate_bytes(3) == PLANES3
    assert k.fs["main"].interpolate_bytes(1) == PLANES1
    k.fs["main"].render_visibility(vis.data_ptr(), PLANES4, F, stream())
    torch.cuda.synchronize()
    # sc = (1, 1, 1) against a map of ones with bias 0.25 and width 1: every corner sits on the ramp, so a valid call adds to d_gmap
    k.buf = {"vis": vis, "sc": torch.ones(PLANES4 // 4, dtype=torch.float32, device="cuda"),
             "g": torch.ones(PLANES4 // 4, dtype=torch.float32, device="cuda"),
             "map": torch.ones(2 * MAP // 4, dtype=torch.float32, device="cuda"),
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
    entry, fault, text = case
    L = srz.lib()
    # every context's text is first set to another refusal's, so that a stale text cannot stand in for the one expected
    marker = "srz_frameset_render: null frameset / output"
    for c in kit.ctx.values():
        assert L.srz_frameset_render(c.h, None, None, 0, 0, None) == E and L.srz_last_error(c.h).decode() == marker
    created = L.srz_last_error(None)
    rc, h = call(kit, entry, fault)
    assert rc == E, (rc, L.srz_last_error(h))
    if text is None:  # (no context to leave a text in: nobody's text changes)
        assert h is None and L.srz_last_error(None) == created
        assert all(L.srz_last_error(c.h).decode() == marker for c in kit.ctx.values())
    else:
        assert L.srz_last_error(h).decode() == (text if text is WRONG_SHARD else f"srz_frameset_{entry}{text}")
    torch.cuda.synchronize()
    for name, t in kit.buf.items():
        assert torch.equal(t, kit.before[name]), f"{name} was written"


def test_the_valid_calls_are_accepted(kit):
    """ENTRIES' arguments are a valid call of both entry points, and so are the calls that leave out what may be left out and the hard
    test with d_gmap given: the refusals above are each due to the one argument their row changes.  This runs after them: a valid
    call still works behind every refusal"""
    kit.buf["o2"].zero_()  # (d_gmap is added into: the sentinel, 2e18 as a float, would swallow the adds)
    for entry, fault in (("shadow", {}), ("shadow", dict(map_frames=2)), ("shadow", dict(width=0.0)), ("shadow", dict(flags=0)),
                         ("shadow_grad", {}), ("shadow_grad", dict(gsc=None)), ("shadow_grad", dict(gmap=None)),
                         ("shadow_grad", dict(map_frames=2)), ("shadow_grad", dict(width=0.0))):
        rc, h = call(kit, entry, fault)
        assert rc == 0, (entry, fault, srz.lib().srz_last_error(h))
    torch.cuda.synchronize()
    assert not torch.equal(kit.buf["o1"], kit.before["o1"]) and bool(kit.buf["o2"].any())
    for name, t in kit.buf.items():  # (the outputs are written now: the sentinels go back for whatever runs next)
        t.copy_(kit.before[name])
