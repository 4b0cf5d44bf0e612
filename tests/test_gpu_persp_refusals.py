"""-m gpu: what srz_frameset_perspective, _perspective_grad and _interpolate_deriv_persp refuse, and in which words.  One call per row
of CASES: every argument is valid but the one the row names, so the call has exactly one fault; it must return SRZ_E_INVALID, leave
the row's text in srz_last_error, and touch no buffer.  Nothing reaches a kernel: every call is refused on the host.
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
T, C, W, H = 24, 3, 64, 64  # triangles per frame, channels, frame size
PLANES4 = 2 * 4 * H * W * 4  # bytes of a visibility buffer of the two-frame set
PLANES2 = 2 * 2 * H * W * 4  # bytes of the gradient planes
PLANES6 = 2 * 2 * C * H * W * 4  # bytes of the derivative planes at C = 3
QB = T * 3 * 4               # bytes of one frame's q
WRONG_SHARD = "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)"
ONLY_FUSED = ": only SRZ_FUSED_CLEAR is accepted in flags"
Q_FRAMES, Q_TRIS = ": q_frames must be 1 or the set's frame count", ": q_tris is below a frame's triangle count"
FWD_NULL, FWD_16, FWD_OVER = ": null frameset / visibility buffer / q / output", ": buffers must be 16-byte aligned", ": the output overlaps the visibility buffer or q"
BWD_NULL, BWD_16 = ": null frameset / visibility buffer / q / gradient planes", ": the plane buffers must be 16-byte aligned"
BWD_4, OUT_IN, OUT_OUT = ": q and its gradient must be 4-byte aligned", ": an output overlaps an input", ": the two outputs overlap"
DRV_NULL, DRV_OVER = ": null frameset / visibility buffer / q / attributes / output", ": the output overlaps the visibility buffer, the attributes or q"
DRV_4, SMALL = ": the attributes and q must be 4-byte aligned", ": output buffer too small"

# entry point -> its arguments after (ctx, fs), in order, each with the value of a valid call.  (name, offset): the address of a
# buffer of the kit plus `offset` bytes — vis: a visibility buffer; q: two frames of q; g: gradient planes; attr: two frames of
# attributes; o1, o2: sentinel-filled outputs of PLANES6 + 256 bytes (the largest output any call here names, and room to spare).
ENTRIES = {
    "perspective": dict(vis=("vis", 0), q=("q", 0), q_frames=1, q_tris=T, out=("o1", 0), out_bytes=PLANES4, flags=F),
    "perspective_grad": dict(vis=("vis", 0), q=("q", 0), q_frames=1, q_tris=T, gbp=("g", 0), gbary=("o1", 0), gq=("o2", 0), flags=F),
    "interpolate_deriv_persp": dict(vis=("vis", 0), q=("q", 0), q_frames=1, q_tris=T, attr=("attr", 0), n_ch=C, attr_frames=1, attr_tris=T,
                                    out=("o1", 0), out_bytes=PLANES6, flags=F),
}

CASES = [
    ("perspective", dict(ctx=None), None),
    ("perspective", dict(fs=None), FWD_NULL),
    ("perspective", dict(vis=None), FWD_NULL),
    ("perspective", dict(q=None), FWD_NULL),
    ("perspective", dict(out=None), FWD_NULL),
    ("perspective", dict(q_frames=0), Q_FRAMES),
    ("perspective", dict(q_frames=3), Q_FRAMES),
    ("perspective", dict(q_tris=T - 1), Q_TRIS),
    ("perspective", dict(out_bytes=PLANES4 - 1), SMALL),
    ("perspective", dict(flags=abi.UNIFIED), ONLY_FUSED),
    ("perspective", dict(flags=F | abi.ORDERED_RASTER), ONLY_FUSED),
    ("perspective", dict(vis=("vis", 4)), FWD_16),
    ("perspective", dict(out=("o1", 4)), FWD_16),
    ("perspective", dict(q=("q", 2)), ": q must be 4-byte aligned"),
    ("perspective", dict(out=("vis", 0)), FWD_OVER),  # in place is an overlap
    ("perspective", dict(out=("vis", 64)), FWD_OVER),
    ("perspective", dict(q=("o1", 4)), FWD_OVER),
    ("perspective", dict(ctx="sharded"), WRONG_SHARD),

    ("perspective_grad", dict(ctx=None), None),
    ("perspective_grad", dict(fs=None), BWD_NULL),
    ("perspective_grad", dict(vis=None), BWD_NULL),
    ("perspective_grad", dict(q=None), BWD_NULL),
    ("perspective_grad", dict(gbp=None), BWD_NULL),
    ("perspective_grad", dict(gbary=None, gq=None), ": neither d_gbary nor d_gq is asked for"),
    ("perspective_grad", dict(q_frames=0), Q_FRAMES),
    ("perspective_grad", dict(q_frames=3), Q_FRAMES),
    ("perspective_grad", dict(q_tris=T - 1), Q_TRIS),
    ("perspective_grad", dict(flags=16), ONLY_FUSED),
    ("perspective_grad", dict(vis=("vis", 4)), BWD_16),
    ("perspective_grad", dict(gbp=("g", 8)), BWD_16),
    ("perspective_grad", dict(gbary=("o1", 4)), BWD_16),
    ("perspective_grad", dict(q=("q", 2)), BWD_4),
    ("perspective_grad", dict(gq=("o2", 2)), BWD_4),
    ("perspective_grad", dict(gq=("vis", 4)), OUT_IN),
    ("perspective_grad", dict(gq=("g", 4)), OUT_IN),
    ("perspective_grad", dict(gq=("q", QB - 4)), OUT_IN),
    ("perspective_grad", dict(gbary=("vis", 16)), OUT_IN),
    ("perspective_grad", dict(gbary=("g", 0)), OUT_IN),
    ("perspective_grad", dict(gbp=("o1", PLANES2 - 16)), OUT_IN),
    ("perspective_grad", dict(q=("o1", 4)), OUT_IN),
    ("perspective_grad", dict(gq=("o1", PLANES2 - 4)), OUT_OUT),
    ("perspective_grad", dict(gbary=("o2", 16)), OUT_OUT),
    ("perspective_grad", dict(ctx="sharded"), WRONG_SHARD),

    ("interpolate_deriv_persp", dict(ctx=None), None),
    ("interpolate_deriv_persp", dict(fs=None), DRV_NULL),
    ("interpolate_deriv_persp", dict(vis=None), DRV_NULL),
    ("interpolate_deriv_persp", dict(q=None), DRV_NULL),
    ("interpolate_deriv_persp", dict(attr=None), DRV_NULL),
    ("interpolate_deriv_persp", dict(out=None), DRV_NULL),
    ("interpolate_deriv_persp", dict(n_ch=0), ": n_ch must be 1 .. SRZ_ATTR_MAX_CH"),
    ("interpolate_deriv_persp", dict(n_ch=abi.ATTR_MAX_CH // 2 + 1), ": n_ch must be 1 .. SRZ_ATTR_MAX_CH / 2"),
    ("interpolate_deriv_persp", dict(attr_frames=3), ": attr_frames must be 1 or the set's frame count"),
    ("interpolate_deriv_persp", dict(attr_tris=T - 1), ": attr_tris is below a frame's triangle count"),
    ("interpolate_deriv_persp", dict(q_frames=0), Q_FRAMES),
    ("interpolate_deriv_persp", dict(q_frames=3), Q_FRAMES),
    ("interpolate_deriv_persp", dict(q_tris=T - 1), Q_TRIS),
    ("interpolate_deriv_persp", dict(out_bytes=PLANES6 - 1), SMALL),
    ("interpolate_deriv_persp", dict(flags=abi.UNIFIED), ONLY_FUSED),
    ("interpolate_deriv_persp", dict(vis=("vis", 4)), FWD_16),
    ("interpolate_deriv_persp", dict(out=("o1", 8)), FWD_16),
    ("interpolate_deriv_persp", dict(attr=("attr", 2)), DRV_4),
    ("interpolate_deriv_persp", dict(q=("q", 2)), DRV_4),
    ("interpolate_deriv_persp", dict(out=("vis", 64)), DRV_OVER),
    ("interpolate_deriv_persp", dict(attr=("o1", 4)), DRV_OVER),
    ("interpolate_deriv_persp", dict(q=("o1", PLANES6 - 4)), DRV_OVER),
    ("interpolate_deriv_persp", dict(ctx="sharded"), WRONG_SHARD),
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
    assert vis.numel() * 4 == PLANES4 == k.fs["main"].out_bytes and k.fs["main"].interpolate_bytes(2) == PLANES2
    assert k.fs["main"].interpolate_bytes(2 * C) == PLANES6
    k.fs["main"].render_visibility(vis.data_ptr(), PLANES4, F, stream())
    torch.cuda.synchronize()
    k.buf = {"vis": vis, "q": torch.ones(2 * QB // 4 + 4, dtype=torch.float32, device="cuda"),
             "g": torch.ones(PLANES4 // 4, dtype=torch.float32, device="cuda"),
             "attr": torch.ones(2 * T * 3 * C + 4, dtype=torch.float32, device="cuda"),
             "o1": torch.full((PLANES6 // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda"),
             "o2": torch.full((PLANES6 // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda")}
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
    """ENTRIES' arguments are a valid call of every entry point, and so are the calls that leave out what may be left out: the
    refusals above are each due to the one argument their row changes"""
    kit.buf["o2"].zero_()  # (d_gq is added into: the sentinel, 2e18 as a float, would swallow the adds)
    for entry, fault in (("perspective", {}), ("perspective", dict(q_frames=2)), ("perspective_grad", {}),
                         ("perspective_grad", dict(gbary=None)), ("perspective_grad", dict(gq=None)), ("perspective_grad", dict(q_frames=2)),
                         ("interpolate_deriv_persp", {}), ("interpolate_deriv_persp", dict(q_frames=2, attr_frames=2))):
        rc, h = call(kit, entry, fault)
        assert rc == 0, (entry, fault, srz.lib().srz_last_error(h))
    torch.cuda.synchronize()
    assert not torch.equal(kit.buf["o1"], kit.before["o1"]) and bool(kit.buf["o2"].any())
    for name, t in kit.buf.items():  # (the outputs are written now: the sentinels go back for whatever runs next)
        t.copy_(kit.before[name])
