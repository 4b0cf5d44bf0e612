"""-m gpu: what srz_frameset_texture_cube and _texture_cube_grad refuse, and in which words.  One call per row of CASES: every
argument is valid but the one the row names, so the call has exactly one fault; it must return SRZ_E_INVALID, leave the row's text —
which names the argument — in srz_last_error, and touch no buffer.  Nothing reaches a kernel: every call is refused on the host.
(tests/test_gpu_pass_refusals.py's scheme.)"""
import types

import pytest
import torch

import srz
from srz import abi
from support import frame, soup, stream

pytestmark = pytest.mark.gpu

F, E = abi.FUSED_CLEAR, abi.SRZ_E_INVALID
SENTINEL = 0x5eed5eed
T, C, W, H, N = 24, 3, 64, 64, 8  # triangles per frame, channels, frame size, cube size
PLANES4 = 2 * 4 * H * W * 4  # bytes of a visibility buffer of the two-frame set = the largest buffer any call here names
PLANES3 = 2 * 3 * H * W * 4  # bytes of the direction planes, and of the output at C = 3
CUBE = 6 * N * N * C * 4     # bytes of one cube
WRONG_SHARD = "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)"
ONLY_FUSED = "only SRZ_FUSED_CLEAR is accepted in flags"
N_CH, N_SIZE = "n_ch must be 1 .. SRZ_ATTR_MAX_CH", "n must be 1 .. SRZ_TEX_MAX_SIZE"
TEX_FRAMES = "tex_frames must be 1 or the set's frame count"
FWD_16, FWD_OVER = "the plane buffers (d_vis, d_dir, d_out) must be 16-byte aligned", "d_out overlaps d_vis, d_dir or d_tex"
BWD_16 = "the plane buffers (d_vis, d_dir, d_gout, d_gdir) must be 16-byte aligned"
BWD_NAMES = " (d_gtex, d_gdir against d_vis, d_dir, d_gout, d_tex)"
OUT_IN, OUT_OUT = "an output overlaps an input", "the two outputs overlap"

# entry point -> its arguments after (ctx, fs), in order, each with the value of a valid call.  (name, offset): the address of a
# buffer of the kit plus `offset` bytes — vis: a visibility buffer; dir, g: inputs of PLANES4 bytes; tex: two cubes; o1, o2:
# sentinel-filled outputs of PLANES4 + 256 bytes.
ENTRIES = {
    "texture_cube": dict(vis=("vis", 0), dir=("dir", 0), tex=("tex", 0), n=N, n_ch=C, tex_frames=1, out=("o1", 0), out_bytes=PLANES3, flags=F),
    "texture_cube_grad": dict(vis=("vis", 0), dir=("dir", 0), gout=("g", 0), tex=("tex", 0), n=N, n_ch=C, tex_frames=1, gtex=("o2", 0),
                              gdir=("o1", 0), flags=F),
}

# (entry point, the faulty argument(s), text after "srz_frameset_<entry point>"; WRONG_SHARD stands alone; None: no text is set)
CASES = [
    ("texture_cube", dict(ctx=None), None),
    ("texture_cube", dict(fs=None), ": null frameset"),
    ("texture_cube", dict(vis=None), ": null d_vis"),
    ("texture_cube", dict(dir=None), ": null d_dir"),
    ("texture_cube", dict(tex=None), ": null d_tex"),
    ("texture_cube", dict(out=None), ": null d_out"),
    ("texture_cube", dict(n=0), ": " + N_SIZE),
    ("texture_cube", dict(n=abi.TEX_MAX_SIZE + 1), ": " + N_SIZE),
    ("texture_cube", dict(n_ch=0), ": " + N_CH),
    ("texture_cube", dict(n_ch=abi.ATTR_MAX_CH + 1), ": " + N_CH),
    ("texture_cube", dict(tex_frames=0), ": " + TEX_FRAMES),
    ("texture_cube", dict(tex_frames=3), ": " + TEX_FRAMES),
    ("texture_cube", dict(out_bytes=PLANES3 - 1), ": out_bytes is too small for d_out"),
    ("texture_cube", dict(flags=abi.UNIFIED), ": " + ONLY_FUSED),
    ("texture_cube", dict(flags=F | abi.ORDERED_RASTER), ": " + ONLY_FUSED),
    ("texture_cube", dict(vis=("vis", 4)), ": " + FWD_16),
    ("texture_cube", dict(dir=("dir", 8)), ": " + FWD_16),
    ("texture_cube", dict(out=("o1", 4)), ": " + FWD_16),
    ("texture_cube", dict(tex=("tex", 2)), ": d_tex must be 4-byte aligned"),
    ("texture_cube", dict(out=("vis", 64)), ": " + FWD_OVER),
    ("texture_cube", dict(out=("dir", 0)), ": " + FWD_OVER),
    ("texture_cube", dict(out=("tex", 0)), ": " + FWD_OVER),
    ("texture_cube", dict(dir=("o1", PLANES3 - 16)), ": " + FWD_OVER),
    ("texture_cube", dict(tex=("o1", 4)), ": " + FWD_OVER),
    ("texture_cube", dict(ctx="sharded"), WRONG_SHARD),

    ("texture_cube_grad", dict(ctx=None), None),
    ("texture_cube_grad", dict(fs=None), ": null frameset"),
    ("texture_cube_grad", dict(vis=None), ": null d_vis"),
    ("texture_cube_grad", dict(dir=None), ": null d_dir"),
    ("texture_cube_grad", dict(gout=None), ": null d_gout"),
    ("texture_cube_grad", dict(tex=None), ": d_gdir needs d_tex"),
    ("texture_cube_grad", dict(gtex=None, gdir=None), ": neither d_gtex nor d_gdir is asked for"),
    ("texture_cube_grad", dict(n=0), ": " + N_SIZE),
    ("texture_cube_grad", dict(n=abi.TEX_MAX_SIZE + 1), ": " + N_SIZE),
    ("texture_cube_grad", dict(n_ch=0), ": " + N_CH),
    ("texture_cube_grad", dict(n_ch=abi.ATTR_MAX_CH + 1), ": " + N_CH),
    ("texture_cube_grad", dict(tex_frames=0), ": " + TEX_FRAMES),
    ("texture_cube_grad", dict(tex_frames=3), ": " + TEX_FRAMES),
    ("texture_cube_grad", dict(flags=16), ": " + ONLY_FUSED),
    ("texture_cube_grad", dict(vis=("vis", 4)), ": " + BWD_16),
    ("texture_cube_grad", dict(dir=("dir", 4)), ": " + BWD_16),
    ("texture_cube_grad", dict(gout=("g", 8)), ": " + BWD_16),
    ("texture_cube_grad", dict(gdir=("o1", 4)), ": " + BWD_16),
    ("texture_cube_grad", dict(tex=("tex", 2)), ": d_tex and d_gtex must be 4-byte aligned"),
    ("texture_cube_grad", dict(gtex=("o2", 2)), ": d_tex and d_gtex must be 4-byte aligned"),
    ("texture_cube_grad", dict(gtex=("vis", 4)), BWD_NAMES + ": " + OUT_IN),
    ("texture_cube_grad", dict(gtex=("dir", 4)), BWD_NAMES + ": " + OUT_IN),
    ("texture_cube_grad", dict(gtex=("g", 4)), BWD_NAMES + ": " + OUT_IN),
    ("texture_cube_grad", dict(gtex=("tex", CUBE - 4)), BWD_NAMES + ": " + OUT_IN),
    ("texture_cube_grad", dict(gdir=("vis", 16)), BWD_NAMES + ": " + OUT_IN),
    ("texture_cube_grad", dict(gdir=("dir", PLANES3 - 16)), BWD_NAMES + ": " + OUT_IN),
    ("texture_cube_grad", dict(gdir=("g", 0)), BWD_NAMES + ": " + OUT_IN),
    ("texture_cube_grad", dict(gdir=("tex", 0)), BWD_NAMES + ": " + OUT_IN),
    ("texture_cube_grad", dict(gout=("o1", 16)), BWD_NAMES + ": " + OUT_IN),
    ("texture_cube_grad", dict(gtex=("o1", PLANES3 - 4)), BWD_NAMES + ": " + OUT_OUT),
    ("texture_cube_grad", dict(gdir=("o2", 16)), BWD_NAMES + ": " + OUT_OUT),
    ("texture_cube_grad", dict(ctx="sharded"), WRONG_SHARD),
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
    k.fs["main"].render_visibility(vis.data_ptr(), PLANES4, F, stream())
    torch.cuda.synchronize()
    k.buf = {"vis": vis, "dir": torch.ones(PLANES4 // 4, dtype=torch.float32, device="cuda"),
             "g": torch.ones(PLANES4 // 4, dtype=torch.float32, device="cuda"),
             "tex": torch.ones(2 * CUBE // 4, dtype=torch.float32, device="cuda"),
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
    """ENTRIES' arguments are a valid call of both entry points, and so are the calls that leave out what may be left out: the
    refusals above are each due to the one argument their row changes"""
    kit.buf["o2"].zero_()  # (d_gtex is added into: the sentinel, 2e18 as a float, would swallow the adds)
    for entry, fault in (("texture_cube", {}), ("texture_cube", dict(tex=("tex", 0), tex_frames=2)), ("texture_cube_grad", {}),
                         ("texture_cube_grad", dict(gdir=None, tex=None)), ("texture_cube_grad", dict(gtex=None)),
                         ("texture_cube_grad", dict(tex_frames=2))):
        rc, h = call(kit, entry, fault)
        assert rc == 0, (entry, fault, srz.lib().srz_last_error(h))
    torch.cuda.synchronize()
    assert not torch.equal(kit.buf["o1"], kit.before["o1"]) and bool(kit.buf["o2"].any())
    for name, t in kit.buf.items():  # (the outputs are written now: the sentinels go back for whatever runs next)
        t.copy_(kit.before[name])
