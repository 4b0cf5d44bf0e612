"""-m gpu: what srz_frameset_background and _background_grad refuse, and in which words.  One call per row of CASES: every argument
is valid but the one the row names, so the call has exactly one fault; it must return SRZ_E_INVALID, leave the row's text — which
names the argument — in srz_last_error, and touch no buffer.  Nothing reaches a kernel: every call is refused on the host.
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
T, C, W, H, N = 24, 3, 64, 64, 8  # triangles per frame, channels, frame size, cube size
PLANES4 = 2 * 4 * H * W * 4  # bytes of a visibility buffer of the two-frame set = the largest buffer any call here names
PLANES3 = 2 * 3 * H * W * 4  # bytes of the output and of gout at C = 3
CUBE = 6 * N * N * C * 4     # bytes of one cube
WORK = 2 * (2 * 2 + 1) * 9 * 4  # srz_frameset_background_work_bytes: two frames of 2 x 2 tiles
WRONG_SHARD = "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)"
ONLY_FUSED = "only SRZ_FUSED_CLEAR is accepted in flags"
N_CH, N_SIZE = "n_ch must be 1 .. SRZ_ATTR_MAX_CH", "n must be 1 .. SRZ_TEX_MAX_SIZE"
TEX_FRAMES, RAY_FRAMES = "tex_frames must be 1 or the set's frame count", "ray_frames must be 1 or the set's frame count"
WHERE = "where must be SRZ_BG_NOBODY or SRZ_BG_ALL"
FWD_16, FWD_4 = "the plane buffers (d_vis, d_out) must be 16-byte aligned", "d_ray and d_tex must be 4-byte aligned"
FWD_NAMES = " (d_out against d_vis, d_ray, d_tex)"
BWD_16, BWD_4 = "the plane buffers (d_vis, d_gout) must be 16-byte aligned", "d_ray, d_tex, d_gtex, d_gray and d_work must be 4-byte aligned"
BWD_NAMES = " (d_gtex, d_gray, d_work against d_vis, d_ray, d_gout, d_tex)"
OUT_IN, OUT_OUT = "an output overlaps an input", "two outputs overlap"

# entry point -> its arguments after (ctx, fs), in order, each with the value of a valid call.  (name, offset): the address of a
# buffer of the kit plus `offset` bytes — vis: a visibility buffer; g: an input of PLANES4 bytes; ray: two blocks; tex: two cubes;
# o1, o2, o3: sentinel-filled outputs of PLANES4 + 256 bytes.
ENTRIES = {
    "background": dict(vis=("vis", 0), ray=("ray", 0), ray_frames=1, tex=("tex", 0), n=N, n_ch=C, tex_frames=1, where=0, out=("o1", 0),
                       out_bytes=PLANES3, flags=F),
    "background_grad": dict(vis=("vis", 0), ray=("ray", 0), ray_frames=1, gout=("g", 0), tex=("tex", 0), n=N, n_ch=C, tex_frames=1, where=0,
                            gtex=("o2", 0), gray=("o1", 0), work=("o3", 0), work_bytes=WORK, flags=F),
}

# (entry point, the faulty argument(s), text after "srz_frameset_<entry point>"; WRONG_SHARD stands alone; None: no text is set)
CASES = [
    ("background", dict(ctx=None), None),
    ("background", dict(fs=None), ": null frameset"),
    ("background", dict(vis=None), ": null d_vis"),
    ("background", dict(ray=None), ": null d_ray"),
    ("background", dict(tex=None), ": null d_tex"),
    ("background", dict(out=None), ": null d_out"),
    ("background", dict(out=None, where=1, vis=None), ": null d_out"),
    ("background", dict(n=0), ": " + N_SIZE),
    ("background", dict(n=abi.TEX_MAX_SIZE + 1), ": " + N_SIZE),
    ("background", dict(n_ch=0), ": " + N_CH),
    ("background", dict(n_ch=abi.ATTR_MAX_CH + 1), ": " + N_CH),
    ("background", dict(tex_frames=0), ": " + TEX_FRAMES),
    ("background", dict(tex_frames=3), ": " + TEX_FRAMES),
    ("background", dict(ray_frames=0), ": " + RAY_FRAMES),
    ("background", dict(ray_frames=3), ": " + RAY_FRAMES),
    ("background", dict(where=2), ": " + WHERE),
    ("background", dict(where=0xffffffff), ": " + WHERE),
    ("background", dict(out_bytes=PLANES3 - 1), ": out_bytes is too small for d_out"),
    ("background", dict(flags=abi.UNIFIED), ": " + ONLY_FUSED),
    ("background", dict(flags=F | abi.ORDERED_RASTER), ": " + ONLY_FUSED),
    ("background", dict(vis=("vis", 4)), ": " + FWD_16),
    ("background", dict(out=("o1", 4)), ": " + FWD_16),
    ("background", dict(ray=("ray", 2)), ": " + FWD_4),
    ("background", dict(tex=("tex", 2)), ": " + FWD_4),
    ("background", dict(out=("vis", 64)), FWD_NAMES + ": " + OUT_IN),
    ("background", dict(ray=("o1", 8)), FWD_NAMES + ": " + OUT_IN),
    ("background", dict(tex=("o1", PLANES3 - 4)), FWD_NAMES + ": " + OUT_IN),
    ("background", dict(out=("tex", 0)), FWD_NAMES + ": " + OUT_IN),
    ("background", dict(ctx="sharded"), WRONG_SHARD),

    ("background_grad", dict(ctx=None), None),
    ("background_grad", dict(fs=None), ": null frameset"),
    ("background_grad", dict(vis=None), ": null d_vis"),
    ("background_grad", dict(ray=None), ": null d_ray"),
    ("background_grad", dict(gout=None), ": null d_gout"),
    ("background_grad", dict(gtex=None, gray=None), ": neither d_gtex nor d_gray is asked for"),
    ("background_grad", dict(tex=None), ": d_gray needs d_tex"),
    ("background_grad", dict(work=None), ": d_gray needs d_work"),
    ("background_grad", dict(n=0), ": " + N_SIZE),
    ("background_grad", dict(n=abi.TEX_MAX_SIZE + 1), ": " + N_SIZE),
    ("background_grad", dict(n_ch=0), ": " + N_CH),
    ("background_grad", dict(n_ch=abi.ATTR_MAX_CH + 1), ": " + N_CH),
    ("background_grad", dict(tex_frames=0), ": " + TEX_FRAMES),
    ("background_grad", dict(tex_frames=3), ": " + TEX_FRAMES),
    ("background_grad", dict(ray_frames=0), ": " + RAY_FRAMES),
    ("background_grad", dict(ray_frames=3), ": " + RAY_FRAMES),
    ("background_grad", dict(where=2), ": " + WHERE),
    ("background_grad", dict(work_bytes=WORK - 1), ": work_bytes is below srz_frameset_background_work_bytes"),
    ("background_grad", dict(flags=16), ": " + ONLY_FUSED),
    ("background_grad", dict(vis=("vis", 4)), ": " + BWD_16),
    ("background_grad", dict(gout=("g", 8)), ": " + BWD_16),
    ("background_grad", dict(ray=("ray", 2)), ": " + BWD_4),
    ("background_grad", dict(tex=("tex", 2)), ": " + BWD_4),
    ("background_grad", dict(gtex=("o2", 2)), ": " + BWD_4),
    ("background_grad", dict(gray=("o1", 2)), ": " + BWD_4),
    ("background_grad", dict(work=("o3", 2)), ": " + BWD_4),
    ("background_grad", dict(gtex=("vis", 4)), BWD_NAMES + ": " + OUT_IN),
    ("background_grad", dict(gtex=("g", 4)), BWD_NAMES + ": " + OUT_IN),
    ("background_grad", dict(gtex=("tex", CUBE - 4)), BWD_NAMES + ": " + OUT_IN),
    ("background_grad", dict(gray=("ray", 32)), BWD_NAMES + ": " + OUT_IN),
    ("background_grad", dict(gray=("g", 0)), BWD_NAMES + ": " + OUT_IN),
    ("background_grad", dict(work=("vis", 16)), BWD_NAMES + ": " + OUT_IN),
    ("background_grad", dict(work=("tex", 0)), BWD_NAMES + ": " + OUT_IN),
    ("background_grad", dict(gout=("o2", 16)), BWD_NAMES + ": " + OUT_IN),
    ("background_grad", dict(gtex=("o1", 32)), BWD_NAMES + ": " + OUT_OUT),
    ("background_grad", dict(work=("o2", CUBE - 4)), BWD_NAMES + ": " + OUT_OUT),
    ("background_grad", dict(work=("o1", 4)), BWD_NAMES + ": " + OUT_OUT),
    ("background_grad", dict(ctx="sharded"), WRONG_SHARD),
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
    assert k.fs["main"].background_work_bytes() == WORK
    k.fs["main"].render_visibility(vis.data_ptr(), PLANES4, F, stream())
    torch.cuda.synchronize()
    k.buf = {"vis": vis, "g": torch.ones(PLANES4 // 4, dtype=torch.float32, device="cuda"),
             "ray": torch.ones(2 * 9 + 8, dtype=torch.float32, device="cuda"),
             "tex": torch.ones(2 * CUBE // 4, dtype=torch.float32, device="cuda"),
             "o1": torch.full((PLANES4 // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda"),
             "o2": torch.full((PLANES4 // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda"),
             "o3": torch.full((PLANES4 // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda")}
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
    """ENTRIES' arguments are a valid call of both entry points, and so are the calls that leave out what may be left out — d_vis with
    SRZ_BG_ALL among them, a misaligned one too: it is not read —: the refusals above are each due to the one argument their row
    changes"""
    kit.buf["o2"].zero_()  # (d_gtex is added into: the sentinel as a float would swallow the adds)
    for entry, fault in (("background", {}), ("background", dict(tex_frames=2, ray_frames=2)), ("background", dict(where=1, vis=None)),
                         ("background", dict(where=1, vis=("vis", 4))), ("background_grad", {}),
                         ("background_grad", dict(gray=None, work=None, work_bytes=0, tex=None)), ("background_grad", dict(gtex=None)),
                         ("background_grad", dict(tex_frames=2, ray_frames=2)), ("background_grad", dict(where=1, vis=None))):
        rc, h = call(kit, entry, fault)
        assert rc == 0, (entry, fault, srz.lib().srz_last_error(h))
    torch.cuda.synchronize()
    assert not torch.equal(kit.buf["o1"], kit.before["o1"]) and bool(kit.buf["o2"].any())
    for name, t in kit.buf.items():  # (the outputs are written now: the sentinels go back for whatever runs next)
        t.copy_(kit.before[name])
