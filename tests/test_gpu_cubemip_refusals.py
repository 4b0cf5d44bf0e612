"""-m gpu: what srz_frameset_texture_cube_mip, _texture_cube_mip_grad, srz_frameset_cube_level and srz_cube_mip_build / _fold refuse,
and in which words.  One call per row of CASES: every argument is valid but the one(s) the row names, so the call has exactly one
fault; it must return SRZ_E_INVALID, leave the row's text in srz_last_error, and touch no buffer.  Nothing reaches a kernel: every
call is refused on the host.  (tests/test_gpu_cube_refusals.py's scheme.)"""
import types

import pytest
import torch

import srz
from srz import abi
from support import frame, soup, stream

pytestmark = pytest.mark.gpu

F, E = abi.FUSED_CLEAR, abi.SRZ_E_INVALID
SENTINEL = 0x5eed5eed
T, C, W, H, N, L = 24, 3, 64, 64, 8, 4  # triangles per frame, channels, frame size, cube size, its levels
PLANES4 = 2 * 4 * H * W * 4  # bytes of a visibility buffer of the two-frame set
PLANES6 = 2 * 6 * H * W * 4  # bytes of the derivative planes = the largest buffer any call here names
PLANES3 = 2 * 3 * H * W * 4  # bytes of the direction planes, and of the output at C = 3
PLANES1 = 2 * 1 * H * W * 4  # bytes of a level plane
CUBE = 6 * N * N * C * 4     # bytes of one cube
MIP = 6 * (16 + 4 + 1) * C * 4  # bytes of one cube's levels 1 .. 3
WRONG_SHARD = "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)"
ONLY_FUSED = "only SRZ_FUSED_CLEAR is accepted in flags"
N_CH, N_SIZE = "n_ch must be 1 .. SRZ_ATTR_MAX_CH", "n must be 1 .. SRZ_TEX_MAX_SIZE"
TEX_FRAMES = "tex_frames must be 1 or the set's frame count"
LEVELS = "n_levels must be 1 .. srz_cube_mip_levels(n)"
FWD_16 = "the plane buffers (d_vis, d_dir, d_lam, d_out) must be 16-byte aligned"
BWD_16 = "the plane buffers (d_vis, d_dir, d_lam, d_gout, d_gdir, d_glam) must be 16-byte aligned"
LVL_16 = "the plane buffers (d_vis, d_dir, d_dird, d_out) must be 16-byte aligned"
BWD_4 = "the cube, the pyramid and their gradients must be 4-byte aligned"
OUT_IN, OUT_OUT = "an output overlaps an input", "two outputs overlap"
TOGETHER = "d_gtex and d_gmip come together when n_levels > 1"

# entry point -> its arguments after (ctx, fs), in order, each with the value of a valid call.  (name, offset): the address of a
# buffer of the kit plus `offset` bytes — vis: a visibility buffer; dir, dird, lam, g: inputs of PLANES6 bytes; tex: two cubes; mip:
# two cubes' pyramids; o1 .. o4: sentinel-filled outputs of PLANES6 + 256 bytes.
ENTRIES = {
    "texture_cube_mip": dict(vis=("vis", 0), dir=("dir", 0), lam=("lam", 0), tex=("tex", 0), n=N, n_ch=C, tex_frames=1, mip=("mip", 0), n_levels=L,
                             out=("o1", 0), out_bytes=PLANES3, flags=F),
    "texture_cube_mip_grad": dict(vis=("vis", 0), dir=("dir", 0), lam=("lam", 0), gout=("g", 0), tex=("tex", 0), mip=("mip", 0), n=N, n_ch=C,
                                  tex_frames=1, n_levels=L, gtex=("o2", 0), gmip=("o3", 0), gdir=("o1", 0), glam=("o4", 0), flags=F),
    "cube_level": dict(vis=("vis", 0), dir=("dir", 0), dird=("dird", 0), n=N, n_levels=L, out=("o1", 0), out_bytes=PLANES1, flags=F),
}
FWD, BWD, LVL = "texture_cube_mip", "texture_cube_mip_grad", "cube_level"

# (entry point, the faulty argument(s), text after "srz_frameset_<entry point>"; WRONG_SHARD stands alone; None: no text is set)
CASES = [
    (FWD, dict(ctx=None), None),
    (FWD, dict(fs=None), ": null frameset"),
    (FWD, dict(vis=None), ": null d_vis"),
    (FWD, dict(dir=None), ": null d_dir"),
    (FWD, dict(tex=None), ": null d_tex"),
    (FWD, dict(out=None), ": null d_out"),
    (FWD, dict(lam=None), ": n_levels > 1 needs the level plane"),
    (FWD, dict(mip=None), ": n_levels > 1 needs the pyramid"),
    (FWD, dict(n=0), ": " + N_SIZE),
    (FWD, dict(n=abi.TEX_MAX_SIZE + 1), ": " + N_SIZE),
    (FWD, dict(n_ch=0), ": " + N_CH),
    (FWD, dict(n_ch=abi.ATTR_MAX_CH + 1), ": " + N_CH),
    (FWD, dict(tex_frames=0), ": " + TEX_FRAMES),
    (FWD, dict(tex_frames=3), ": " + TEX_FRAMES),
    (FWD, dict(n_levels=0), ": " + LEVELS),
    (FWD, dict(n_levels=L + 1), ": " + LEVELS),
    (FWD, dict(n=6, n_levels=3), ": " + LEVELS),
    (FWD, dict(out_bytes=PLANES3 - 1), ": out_bytes is too small for d_out"),
    (FWD, dict(flags=abi.UNIFIED), ": " + ONLY_FUSED),
    (FWD, dict(flags=F | abi.ORDERED_RASTER), ": " + ONLY_FUSED),
    (FWD, dict(vis=("vis", 4)), ": " + FWD_16),
    (FWD, dict(dir=("dir", 8)), ": " + FWD_16),
    (FWD, dict(lam=("lam", 4)), ": " + FWD_16),
    (FWD, dict(out=("o1", 4)), ": " + FWD_16),
    (FWD, dict(tex=("tex", 2)), ": d_tex and d_mip must be 4-byte aligned"),
    (FWD, dict(mip=("mip", 1)), ": d_tex and d_mip must be 4-byte aligned"),
    (FWD, dict(out=("vis", 64)), ": " + OUT_IN),
    (FWD, dict(out=("dir", 0)), ": " + OUT_IN),
    (FWD, dict(out=("lam", 0)), ": " + OUT_IN),
    (FWD, dict(out=("tex", 0)), ": " + OUT_IN),
    (FWD, dict(out=("mip", 0)), ": " + OUT_IN),
    (FWD, dict(lam=("o1", PLANES3 - 16)), ": " + OUT_IN),
    (FWD, dict(mip=("o1", 4)), ": " + OUT_IN),
    (FWD, dict(ctx="sharded"), WRONG_SHARD),

    (BWD, dict(ctx=None), None),
    (BWD, dict(fs=None), ": null frameset"),
    (BWD, dict(vis=None), ": null d_vis"),
    (BWD, dict(dir=None), ": null d_dir"),
    (BWD, dict(gout=None), ": null d_gout"),
    (BWD, dict(lam=None), ": n_levels > 1 needs the level plane"),
    (BWD, dict(tex=None), ": d_gdir and d_glam need d_tex"),
    (BWD, dict(tex=None, gdir=None), ": d_gdir and d_glam need d_tex"),  # d_glam without the texels
    (BWD, dict(mip=None), ": d_gdir and d_glam need the pyramid when n_levels > 1"),
    (BWD, dict(mip=None, gdir=None), ": d_gdir and d_glam need the pyramid when n_levels > 1"),
    (BWD, dict(gtex=None, gmip=None, gdir=None, glam=None), ": no output is asked for"),
    (BWD, dict(n_levels=1, gtex=None, gdir=None, glam=None), ": no output is asked for"),  # (d_gmip alone is nothing at one level)
    (BWD, dict(gmip=None), ": " + TOGETHER),
    (BWD, dict(gtex=None), ": " + TOGETHER),
    (BWD, dict(n=0), ": " + N_SIZE),
    (BWD, dict(n=abi.TEX_MAX_SIZE + 1), ": " + N_SIZE),
    (BWD, dict(n_ch=0), ": " + N_CH),
    (BWD, dict(n_ch=abi.ATTR_MAX_CH + 1), ": " + N_CH),
    (BWD, dict(tex_frames=0), ": " + TEX_FRAMES),
    (BWD, dict(tex_frames=3), ": " + TEX_FRAMES),
    (BWD, dict(n_levels=0), ": " + LEVELS),
    (BWD, dict(n_levels=L + 1), ": " + LEVELS),
    (BWD, dict(flags=16), ": " + ONLY_FUSED),
    (BWD, dict(vis=("vis", 4)), ": " + BWD_16),
    (BWD, dict(dir=("dir", 4)), ": " + BWD_16),
    (BWD, dict(lam=("lam", 8)), ": " + BWD_16),
    (BWD, dict(gout=("g", 8)), ": " + BWD_16),
    (BWD, dict(gdir=("o1", 4)), ": " + BWD_16),
    (BWD, dict(glam=("o4", 4)), ": " + BWD_16),
    (BWD, dict(tex=("tex", 2)), ": " + BWD_4),
    (BWD, dict(mip=("mip", 2)), ": " + BWD_4),
    (BWD, dict(gtex=("o2", 2)), ": " + BWD_4),
    (BWD, dict(gmip=("o3", 1)), ": " + BWD_4),
    (BWD, dict(gtex=("vis", 4)), ": " + OUT_IN),
    (BWD, dict(gtex=("tex", CUBE - 4)), ": " + OUT_IN),
    (BWD, dict(gmip=("mip", MIP - 4)), ": " + OUT_IN),
    (BWD, dict(gmip=("lam", 4)), ": " + OUT_IN),
    (BWD, dict(gdir=("dir", PLANES3 - 16)), ": " + OUT_IN),
    (BWD, dict(gdir=("g", 0)), ": " + OUT_IN),
    (BWD, dict(glam=("lam", PLANES1 - 16)), ": " + OUT_IN),
    (BWD, dict(glam=("g", 16)), ": " + OUT_IN),
    (BWD, dict(gout=("o4", 16)), ": " + OUT_IN),
    (BWD, dict(gtex=("o1", PLANES3 - 4)), ": " + OUT_OUT),
    (BWD, dict(gmip=("o2", CUBE - 4)), ": " + OUT_OUT),
    (BWD, dict(glam=("o1", PLANES3 - 16)), ": " + OUT_OUT),
    (BWD, dict(glam=("o3", 0)), ": " + OUT_OUT),
    (BWD, dict(ctx="sharded"), WRONG_SHARD),

    (LVL, dict(ctx=None), None),
    (LVL, dict(fs=None), ": null frameset"),
    (LVL, dict(vis=None), ": null d_vis"),
    (LVL, dict(dir=None), ": null d_dir"),
    (LVL, dict(dird=None), ": null d_dird"),
    (LVL, dict(out=None), ": null d_out"),
    (LVL, dict(n=0), ": " + N_SIZE),
    (LVL, dict(n=abi.TEX_MAX_SIZE + 1), ": " + N_SIZE),
    (LVL, dict(n_levels=0), ": " + LEVELS),
    (LVL, dict(n_levels=L + 1), ": " + LEVELS),
    (LVL, dict(out_bytes=PLANES1 - 1), ": out_bytes is too small for d_out"),
    (LVL, dict(flags=F | abi.UNIFIED), ": " + ONLY_FUSED),
    (LVL, dict(vis=("vis", 8)), ": " + LVL_16),
    (LVL, dict(dir=("dir", 4)), ": " + LVL_16),
    (LVL, dict(dird=("dird", 4)), ": " + LVL_16),
    (LVL, dict(out=("o1", 8)), ": " + LVL_16),
    (LVL, dict(out=("vis", 0)), ": " + OUT_IN),
    (LVL, dict(out=("dir", PLANES3 - 16)), ": " + OUT_IN),
    (LVL, dict(out=("dird", PLANES6 - 16)), ": " + OUT_IN),
    (LVL, dict(ctx="sharded"), WRONG_SHARD),
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
    assert vis.numel() * 4 == PLANES4 == fs.out_bytes and fs.interpolate_bytes(3) == PLANES3 and fs.interpolate_bytes(1) == PLANES1
    assert fs.interpolate_bytes(6) == PLANES6 and srz.cube_mip_bytes(N, C, 1, L) == MIP and srz.cube_mip_levels(N) == L
    fs.render_visibility(vis.data_ptr(), PLANES4, F, stream())
    torch.cuda.synchronize()
    ones = lambda nbytes: torch.ones(nbytes // 4, dtype=torch.float32, device="cuda")  # noqa: E731
    out = lambda: torch.full((PLANES6 // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda")  # noqa: E731
    k.buf = {"vis": vis, "dir": ones(PLANES6), "dird": ones(PLANES6), "lam": ones(PLANES6), "g": ones(PLANES6), "tex": ones(2 * CUBE),
             "mip": ones(2 * MIP), "o1": out(), "o2": out(), "o3": out(), "o4": out()}
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


def untouched(kit):
    torch.cuda.synchronize()
    for name, t in kit.buf.items():
        assert torch.equal(t, kit.before[name]), f"{name} was written"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_refusal(kit, case):
    entry, fault, text = case
    lib = srz.lib()
    # every context's text is first set to another refusal's, so that a stale text cannot stand in for the one expected
    marker = "srz_frameset_render: null frameset / output"
    for c in kit.ctx.values():
        assert lib.srz_frameset_render(c.h, None, None, 0, 0, None) == E and lib.srz_last_error(c.h).decode() == marker
    created = lib.srz_last_error(None)
    rc, h = call(kit, entry, fault)
    assert rc == E, (rc, lib.srz_last_error(h))
    if text is None:  # (no context to leave a text in: nobody's text changes)
        assert h is None and lib.srz_last_error(None) == created
        assert all(lib.srz_last_error(c.h).decode() == marker for c in kit.ctx.values())
    else:
        assert lib.srz_last_error(h).decode() == (text if text is WRONG_SHARD else f"srz_frameset_{entry}{text}")
    untouched(kit)


def test_the_pyramid_wrappers_refuse_what_the_2d_functions_refuse_and_too_many_frames(kit):
    """srz_cube_mip_build / _fold: tex_frames of 0 and 6 * tex_frames above 65536 (10923 frames), refused before any size is looked
    at, and srz_texture_mip_build's own refusals through the wrapper"""
    lib, h = srz.lib(), kit.ctx["main"].h
    tex, mip, o2, o3 = (kit.buf[k].data_ptr() for k in ("tex", "mip", "o2", "o3"))
    rows = [(lambda: lib.srz_cube_mip_build(h, tex, 2, 1, 10923, 2, o3, 1 << 40, None), "srz_cube_mip_build: 6 * tex_frames must be 6 .. 65536"),
            (lambda: lib.srz_cube_mip_build(h, tex, 2, 1, 0, 2, o3, 1 << 40, None), "srz_cube_mip_build: 6 * tex_frames must be 6 .. 65536"),
            (lambda: lib.srz_cube_mip_fold(h, mip, 1 << 40, 2, 1, 10923, 2, o2, None), "srz_cube_mip_fold: 6 * tex_frames must be 6 .. 65536"),
            (lambda: lib.srz_cube_mip_build(h, tex, N, C, 1, L + 1, o3, MIP, None),
             "srz_texture_mip_build: n_levels must be 1 .. srz_texture_mip_levels(tex_w, tex_h)"),
            (lambda: lib.srz_cube_mip_build(h, tex, N, C, 1, L, o3, MIP - 1, None), "srz_texture_mip_build: mip_bytes is below srz_texture_mip_bytes"),
            (lambda: lib.srz_cube_mip_build(h, None, N, C, 1, L, o3, MIP, None), "srz_texture_mip_build: null texture"),
            (lambda: lib.srz_cube_mip_build(h, tex, N, C, 1, L, tex + CUBE - 4, MIP, None), "srz_texture_mip_build: the pyramid overlaps the texture"),
            (lambda: lib.srz_cube_mip_fold(h, None, MIP, N, C, 1, L, o2, None), "srz_texture_mip_fold: null pyramid")]
    for fn, text in rows:
        assert fn() == E and lib.srz_last_error(h).decode() == text, text
    # the lookup with a pyramid refuses a frame count the pyramid's layout cannot hold (only reachable with a set of that many frames;
    # the helper is what the pass asks)
    assert srz.cube_mip_bytes(N, C, 10923, L) == 0 and srz.cube_mip_bytes(N, C, 10922, L) == 10922 * MIP
    untouched(kit)


def test_the_valid_calls_are_accepted(kit):
    """ENTRIES' arguments are a valid call of each entry point, and so are the calls that leave out what may be left out: the refusals
    above are each due to the argument(s) their row changes"""
    for name in ("o2", "o3"):
        kit.buf[name].zero_()  # (added into: the sentinel, 2e18 as a float, would swallow the adds)
    for entry, fault in ((FWD, {}), (FWD, dict(tex_frames=2)), (FWD, dict(n_levels=1, lam=None, mip=None)), (FWD, dict(n_levels=2)),
                         (BWD, {}), (BWD, dict(gdir=None, glam=None, tex=None, mip=None)), (BWD, dict(gtex=None, gmip=None)),
                         (BWD, dict(gtex=None, gmip=None, gdir=None)), (BWD, dict(tex_frames=2)),
                         (BWD, dict(n_levels=1, lam=None, mip=None, gmip=None)), (BWD, dict(n_levels=1, gtex=None, gmip=("o3", 1), glam=None)),
                         (LVL, {}), (LVL, dict(n_levels=1))):
        rc, h = call(kit, entry, fault)
        assert rc == 0, (entry, fault, srz.lib().srz_last_error(h))
    torch.cuda.synchronize()
    assert not torch.equal(kit.buf["o1"], kit.before["o1"]) and bool(kit.buf["o2"].any()) and bool(kit.buf["o3"].any())
    assert not torch.equal(kit.buf["o4"], kit.before["o4"])
    for name, t in kit.buf.items():  # (the outputs are written now: the sentinels go back for whatever runs next)
        t.copy_(kit.before[name])
