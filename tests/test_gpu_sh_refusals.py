"""-m gpu: what srz_frameset_sh, srz_frameset_sh_grad, srz_cube_sh and srz_cube_sh_grad refuse, and in which words.  One call per row
of CASES: every argument is valid but the one the row names, so the call has exactly one fault; it must return SRZ_E_INVALID, leave
the row's text — which names the function and the argument — in srz_last_error, and touch no buffer.  Nothing reaches a kernel: every
call is refused on the host.  (tests/test_gpu_microfacet_refusals.py's scheme.)  Then the torch layer's own refusals."""
import types

import pytest
import torch

import srz
from srz import abi
from support import frame, soup, stream

pytestmark = pytest.mark.gpu

F, E = abi.FUSED_CLEAR, abi.SRZ_E_INVALID
SENTINEL = 0x5eed5eed
T, W, H, C = 24, 64, 64, 3        # triangles per frame, frame size, channels
PLANES4 = 2 * 4 * H * W * 4       # bytes of a visibility buffer of the two-frame set = the largest buffer any call here names
PLANES3 = 2 * 3 * H * W * 4       # bytes of every three-plane buffer (the normals; C = 3: the output too)
SH = 9 * C * 4                    # bytes of one frame's coefficients
WORK = 2 * (4 + 1) * SH           # srz_frameset_sh_work_bytes of the set: two frames of four tiles, and a row per frame
N, CF = 8, 2                      # the cube: faces of 8 x 8, two frames
CUBE = CF * 6 * N * N * C * 4     # its bytes
CWORK = CF * (6 * N + 7) * (9 * C + 1) * 4  # srz_cube_sh_work_bytes
WRONG_SHARD = "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)"
ONLY_FUSED = "only SRZ_FUSED_CLEAR is accepted in flags"
N_CH, SH_FRAMES, KIND = "n_ch must be 1 .. SRZ_SH_MAX_CH", "sh_frames must be 1 or the set's frame count", "kind must be SRZ_SH_IRRADIANCE or SRZ_SH_RADIANCE"
FWD_16 = "the plane buffers (d_vis, d_nrm, d_out) must be 16-byte aligned"
BWD_16 = "the plane buffers (d_vis, d_nrm, d_gout, d_gnrm) must be 16-byte aligned"
BWD_4 = "d_sh, d_gsh and d_work must be 4-byte aligned"
FWD_NAMES = " (d_out against d_vis, d_nrm, d_sh)"
BWD_NAMES = " (d_gnrm, d_gsh, d_work against d_vis, d_nrm, d_sh, d_gout)"
OUT_IN, OUT_OUT = "an output overlaps an input", "two outputs overlap"
WORK_SHORT = "work_bytes is below srz_frameset_sh_work_bytes"
CN, CFR = "n must be 1 .. SRZ_TEX_MAX_SIZE", "tex_frames must be 1 .. 65536"
C_4, CG_4 = "d_src, d_sh, d_den and d_work must be 4-byte aligned", "d_gsh, d_den, d_gsrc and d_work must be 4-byte aligned"
C_NAMES, CG_NAMES = " (d_sh, d_den, d_work against d_src)", " (d_gsrc, d_work against d_gsh, d_den)"
C_WORK = "work_bytes is below srz_cube_sh_work_bytes"

# entry point -> its arguments after ctx (and fs, for the set's passes), in order, each with the value of a valid call.  (name, offset):
# the address of a buffer of the kit plus `offset` bytes — vis: a visibility buffer; nrm, g, sh, src, den: inputs of PLANES4 bytes;
# o1 .. o4: sentinel-filled outputs of PLANES4 + 256 bytes.
ENTRIES = {
    "srz_frameset_sh": dict(vis=("vis", 0), nrm=("nrm", 0), sh=("sh", 0), n_ch=C, sh_frames=1, kind=0, out=("o1", 0), out_bytes=PLANES3, flags=F),
    "srz_frameset_sh_grad": dict(vis=("vis", 0), nrm=("nrm", 0), sh=("sh", 0), n_ch=C, sh_frames=1, kind=0, gout=("g", 0), gnrm=("o1", 0),
                                 gsh=("o2", 0), work=("o3", 0), work_bytes=WORK, flags=F),
    "srz_cube_sh": dict(src=("src", 0), n=N, n_ch=C, tex_frames=CF, sh=("o1", 0), den=("o2", 0), work=("o3", 0), work_bytes=CWORK),
    "srz_cube_sh_grad": dict(gsh=("sh", 0), den=("den", 0), n=N, n_ch=C, tex_frames=CF, gsrc=("o1", 0), work=("o3", 0), work_bytes=CWORK),
}
FS, FG, CS, CG = ENTRIES

# (entry point, the faulty argument(s), text after the function's name; WRONG_SHARD stands alone; None: no text is set)
CASES = [
    (FS, dict(ctx=None), None),
    (FS, dict(fs=None), ": null frameset"),
    (FS, dict(vis=None), ": null d_vis"),
    (FS, dict(nrm=None), ": null d_nrm"),
    (FS, dict(sh=None), ": null d_sh"),
    (FS, dict(out=None), ": null d_out"),
    (FS, dict(n_ch=0), ": " + N_CH),
    (FS, dict(n_ch=abi.SH_MAX_CH + 1), ": " + N_CH),
    (FS, dict(n_ch=0xffffffff), ": " + N_CH),
    (FS, dict(sh_frames=0), ": " + SH_FRAMES),
    (FS, dict(sh_frames=3), ": " + SH_FRAMES),
    (FS, dict(kind=2), ": " + KIND),
    (FS, dict(kind=0xffffffff), ": " + KIND),
    (FS, dict(out_bytes=PLANES3 - 1), ": out_bytes is too small for d_out"),
    (FS, dict(flags=abi.UNIFIED), ": " + ONLY_FUSED),
    (FS, dict(flags=F | abi.ORDERED_RASTER), ": " + ONLY_FUSED),
    (FS, dict(vis=("vis", 4)), ": " + FWD_16),
    (FS, dict(nrm=("nrm", 8)), ": " + FWD_16),
    (FS, dict(out=("o1", 4)), ": " + FWD_16),
    (FS, dict(sh=("sh", 2)), ": d_sh must be 4-byte aligned"),
    (FS, dict(out=("vis", 64)), FWD_NAMES + ": " + OUT_IN),
    (FS, dict(out=("nrm", 0)), FWD_NAMES + ": " + OUT_IN),
    (FS, dict(nrm=("o1", PLANES3 - 16)), FWD_NAMES + ": " + OUT_IN),
    (FS, dict(sh=("o1", 4)), FWD_NAMES + ": " + OUT_IN),
    (FS, dict(ctx="sharded"), WRONG_SHARD),

    (FG, dict(ctx=None), None),
    (FG, dict(fs=None), ": null frameset"),
    (FG, dict(vis=None), ": null d_vis"),
    (FG, dict(nrm=None), ": null d_nrm"),
    (FG, dict(sh=None), ": null d_sh"),
    (FG, dict(gout=None), ": null d_gout"),
    (FG, dict(gnrm=None, gsh=None), ": neither d_gnrm nor d_gsh is asked for"),
    (FG, dict(work=None), ": d_gsh needs d_work"),
    (FG, dict(work_bytes=WORK - 1), ": " + WORK_SHORT),
    (FG, dict(work_bytes=0), ": " + WORK_SHORT),
    (FG, dict(n_ch=0), ": " + N_CH),
    (FG, dict(n_ch=abi.SH_MAX_CH + 1), ": " + N_CH),
    (FG, dict(sh_frames=0), ": " + SH_FRAMES),
    (FG, dict(sh_frames=3), ": " + SH_FRAMES),
    (FG, dict(kind=2), ": " + KIND),
    (FG, dict(flags=16), ": " + ONLY_FUSED),
    (FG, dict(vis=("vis", 4)), ": " + BWD_16),
    (FG, dict(nrm=("nrm", 4)), ": " + BWD_16),
    (FG, dict(gout=("g", 8)), ": " + BWD_16),
    (FG, dict(gnrm=("o1", 4)), ": " + BWD_16),
    (FG, dict(sh=("sh", 2)), ": " + BWD_4),
    (FG, dict(gsh=("o2", 2)), ": " + BWD_4),
    (FG, dict(work=("o3", 1)), ": " + BWD_4),
    (FG, dict(gnrm=("vis", 16)), BWD_NAMES + ": " + OUT_IN),
    (FG, dict(gnrm=("nrm", 0)), BWD_NAMES + ": " + OUT_IN),
    (FG, dict(gnrm=("g", PLANES3 - 16)), BWD_NAMES + ": " + OUT_IN),
    (FG, dict(gsh=("sh", 4)), BWD_NAMES + ": " + OUT_IN),
    (FG, dict(gsh=("g", 4)), BWD_NAMES + ": " + OUT_IN),
    (FG, dict(work=("vis", 4)), BWD_NAMES + ": " + OUT_IN),
    (FG, dict(work=("nrm", 4)), BWD_NAMES + ": " + OUT_IN),
    (FG, dict(gout=("o1", 16)), BWD_NAMES + ": " + OUT_IN),
    (FG, dict(sh=("o2", SH - 4)), BWD_NAMES + ": " + OUT_IN),
    (FG, dict(gsh=("o1", PLANES3 - 4)), BWD_NAMES + ": " + OUT_OUT),
    (FG, dict(work=("o2", SH - 4)), BWD_NAMES + ": " + OUT_OUT),
    (FG, dict(work=("o1", 4)), BWD_NAMES + ": " + OUT_OUT),
    (FG, dict(ctx="sharded"), WRONG_SHARD),

    (CS, dict(ctx=None), None),
    (CS, dict(src=None), ": null d_src"),
    (CS, dict(sh=None), ": null d_sh"),
    (CS, dict(work=None), ": null d_work"),
    (CS, dict(n=0), ": " + CN),
    (CS, dict(n=abi.TEX_MAX_SIZE + 1), ": " + CN),
    (CS, dict(n_ch=0), ": " + N_CH),
    (CS, dict(n_ch=abi.SH_MAX_CH + 1), ": " + N_CH),
    (CS, dict(tex_frames=0), ": " + CFR),
    (CS, dict(tex_frames=65537), ": " + CFR),
    (CS, dict(work_bytes=CWORK - 1), ": " + C_WORK),
    (CS, dict(work_bytes=0), ": " + C_WORK),
    (CS, dict(src=("src", 2)), ": " + C_4),
    (CS, dict(sh=("o1", 2)), ": " + C_4),
    (CS, dict(den=("o2", 1)), ": " + C_4),
    (CS, dict(work=("o3", 2)), ": " + C_4),
    (CS, dict(sh=("src", 0)), C_NAMES + ": " + OUT_IN),
    (CS, dict(den=("src", CUBE - 4)), C_NAMES + ": " + OUT_IN),
    (CS, dict(work=("src", CUBE - 4)), C_NAMES + ": " + OUT_IN),
    (CS, dict(src=("o3", CWORK - 4)), C_NAMES + ": " + OUT_IN),
    (CS, dict(den=("o1", CF * SH - 4)), C_NAMES + ": " + OUT_OUT),
    (CS, dict(work=("o1", 4)), C_NAMES + ": " + OUT_OUT),
    (CS, dict(work=("o2", 0)), C_NAMES + ": " + OUT_OUT),

    (CG, dict(ctx=None), None),
    (CG, dict(gsh=None), ": null d_gsh"),
    (CG, dict(den=None), ": null d_den"),
    (CG, dict(gsrc=None), ": null d_gsrc"),
    (CG, dict(work=None), ": null d_work"),
    (CG, dict(n=0), ": " + CN),
    (CG, dict(n=abi.TEX_MAX_SIZE + 1), ": " + CN),
    (CG, dict(n_ch=0), ": " + N_CH),
    (CG, dict(n_ch=abi.SH_MAX_CH + 1), ": " + N_CH),
    (CG, dict(tex_frames=0), ": " + CFR),
    (CG, dict(tex_frames=65537), ": " + CFR),
    (CG, dict(work_bytes=CWORK - 1), ": " + C_WORK),
    (CG, dict(gsh=("sh", 2)), ": " + CG_4),
    (CG, dict(den=("den", 2)), ": " + CG_4),
    (CG, dict(gsrc=("o1", 1)), ": " + CG_4),
    (CG, dict(work=("o3", 2)), ": " + CG_4),
    (CG, dict(gsrc=("sh", 4)), CG_NAMES + ": " + OUT_IN),
    (CG, dict(gsrc=("den", 0)), CG_NAMES + ": " + OUT_IN),
    (CG, dict(work=("sh", CF * SH - 4)), CG_NAMES + ": " + OUT_IN),
    (CG, dict(den=("o1", CUBE - 4)), CG_NAMES + ": " + OUT_IN),
    (CG, dict(work=("o1", CUBE - 4)), CG_NAMES + ": " + OUT_OUT),
]


def case_id(case):
    entry, fault, _ = case
    return entry[4:] + ":" + ",".join(f"{k}={'+'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in fault.items())


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
    assert vis.numel() * 4 == PLANES4 == fs.out_bytes and fs.interpolate_bytes(3) == PLANES3
    assert fs.sh_work_bytes(C) == WORK and fs.sh_work_bytes(0) == 0 and fs.sh_work_bytes(abi.SH_MAX_CH + 1) == 0
    assert main.cube_sh_work_bytes(N, C, CF) == CWORK and CWORK < PLANES4 and CUBE < PLANES4
    fs.render_visibility(vis.data_ptr(), PLANES4, F, stream())
    torch.cuda.synchronize()
    ones = lambda n: torch.ones(n, dtype=torch.float32, device="cuda")  # noqa: E731
    k.buf = {"vis": vis, "nrm": ones(PLANES4 // 4), "g": ones(PLANES4 // 4), "sh": ones(PLANES4 // 4) * 0.5, "src": ones(PLANES4 // 4) * 2.0,
             "den": ones(PLANES4 // 4) * 3.0}
    for name in ("o1", "o2", "o3"):
        k.buf[name] = torch.full((PLANES4 // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    k.before = {name: t.clone() for name, t in k.buf.items()}
    yield k
    for fs in k.fs.values():
        fs.close()
    main.close(), sharded.close()


def call(kit, entry, fault):
    """one call of `entry` with ENTRIES' arguments, those of `fault` in their place -> (return code, the ctx handle passed)"""
    of_set = entry.startswith("srz_frameset")
    args = dict(ctx="main", **(dict(fs="main") if of_set else {}), **ENTRIES[entry])
    assert set(fault) <= set(args), (entry, fault)
    args.update(fault)
    h = kit.ctx[args.pop("ctx")].h if args["ctx"] is not None else args.pop("ctx")
    head = [h]
    if of_set:
        head.append(kit.fs[args.pop("fs")].h if args["fs"] is not None else args.pop("fs"))
    values = [kit.buf[v[0]].data_ptr() + v[1] if isinstance(v, tuple) else v for v in args.values()]
    return getattr(srz.lib(), entry)(*head, *values, None), h


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
        assert L_.srz_last_error(h).decode() == (text if text is WRONG_SHARD else entry + text)
    torch.cuda.synchronize()
    for name, t in kit.buf.items():
        assert torch.equal(t, kit.before[name]), f"{name} was written"


def test_the_valid_calls_are_accepted(kit):
    """ENTRIES' arguments are a valid call of every entry point, and so are the calls that leave out what may be left out: the
    refusals above are each due to the one argument their row changes"""
    for entry, fault in ((FS, {}), (FS, dict(sh_frames=2)), (FS, dict(kind=1)), (FS, dict(n_ch=1)), (FG, {}), (FG, dict(sh_frames=2)), (FG, dict(kind=1)), (FG, dict(gsh=None, work=None, work_bytes=0)), (FG, dict(gnrm=None)),
                         (FG, dict(gsh=None, work=("sh", 2), work_bytes=0)),  # (without d_gsh, d_work is not looked at)
                         (CS, {}), (CS, dict(den=None)), (CS, dict(tex_frames=1)), (CG, {})):
        rc, h = call(kit, entry, fault)
        torch.cuda.synchronize()
        assert rc == 0, (entry, fault, srz.lib().srz_last_error(h))
    for name in ("o1", "o2", "o3"):
        assert not torch.equal(kit.buf[name], kit.before[name]), name
    for name, t in kit.buf.items():  # (the outputs are written now: the sentinels go back for whatever runs next)
        t.copy_(kit.before[name])


def test_the_torch_layer_refuses(kit):
    """srz.visibility's own refusals for the two functions — ValueError before a pointer leaves Python —, and the library's for what
    the layer leaves to it: more channels than SRZ_SH_MAX_CH"""
    from srz import visibility as V
    fs = kit.fs["main"]
    vis = kit.buf["vis"]
    nrm = torch.ones(fs.interpolate_shape(3), dtype=torch.float32, device="cuda")
    sh = torch.ones((9, C), dtype=torch.float32, device="cuda")
    assert tuple(V.sh_light(fs, vis, sh, nrm).shape) == tuple(fs.interpolate_shape(C))
    for bad, words in ((dict(sh=sh.cpu()), "sh_light: sh must be a CUDA float32 tensor [9, C] or [n_frames, 9, C]"),
                       (dict(sh=sh[:8]), "sh_light: sh must be"), (dict(sh=sh.double()), "sh_light: sh must be"), (dict(sh=None), "sh_light: sh must be"),
                       (dict(sh=sh[None].repeat(3, 1, 1)), "sh_light: sh has 3 frames, the set 2"),
                       (dict(nrm=nrm[:, :2]), "sh_light: nrm must be"), (dict(nrm=nrm.cpu()), "sh_light: nrm must be"),
                       (dict(vis=vis[:1]), "sh_light: vis: expected a contiguous CUDA float32 tensor")):
        args = dict(vis=vis, sh=sh, nrm=nrm, kind="irradiance")
        args.update(bad)
        with pytest.raises(ValueError) as e:
            V.sh_light(fs, args["vis"], args["sh"], args["nrm"], args["kind"])
        assert str(e.value).startswith(words), (bad.keys(), str(e.value))
    g = torch.ones(fs.interpolate_shape(C), dtype=torch.float32, device="cuda")
    for bad, words in ((dict(gout=g[:, :2]), "sh_light_grad: gout must be float32"), (dict(gout=g.cpu()), "sh_light_grad: gout must be on the device"),
                       (dict(gout=None), "sh_light_grad: gout must be")):
        with pytest.raises(ValueError) as e:
            V.sh_light_grad(fs, vis, sh, nrm, bad["gout"])
        assert str(e.value).startswith(words), str(e.value)
    # what the layer leaves to the library: a call that asks for no gradient, an unknown kind, more channels than SRZ_SH_MAX_CH
    with pytest.raises(srz.SrzError, match="srz_frameset_sh_grad: neither d_gnrm nor d_gsh is asked for"):
        V.sh_light_grad(fs, vis, sh, nrm, g, want_gsh=False, want_gnrm=False)
    with pytest.raises(srz.SrzError, match="srz_frameset_sh: kind must be SRZ_SH_IRRADIANCE or SRZ_SH_RADIANCE"):
        V.sh_light(fs, vis, sh, nrm, "diffuse")
    assert not torch.equal(V.sh_light(fs, vis, sh, nrm, "radiance"), V.sh_light(fs, vis, sh, nrm))  # (the two kinds the layer knows)
    wide = torch.ones((9, abi.SH_MAX_CH + 1), dtype=torch.float32, device="cuda")
    with pytest.raises(srz.SrzError, match="srz_frameset_sh: n_ch must be 1 .. SRZ_SH_MAX_CH"):
        V.sh_light(fs, vis, wide, nrm)
    cube = torch.ones((6, 4, 4, C), dtype=torch.float32, device="cuda")
    assert tuple(V.cube_sh(fs, cube).shape) == (9, C) and tuple(V.cube_sh(kit.ctx["main"], cube[None].repeat(2, 1, 1, 1, 1)).shape) == (2, 9, C)
    for bad in (cube.cpu(), cube[:5], cube[:, :3], cube.double(), None):
        with pytest.raises(ValueError, match="cube_sh: a cube is a CUDA float32 tensor"):
            V.cube_sh(fs, bad)
    with pytest.raises(srz.SrzError, match="srz_cube_sh: n_ch must be 1 .. SRZ_SH_MAX_CH"):
        V.cube_sh(fs, torch.ones((6, 4, 4, 8), dtype=torch.float32, device="cuda"))
    den = torch.ones(1, dtype=torch.float32, device="cuda")
    for gsh, d in ((sh.cpu(), den), (sh[:8], den), (sh, den.cpu()), (sh, torch.ones(2, device="cuda")), (sh, None)):
        with pytest.raises(ValueError, match="cube_sh_grad: (gsh|den) must be"):
            V.cube_sh_grad(fs, gsh, d, 4)
