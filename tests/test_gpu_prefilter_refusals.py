"""-m gpu: what srz_cube_prefilter and srz_cube_prefilter_grad refuse, and in which words.  One call per row of CASES: every
argument is valid but the one(s) the row names, so the call has exactly one fault; it must return SRZ_E_INVALID, leave the row's
text — which names the function — in srz_last_error, and touch no buffer.  Nothing reaches a kernel: every call is refused on the
host.  (tests/test_gpu_cubemip_refusals.py's scheme.)"""
import types

import pytest
import torch

import srz
from srz import abi

pytestmark = pytest.mark.gpu

E = abi.SRZ_E_INVALID
SENTINEL = 0x5eed5eed
NS, ND, C, TF = 8, 4, 3, 2  # source and output size, channels, frames
SRC = TF * 6 * NS * NS * C * 4  # bytes of the source cubes
DST = TF * 6 * ND * ND * C * 4  # bytes of the output cubes
DEN = 6 * ND * ND * 4
SIZES = "n_src and n_dst must be 1 .. SRZ_TEX_MAX_SIZE"
N_CH, FRAMES = "n_ch must be 1 .. SRZ_ATTR_MAX_CH", "tex_frames must be 1 .. 65536"
KIND = "kind must be SRZ_PREFILTER_COSINE or SRZ_PREFILTER_GGX"
ROUGH, CMIN = "roughness must be in [0, 1]", "cmin must be in [0, 1)"
WORK, WORK_16 = "work_bytes is below srz_cube_prefilter_work_bytes", "d_work must be 16-byte aligned"
FWD_4, BWD_4 = "d_src, d_dst and d_den must be 4-byte aligned", "d_gdst, d_den and d_gsrc must be 4-byte aligned"
FWD_OVER, BWD_OVER = " (d_dst, d_den, d_work against d_src)", " (d_gsrc, d_work against d_gdst, d_den)"
OUT_IN, OUT_OUT = ": an output overlaps an input", ": two outputs overlap"
NAN, INF = float("nan"), float("inf")

# entry point -> its arguments after ctx, in order, each with the value of a valid call.  (name, offset): the address of a buffer of
# the kit plus `offset` bytes — src, gdst, den: inputs; o1, o2: sentinel-filled outputs; work: sentinel-filled scratch.
ENTRIES = {
    "cube_prefilter": dict(src=("src", 0), n_src=NS, dst=("o1", 0), n_dst=ND, n_ch=C, tex_frames=TF, kind=abi.PREFILTER_GGX, roughness=0.5, cmin=0.25,
                           den=("o2", 0), work=("work", 0), work_bytes="need"),
    "cube_prefilter_grad": dict(gdst=("gdst", 0), den=("den", 0), n_src=NS, n_dst=ND, n_ch=C, tex_frames=TF, kind=abi.PREFILTER_GGX, roughness=0.5,
                                cmin=0.25, gsrc=("o1", 0), work=("work", 0), work_bytes="need"),
}
FWD, BWD = "cube_prefilter", "cube_prefilter_grad"
BOTH = [(dict(n_src=0), ": " + SIZES), (dict(n_src=abi.TEX_MAX_SIZE + 1), ": " + SIZES), (dict(n_dst=0), ": " + SIZES),
        (dict(n_dst=abi.TEX_MAX_SIZE + 1), ": " + SIZES), (dict(n_ch=0), ": " + N_CH), (dict(n_ch=abi.ATTR_MAX_CH + 1), ": " + N_CH),
        (dict(tex_frames=0), ": " + FRAMES), (dict(tex_frames=65537), ": " + FRAMES), (dict(kind=2), ": " + KIND), (dict(kind=0xffffffff), ": " + KIND),
        (dict(roughness=NAN), ": " + ROUGH), (dict(roughness=INF), ": " + ROUGH), (dict(roughness=-0.125), ": " + ROUGH),
        (dict(roughness=1.0000001), ": " + ROUGH), (dict(cmin=NAN), ": " + CMIN), (dict(cmin=-INF), ": " + CMIN), (dict(cmin=-0.125), ": " + CMIN),
        (dict(cmin=1.0), ": " + CMIN), (dict(work=None), ": null d_work"), (dict(work_bytes="short"), ": " + WORK), (dict(work_bytes=0), ": " + WORK),
        (dict(work=("work", 4)), ": " + WORK_16), (dict(work=("work", 8)), ": " + WORK_16)]

# (entry point, the faulty argument(s), text after "srz_<entry point>"; None: no text is set)
CASES = [(e, f, t) for e in (FWD, BWD) for f, t in BOTH] + [
    (FWD, dict(ctx=None), None),
    (FWD, dict(src=None), ": null d_src"),
    (FWD, dict(dst=None), ": null d_dst"),
    (FWD, dict(src=("src", 2)), ": " + FWD_4),
    (FWD, dict(dst=("o1", 1)), ": " + FWD_4),
    (FWD, dict(den=("o2", 2)), ": " + FWD_4),
    (FWD, dict(dst=("src", 0)), FWD_OVER + OUT_IN),
    (FWD, dict(dst=("src", SRC - 4)), FWD_OVER + OUT_IN),
    (FWD, dict(den=("src", 4)), FWD_OVER + OUT_IN),
    (FWD, dict(work=("src", 16)), FWD_OVER + OUT_IN),
    (FWD, dict(src=("work", 32)), FWD_OVER + OUT_IN),
    (FWD, dict(den=("o1", DST - 4)), FWD_OVER + OUT_OUT),
    (FWD, dict(dst=("work", 64)), FWD_OVER + OUT_OUT),
    (FWD, dict(work=("o2", 0)), FWD_OVER + OUT_OUT),

    (BWD, dict(ctx=None), None),
    (BWD, dict(gdst=None), ": null d_gdst"),
    (BWD, dict(den=None), ": null d_den"),
    (BWD, dict(gsrc=None), ": null d_gsrc"),
    (BWD, dict(gdst=("gdst", 2)), ": " + BWD_4),
    (BWD, dict(den=("den", 1)), ": " + BWD_4),
    (BWD, dict(gsrc=("o1", 2)), ": " + BWD_4),
    (BWD, dict(gsrc=("gdst", DST - 4)), BWD_OVER + OUT_IN),
    (BWD, dict(gsrc=("den", 0)), BWD_OVER + OUT_IN),
    (BWD, dict(work=("gdst", 16)), BWD_OVER + OUT_IN),
    (BWD, dict(den=("work", 16)), BWD_OVER + OUT_IN),
    (BWD, dict(gsrc=("work", 4)), BWD_OVER + OUT_OUT),
    (BWD, dict(work=("o1", SRC - 16)), BWD_OVER + OUT_OUT),
]


def case_id(case):
    entry, fault, _ = case
    return entry + ":" + ",".join(f"{k}={'+'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in fault.items())


assert len({case_id(c) for c in CASES}) == len(CASES)


@pytest.fixture(scope="module")
def kit():
    """the context and the buffers every case draws its arguments from"""
    k = types.SimpleNamespace(ctx=srz.Context(0))
    k.need = k.ctx.cube_prefilter_work_bytes(NS, ND, C, TF)
    assert k.need >= 16 and k.need % 4 == 0 and k.ctx.cube_prefilter_work_bytes(0, ND, C, TF) == 0
    big = max(k.need, SRC) + 256
    ones = lambda nbytes: torch.ones(nbytes // 4, dtype=torch.float32, device="cuda")  # noqa: E731
    out = lambda: torch.full((big // 4,), SENTINEL, dtype=torch.int32, device="cuda")  # noqa: E731
    k.buf = {"src": ones(big), "gdst": ones(big), "den": ones(big), "o1": out(), "o2": out(), "work": out()}
    k.before = {name: t.clone() for name, t in k.buf.items()}
    yield k
    k.ctx.close()


def call(kit, entry, fault):
    """one call of srz_<entry> with ENTRIES' arguments, those of `fault` in their place -> (return code, the ctx handle passed)"""
    args = dict(ctx="main", **ENTRIES[entry])
    assert set(fault) <= set(args), (entry, fault)
    args.update(fault)
    h = kit.ctx.h if args.pop("ctx") is not None else None
    values = [kit.buf[v[0]].data_ptr() + v[1] if isinstance(v, tuple) else {"need": kit.need, "short": kit.need - 1}.get(v, v) for v in args.values()]
    return getattr(srz.lib(), "srz_" + entry)(h, *values, None), h


def untouched(kit):
    torch.cuda.synchronize()
    for name, t in kit.buf.items():
        assert torch.equal(t, kit.before[name]), f"{name} was written"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_refusal(kit, case):
    entry, fault, text = case
    lib, h0 = srz.lib(), kit.ctx.h
    # the context's text is first set to another refusal's, so that a stale text cannot stand in for the one expected
    marker = "srz_frameset_render: null frameset / output"
    assert lib.srz_frameset_render(h0, None, None, 0, 0, None) == E and lib.srz_last_error(h0).decode() == marker
    created = lib.srz_last_error(None)
    rc, h = call(kit, entry, fault)
    assert rc == E, (rc, lib.srz_last_error(h))
    if text is None:  # (no context to leave a text in: nobody's text changes)
        assert h is None and lib.srz_last_error(None) == created and lib.srz_last_error(h0).decode() == marker
    else:
        assert lib.srz_last_error(h).decode() == f"srz_{entry}{text}"
    untouched(kit)


def test_the_valid_calls_are_accepted(kit):
    """ENTRIES' arguments are a valid call of each entry point, and so are the calls at the ends of the ranges and without d_den: the
    refusals above are each due to the argument(s) their row changes"""
    for entry, fault in ((FWD, {}), (FWD, dict(den=None)), (FWD, dict(kind=abi.PREFILTER_COSINE, roughness=0.0, cmin=0.0)),
                         (FWD, dict(roughness=1.0, cmin=0.99999994)), (BWD, {}), (BWD, dict(tex_frames=1, n_ch=1, cmin=0.0))):
        rc, h = call(kit, entry, fault)
        assert rc == 0, (entry, fault, srz.lib().srz_last_error(h))
    torch.cuda.synchronize()
    assert not torch.equal(kit.buf["o1"], kit.before["o1"]) and not torch.equal(kit.buf["o2"], kit.before["o2"])
    for name, t in kit.buf.items():  # (the outputs are written now: the sentinels go back for whatever runs next)
        t.copy_(kit.before[name])
