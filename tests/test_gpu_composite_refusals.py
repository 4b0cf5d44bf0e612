"""-m gpu: what srz_frameset_composite and _composite_grad refuse, and in which words.  One call per row of CASES: every argument
is valid but the one the row names, so the call has exactly one fault; it must return SRZ_E_INVALID, leave the row's text in
srz_last_error, and touch no buffer.  Nothing reaches a kernel: every call is refused on the host.
(tests/test_gpu_background_refusals.py's scheme; the layers are a host array of structs, so the arguments are built here.)"""
import ctypes as C
import types

import pytest
import torch

import srz
from srz import abi
from support import frame, soup, stream

pytestmark = pytest.mark.gpu

F, E = abi.FUSED_CLEAR, abi.SRZ_E_INVALID
SENTINEL = 0x5eed5eed
T, NCH, W, H = 24, 3, 64, 64
PLANE = 2 * H * W * 4        # bytes of one plane of the two-frame set
PLANES4 = 4 * PLANE          # a visibility buffer = the largest buffer any call here names
WRONG_SHARD = "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)"
ONLY_FUSED = "only SRZ_FUSED_CLEAR is accepted in flags"
N_LAYERS, N_CH, THROUGH = "n_layers must be 1 .. SRZ_COMPOSITE_MAX", "n_ch must be 1 .. SRZ_ATTR_MAX_CH", "want_through must be 0 or 1"
LAYER_16 = "the plane buffers (every layer's vis, color, alpha) must be 16-byte aligned"
FWD_16 = "the plane buffers (d_bg, d_out) must be 16-byte aligned"
BWD_16 = "the plane buffers (d_bg, d_gout, d_gcolor[k], d_galpha[k], d_gbg) must be 16-byte aligned"
FWD_NAMES = " (d_out against every layer's vis, color, alpha and d_bg)"
BWD_NAMES = " (d_gcolor, d_galpha, d_gbg against every layer's vis, color, alpha, d_bg and d_gout)"
OUT_IN, OUT_OUT = "an output overlaps an input", "two outputs overlap"

# A buffer is (name, offset in bytes) into the kit: vis, vis2: visibility buffers; c0, c1: colours; a0: an alpha plane; bg; g: gout;
# o1 .. o5: sentinel-filled outputs.  The valid call: two layers, the first with an alpha plane, the second with a scalar opacity.
LAYERS = [dict(vis=("vis", 0), color=("c0", 0), alpha=("a0", 0), opacity=0.0), dict(vis=("vis2", 0), color=("c1", 0), alpha=None, opacity=0.5)]
ENTRIES = {
    "composite": dict(layers=LAYERS, n_layers=2, n_ch=NCH, bg=("bg", 0), through=1, out=("o1", 0), out_bytes=4 * PLANE, flags=F),
    "composite_grad": dict(layers=LAYERS, n_layers=2, n_ch=NCH, bg=("bg", 0), through=1, gout=("g", 0), gcolor=[("o1", 0), ("o2", 0)],
                           galpha=[("o3", 0), ("o4", 0)], gbg=("o5", 0), flags=F),
}


def layer(k, **kw):
    """LAYERS with the fields `kw` of layer k replaced"""
    out = [dict(l) for l in LAYERS]
    out[k].update(kw)
    return out


# (entry point, the faulty argument(s), text after "srz_frameset_<entry point>"; WRONG_SHARD stands alone; None: no text is set)
CASES = [
    ("composite", dict(ctx=None), None),
    ("composite", dict(fs=None), ": null frameset"),
    ("composite", dict(layers=None), ": null layers"),
    ("composite", dict(layers=layer(0, vis=None)), ": null vis in layer 0"),
    ("composite", dict(layers=layer(1, vis=None)), ": null vis in layer 1"),
    ("composite", dict(layers=layer(1, color=None)), ": null color in layer 1"),
    ("composite", dict(out=None), ": null d_out"),
    ("composite", dict(n_layers=0), ": " + N_LAYERS),
    ("composite", dict(n_layers=abi.COMPOSITE_MAX + 1), ": " + N_LAYERS),
    ("composite", dict(n_ch=0), ": " + N_CH),
    ("composite", dict(n_ch=abi.ATTR_MAX_CH + 1), ": " + N_CH),
    ("composite", dict(through=2), ": " + THROUGH),
    ("composite", dict(out_bytes=4 * PLANE - 1), ": out_bytes is too small for d_out"),
    ("composite", dict(out_bytes=3 * PLANE), ": out_bytes is too small for d_out"),  # (enough without the transmittance plane)
    ("composite", dict(flags=abi.UNIFIED), ": " + ONLY_FUSED),
    ("composite", dict(flags=F | abi.ORDERED_RASTER), ": " + ONLY_FUSED),
    ("composite", dict(layers=layer(0, vis=("vis", 4))), ": " + LAYER_16),
    ("composite", dict(layers=layer(1, color=("c1", 8))), ": " + LAYER_16),
    ("composite", dict(layers=layer(0, alpha=("a0", 4))), ": " + LAYER_16),
    ("composite", dict(bg=("bg", 4)), ": " + FWD_16),
    ("composite", dict(out=("o1", 8)), ": " + FWD_16),
    ("composite", dict(out=("vis", 64)), FWD_NAMES + ": " + OUT_IN),
    ("composite", dict(out=("vis2", 16)), FWD_NAMES + ": " + OUT_IN),
    ("composite", dict(layers=layer(1, color=("o1", 4 * PLANE - 16))), FWD_NAMES + ": " + OUT_IN),
    ("composite", dict(layers=layer(0, alpha=("o1", 16))), FWD_NAMES + ": " + OUT_IN),
    ("composite", dict(bg=("o1", 3 * PLANE)), FWD_NAMES + ": " + OUT_IN),
    ("composite", dict(ctx="sharded"), WRONG_SHARD),

    ("composite_grad", dict(ctx=None), None),
    ("composite_grad", dict(fs=None), ": null frameset"),
    ("composite_grad", dict(layers=None), ": null layers"),
    ("composite_grad", dict(layers=layer(0, color=None)), ": null color in layer 0"),
    ("composite_grad", dict(layers=layer(1, vis=None)), ": null vis in layer 1"),
    ("composite_grad", dict(gout=None), ": null d_gout"),
    ("composite_grad", dict(gcolor=None, galpha=None, gbg=None), ": none of d_gcolor, d_galpha, d_gbg is asked for"),
    ("composite_grad", dict(gcolor=[None, None], galpha=[None, None], gbg=None), ": none of d_gcolor, d_galpha, d_gbg is asked for"),
    ("composite_grad", dict(bg=None), ": d_gbg needs d_bg"),
    ("composite_grad", dict(n_layers=0), ": " + N_LAYERS),
    ("composite_grad", dict(n_layers=abi.COMPOSITE_MAX + 1), ": " + N_LAYERS),
    ("composite_grad", dict(n_ch=0), ": " + N_CH),
    ("composite_grad", dict(n_ch=abi.ATTR_MAX_CH + 1), ": " + N_CH),
    ("composite_grad", dict(through=7), ": " + THROUGH),
    ("composite_grad", dict(flags=16), ": " + ONLY_FUSED),
    ("composite_grad", dict(layers=layer(1, vis=("vis2", 8))), ": " + LAYER_16),
    ("composite_grad", dict(bg=("bg", 8)), ": " + BWD_16),
    ("composite_grad", dict(gout=("g", 4)), ": " + BWD_16),
    ("composite_grad", dict(gcolor=[("o1", 0), ("o2", 4)]), ": " + BWD_16),
    ("composite_grad", dict(galpha=[("o3", 8), ("o4", 0)]), ": " + BWD_16),
    ("composite_grad", dict(gbg=("o5", 4)), ": " + BWD_16),
    ("composite_grad", dict(gcolor=[("vis", 16), ("o2", 0)]), BWD_NAMES + ": " + OUT_IN),
    ("composite_grad", dict(gcolor=[("o1", 0), ("c1", 0)]), BWD_NAMES + ": " + OUT_IN),
    ("composite_grad", dict(galpha=[("a0", 0), ("o4", 0)]), BWD_NAMES + ": " + OUT_IN),
    ("composite_grad", dict(galpha=[("o3", 0), ("g", 3 * PLANE)]), BWD_NAMES + ": " + OUT_IN),
    ("composite_grad", dict(gbg=("bg", 16)), BWD_NAMES + ": " + OUT_IN),
    ("composite_grad", dict(gout=("o2", 16)), BWD_NAMES + ": " + OUT_IN),
    ("composite_grad", dict(layers=layer(0, alpha=("o5", 32))), BWD_NAMES + ": " + OUT_IN),
    ("composite_grad", dict(gcolor=[("o1", 0), ("o1", 3 * PLANE - 16)]), BWD_NAMES + ": " + OUT_OUT),
    ("composite_grad", dict(galpha=[("o3", 0), ("o3", PLANE - 16)]), BWD_NAMES + ": " + OUT_OUT),
    ("composite_grad", dict(galpha=[("o1", 16), ("o4", 0)]), BWD_NAMES + ": " + OUT_OUT),
    ("composite_grad", dict(gbg=("o2", 32)), BWD_NAMES + ": " + OUT_OUT),
    ("composite_grad", dict(ctx="sharded"), WRONG_SHARD),
]


def show(v):
    if isinstance(v, tuple):
        return "+".join(map(str, v))
    if isinstance(v, list):
        return "[" + ";".join(show(x) for x in v) + "]"
    if isinstance(v, dict):
        return "{" + ";".join(f"{k}:{show(x)}" for k, x in v.items() if k != "opacity") + "}"
    return str(v)


def case_id(case):
    entry, fault, _ = case
    return entry + ":" + ",".join(f"{k}={show(v)}" for k, v in fault.items())


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
    assert vis.numel() * 4 == PLANES4 == fs.out_bytes and fs.interpolate_bytes(1) == PLANE
    fs.render_visibility(vis.data_ptr(), PLANES4, F, stream())
    torch.cuda.synchronize()
    ones = lambda: torch.ones(PLANES4 // 4 + 64, dtype=torch.float32, device="cuda")  # noqa: E731
    k.buf = {"vis": vis, "vis2": vis.clone(), "c0": ones(), "c1": ones(), "a0": ones(), "bg": ones(), "g": ones()}
    for name in ("o1", "o2", "o3", "o4", "o5"):
        k.buf[name] = torch.full((PLANES4 // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    k.before = {name: t.clone() for name, t in k.buf.items()}
    yield k
    fs.close()
    main.close(), sharded.close()


def call(kit, entry, fault):
    """one call of srz_frameset_<entry> with ENTRIES' arguments, those of `fault` in their place -> (return code, the ctx handle passed)"""
    args = dict(ctx="main", fs="main", **ENTRIES[entry])
    assert set(fault) <= set(args), (entry, fault)
    args.update(fault)
    addr = lambda v: None if v is None else kit.buf[v[0]].data_ptr() + v[1]  # noqa: E731
    h = kit.ctx[args["ctx"]].h if args["ctx"] is not None else None
    fs = kit.fs[args["fs"]].h if args["fs"] is not None else None
    layers = None
    if args["layers"] is not None:
        layers = abi.composite_layers_array([(addr(l["vis"]), addr(l["color"]), addr(l["alpha"]), l["opacity"]) for l in args["layers"]] +
                                            [(0, 0, 0, 0.0)] * abi.COMPOSITE_MAX)  # (room for any n_layers a row passes)
    table = lambda seq: None if seq is None else (C.c_void_p * (abi.COMPOSITE_MAX + 1))(*[addr(v) for v in seq])  # noqa: E731
    L = srz.lib()
    if entry == "composite":
        return L.srz_frameset_composite(h, fs, layers, args["n_layers"], args["n_ch"], addr(args["bg"]), args["through"], addr(args["out"]),
                                        args["out_bytes"], args["flags"], None), h
    return L.srz_frameset_composite_grad(h, fs, layers, args["n_layers"], args["n_ch"], addr(args["bg"]), args["through"], addr(args["gout"]),
                                         table(args["gcolor"]), table(args["galpha"]), addr(args["gbg"]), args["flags"], None), h


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
    """ENTRIES' arguments are a valid call of both entry points, and so are the calls that leave out what may be left out or alias
    inputs with each other (the same buffers as both layers): the refusals above are each due to the one argument their row changes"""
    same_twice = [dict(LAYERS[0]), dict(LAYERS[0])]
    for entry, fault in (("composite", {}), ("composite", dict(bg=None, through=0, out_bytes=3 * PLANE)), ("composite", dict(layers=same_twice)),
                         ("composite", dict(bg=("c0", 0))), ("composite", dict(n_layers=1)), ("composite_grad", {}),
                         ("composite_grad", dict(gcolor=None, galpha=None)), ("composite_grad", dict(bg=None, gbg=None)),
                         ("composite_grad", dict(gcolor=[None, ("o2", 0)], galpha=None, gbg=None)), ("composite_grad", dict(layers=same_twice)),
                         ("composite_grad", dict(through=0))):
        rc, h = call(kit, entry, fault)
        assert rc == 0, (entry, fault, srz.lib().srz_last_error(h))
    torch.cuda.synchronize()
    for name in ("o1", "o2", "o3", "o4", "o5"):
        assert not torch.equal(kit.buf[name], kit.before[name]), name
    for name, t in kit.buf.items():  # (the outputs are written now: the sentinels go back for whatever runs next)
        t.copy_(kit.before[name])
