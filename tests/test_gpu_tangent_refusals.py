"""-m gpu: what srz_mesh_tangents / _tangents_grad and srz_frameset_normal_map / _normal_map_grad refuse, and in which words.  One
call per row of CASES: every argument is valid but the one(s) the row names, so the call has exactly one fault; it must return
SRZ_E_INVALID, leave the row's text in srz_last_error, and touch no buffer.  Nothing reaches a kernel: every call is refused on the
host.  (tests/test_gpu_light_refusals.py's scheme.)"""
import types

import pytest
import torch

import srz
import vgkit
from srz import abi
from support import frame, soup, stream

pytestmark = pytest.mark.gpu

F, E = abi.FUSED_CLEAR, abi.SRZ_E_INVALID
SENTINEL = 0x5eed5eed
T, W, H = 24, 64, 64         # triangles per frame, frame size
SLOT, NV = 11, 13            # the mesh slot and its vertex count (vgkit.fan(10, 2))
PLANES4 = 2 * 4 * H * W * 4  # bytes of a visibility buffer of the two-frame set, and of a four-plane buffer
PLANES3 = 2 * 3 * H * W * 4  # bytes of every three-plane buffer
POS2, UV1, TAN2 = 2 * NV * 3 * 4, NV * 2 * 4, 2 * NV * 4 * 4  # bytes of two packed position sets, one uv set, two sets of tangents
WRONG_SHARD = "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)"
ONLY_FUSED = "only SRZ_FUSED_CLEAR is accepted in flags"
FWD_16 = "the plane buffers (d_vis, d_nrm, d_tan, d_m, d_out) must be 16-byte aligned"
BWD_16 = "the plane buffers (d_vis, d_nrm, d_tan, d_m, d_gout, d_gnrm, d_gtan, d_gm) must be 16-byte aligned"
FWD_NAMES = " (d_out against d_vis, d_nrm, d_tan, d_m)"
BWD_NAMES = " (d_gnrm, d_gtan, d_gm against d_vis, d_nrm, d_tan, d_m, d_gout)"
OUT_IN, OUT_OUT = "an output overlaps an input", "two outputs overlap"
NO_MESH, N_SETS, OWN_ONE = "no mesh in that slot", "n_sets must be 1 .. 65535", "the slot's own vertices are one set (n_sets must be 1)"
ALIGN4 = "the buffers must be 4-byte aligned"
TAN_OVER = "the tangents overlap the positions or the uv"

# entry point -> its arguments after ctx (and fs), in order, each with the value of a valid call.  (name, offset): the address of a
# buffer of the kit plus `offset` bytes — vis: a visibility buffer; nrm, tan, m, g, pos, uv: inputs of PLANES4 bytes; o1 .. o3:
# sentinel-filled outputs of PLANES4 + 256 bytes.
ENTRIES = {
    "srz_mesh_tangents": dict(mesh_id=SLOT, pos=("pos", 0), pos_stride=3, n_sets=2, uv=("uv", 0), uv_stride=2, tan=("o1", 0), tan_stride=4),
    "srz_mesh_tangents_grad": dict(mesh_id=SLOT, pos=("pos", 0), pos_stride=3, n_sets=2, uv=("uv", 0), uv_stride=2, gtan=("g", 0), gtan_stride=4,
                                   work=("o1", 0), gpos=("o2", 0)),
    "srz_frameset_normal_map": dict(vis=("vis", 0), nrm=("nrm", 0), tan=("tan", 0), m=("m", 0), out=("o1", 0), out_bytes=PLANES3, flags=F),
    "srz_frameset_normal_map_grad": dict(vis=("vis", 0), nrm=("nrm", 0), tan=("tan", 0), m=("m", 0), gout=("g", 0), gnrm=("o1", 0),
                                         gtan=("o2", 0), gm=("o3", 0), flags=F),
}
MT, MG, NM, NG = ENTRIES  # the four names

# (entry point, the faulty argument(s), text after the entry point's name; WRONG_SHARD stands alone; None: no text is set)
CASES = [
    (MT, dict(ctx=None), None),
    (MT, dict(mesh_id=-1), ": " + NO_MESH),
    (MT, dict(mesh_id=256), ": " + NO_MESH),
    (MT, dict(mesh_id=200), ": " + NO_MESH),
    (MT, dict(n_sets=0), ": " + N_SETS),
    (MT, dict(n_sets=65536), ": " + N_SETS),
    (MT, dict(pos=None), ": " + OWN_ONE),
    (MT, dict(pos_stride=2), ": pos_stride must be at least 3"),
    (MT, dict(uv_stride=1), ": uv_stride must be at least 2"),
    (MT, dict(uv_stride=0), ": uv_stride must be at least 2"),
    (MT, dict(tan=None), ": null d_tan (a vertex record has no tangent field)"),
    (MT, dict(tan=None, pos=None, uv=None, n_sets=1), ": null d_tan (a vertex record has no tangent field)"),  # no in-place record form
    (MT, dict(tan_stride=3), ": tan_stride must be at least 4"),
    (MT, dict(pos=("pos", 2)), ": " + ALIGN4),
    (MT, dict(uv=("uv", 1)), ": " + ALIGN4),
    (MT, dict(tan=("o1", 2)), ": " + ALIGN4),
    (MT, dict(tan=("pos", POS2 - 4)), ": " + TAN_OVER),           # the first tangent float on the positions' last
    (MT, dict(pos=("o1", TAN2 - 4)), ": " + TAN_OVER),            # the positions' first float on the tangents' last
    (MT, dict(tan=("uv", UV1 - 4)), ": " + TAN_OVER),
    (MT, dict(uv=("o1", 16), uv_stride=8), ": " + TAN_OVER),       # uv read from records the tangents are written into
    (MT, dict(pos=("o1", 0), pos_stride=8, tan=("o1", 12), tan_stride=8), ": " + TAN_OVER),  # records: no field for a tangent

    (MG, dict(ctx=None), None),
    (MG, dict(mesh_id=-1), ": " + NO_MESH),
    (MG, dict(mesh_id=200), ": " + NO_MESH),
    (MG, dict(n_sets=0), ": " + N_SETS),
    (MG, dict(n_sets=65536), ": " + N_SETS),
    (MG, dict(pos=None), ": " + OWN_ONE),
    (MG, dict(pos_stride=2), ": pos_stride must be at least 3"),
    (MG, dict(uv_stride=1), ": uv_stride must be at least 2"),
    (MG, dict(gtan=None), ": null tangent gradient / workspace / output"),
    (MG, dict(work=None), ": null tangent gradient / workspace / output"),
    (MG, dict(gpos=None), ": null tangent gradient / workspace / output"),
    (MG, dict(gtan_stride=3), ": gtan_stride must be at least 4"),
    (MG, dict(pos=("pos", 2)), ": " + ALIGN4),
    (MG, dict(uv=("uv", 2)), ": " + ALIGN4),
    (MG, dict(gtan=("g", 1)), ": " + ALIGN4),
    (MG, dict(work=("o1", 2)), ": " + ALIGN4),
    (MG, dict(gpos=("o2", 3)), ": " + ALIGN4),
    (MG, dict(gpos=("pos", POS2 - 4)), ": " + OUT_IN),
    (MG, dict(work=("pos", 0)), ": " + OUT_IN),
    (MG, dict(gpos=("uv", UV1 - 4)), ": " + OUT_IN),
    (MG, dict(work=("uv", 0)), ": " + OUT_IN),
    (MG, dict(gpos=("g", TAN2 - 4)), ": " + OUT_IN),
    (MG, dict(gtan=("o1", POS2 - 4)), ": " + OUT_IN),
    (MG, dict(gpos=("o1", POS2 - 4)), ": " + OUT_OUT),

    (NM, dict(ctx=None), None),
    (NM, dict(fs=None), ": null frameset"),
    (NM, dict(vis=None), ": null d_vis"),
    (NM, dict(nrm=None), ": null d_nrm"),
    (NM, dict(tan=None), ": null d_tan"),
    (NM, dict(m=None), ": null d_m"),
    (NM, dict(out=None), ": null d_out"),
    (NM, dict(out_bytes=PLANES3 - 1), ": out_bytes is too small for d_out"),
    (NM, dict(flags=abi.UNIFIED), ": " + ONLY_FUSED),
    (NM, dict(flags=F | abi.ORDERED_RASTER), ": " + ONLY_FUSED),
    (NM, dict(vis=("vis", 4)), ": " + FWD_16),
    (NM, dict(nrm=("nrm", 8)), ": " + FWD_16),
    (NM, dict(tan=("tan", 4)), ": " + FWD_16),
    (NM, dict(m=("m", 12)), ": " + FWD_16),
    (NM, dict(out=("o1", 4)), ": " + FWD_16),
    (NM, dict(out=("vis", 64)), FWD_NAMES + ": " + OUT_IN),
    (NM, dict(out=("nrm", 0)), FWD_NAMES + ": " + OUT_IN),
    (NM, dict(out=("tan", PLANES4 - 16)), FWD_NAMES + ": " + OUT_IN),   # the tangents are four planes: their last quad
    (NM, dict(out=("m", 16)), FWD_NAMES + ": " + OUT_IN),
    (NM, dict(nrm=("o1", PLANES3 - 16)), FWD_NAMES + ": " + OUT_IN),
    (NM, dict(ctx="sharded"), WRONG_SHARD),

    (NG, dict(ctx=None), None),
    (NG, dict(fs=None), ": null frameset"),
    (NG, dict(vis=None), ": null d_vis"),
    (NG, dict(nrm=None), ": null d_nrm"),
    (NG, dict(tan=None), ": null d_tan"),
    (NG, dict(m=None), ": null d_m"),
    (NG, dict(gout=None), ": null d_gout"),
    (NG, dict(gnrm=None, gtan=None, gm=None), ": none of d_gnrm, d_gtan, d_gm is asked for"),
    (NG, dict(flags=16), ": " + ONLY_FUSED),
    (NG, dict(vis=("vis", 4)), ": " + BWD_16),
    (NG, dict(nrm=("nrm", 4)), ": " + BWD_16),
    (NG, dict(tan=("tan", 8)), ": " + BWD_16),
    (NG, dict(m=("m", 4)), ": " + BWD_16),
    (NG, dict(gout=("g", 8)), ": " + BWD_16),
    (NG, dict(gnrm=("o1", 4)), ": " + BWD_16),
    (NG, dict(gtan=("o2", 8)), ": " + BWD_16),
    (NG, dict(gm=("o3", 4)), ": " + BWD_16),
    (NG, dict(gnrm=("vis", 16)), BWD_NAMES + ": " + OUT_IN),
    (NG, dict(gnrm=("nrm", 0)), BWD_NAMES + ": " + OUT_IN),
    (NG, dict(gtan=("tan", 0)), BWD_NAMES + ": " + OUT_IN),
    (NG, dict(gm=("tan", PLANES4 - 16)), BWD_NAMES + ": " + OUT_IN),
    (NG, dict(gm=("m", PLANES3 - 16)), BWD_NAMES + ": " + OUT_IN),
    (NG, dict(gtan=("g", 0)), BWD_NAMES + ": " + OUT_IN),
    (NG, dict(gout=("o2", PLANES4 - 16)), BWD_NAMES + ": " + OUT_IN),   # the last quad of the four-plane gtan
    (NG, dict(gtan=("o1", PLANES3 - 16)), BWD_NAMES + ": " + OUT_OUT),
    (NG, dict(gm=("o2", PLANES4 - 16)), BWD_NAMES + ": " + OUT_OUT),
    (NG, dict(gm=("o1", 16)), BWD_NAMES + ": " + OUT_OUT),
    (NG, dict(ctx="sharded"), WRONG_SHARD),
]


def case_id(case):
    entry, fault, _ = case
    return entry[4:] + ":" + ",".join(f"{k}={'+'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in fault.items())


assert len({case_id(c) for c in CASES}) == len(CASES)


@pytest.fixture(scope="module")
def kit():
    """the contexts, the mesh, the set and the buffers every case draws its arguments from"""
    tris = soup(3, T, W, H, (10.0, 20.0, 30.0))
    main, sharded = srz.Context(0), srz.Context(0, 0, 2)
    k = types.SimpleNamespace(ctx={"main": main, "sharded": sharded})
    pos, faces = vgkit.fan(10, 2)
    assert len(pos) == NV
    main.mesh_upload(SLOT, vgkit.verts8(pos), faces)
    k.fs = {"main": main.frameset([frame(tris, W, H), frame(tris[::-1].copy(), W, H)])}
    vis = torch.zeros(k.fs["main"].out_shape, dtype=torch.float32, device="cuda")
    assert vis.numel() * 4 == PLANES4 == k.fs["main"].out_bytes == k.fs["main"].interpolate_bytes(4) and k.fs["main"].interpolate_bytes(3) == PLANES3
    k.fs["main"].render_visibility(vis.data_ptr(), PLANES4, F, stream())
    torch.cuda.synchronize()
    rnd = lambda seed: torch.rand(PLANES4 // 4, dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(seed)) + 0.1  # noqa: E731
    k.buf = {"vis": vis, "nrm": rnd(1), "tan": rnd(2), "m": rnd(3), "g": rnd(4), "pos": rnd(5), "uv": rnd(6)}
    for name in ("o1", "o2", "o3"):
        k.buf[name] = torch.full((PLANES4 // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    k.before = {name: t.clone() for name, t in k.buf.items()}
    yield k
    for fs in k.fs.values():
        fs.close()
    main.close(), sharded.close()


def call(kit, entry, fault):
    """one call of `entry` with ENTRIES' arguments, those of `fault` in their place -> (return code, the ctx handle passed)"""
    on_set = entry.startswith("srz_frameset_")
    args = dict(ctx="main", **(dict(fs="main") if on_set else {}), **ENTRIES[entry])
    assert set(fault) <= set(args), (entry, fault)
    args.update(fault)
    ctx = args.pop("ctx")
    h = kit.ctx[ctx].h if ctx is not None else None
    head = [h]
    if on_set:
        fs = args.pop("fs")
        head.append(kit.fs[fs].h if fs is not None else None)
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
    """ENTRIES' arguments are a valid call of every entry point, and so are the calls that leave out what may be left out or put
    buffers right behind one another: the refusals above are each due to the argument(s) their row changes"""
    for entry, fault in ((MT, {}), (MT, dict(pos=None, n_sets=1)), (MT, dict(uv=None)), (MT, dict(pos=None, uv=None, n_sets=1)),
                         (MT, dict(tan=("pos", POS2))), (MT, dict(pos=("o1", TAN2))), (MT, dict(tan_stride=7, uv_stride=3, pos_stride=4)),
                         (MG, {}), (MG, dict(pos=None, uv=None, n_sets=1)), (MG, dict(gpos=("o1", POS2))), (MG, dict(gtan_stride=6)),
                         (NM, {}), (NG, {}), (NG, dict(gnrm=None)), (NG, dict(gtan=None)), (NG, dict(gm=None)),
                         (NG, dict(gnrm=None, gtan=None))):
        rc, h = call(kit, entry, fault)
        assert rc == 0, (entry, fault, srz.lib().srz_last_error(h))
        torch.cuda.synchronize()
    for name in ("o1", "o2", "o3"):
        assert not torch.equal(kit.buf[name], kit.before[name]), name
    for name, t in kit.buf.items():  # (the outputs are written now: the sentinels go back for whatever runs next)
        t.copy_(kit.before[name])
