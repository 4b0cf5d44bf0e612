"""-m gpu: what srz_frameset_texture_set / _texture_set_grad refuse.  Every refusal of include/srz.h's list gives SRZ_E_INVALID,
srz_last_error names the function, every output still holds what it held (nothing was launched), and the valid call beside each
fault is accepted — so that a refusal is the fault's, not the kit's.  Then the ValueErrors of srz.visibility's layer."""
import ctypes as C

import pytest
import torch

import srz
import texsetref
from srz import abi, visibility
from support import ctx, filled, visibility as render_visibility, words  # noqa: F401

pytestmark = pytest.mark.gpu

F, E = abi.FUSED_CLEAR, abi.SRZ_E_INVALID
SENTINEL = 0x5eed5eed
NCH = 3
FWD, BWD = "srz_frameset_texture_set", "srz_frameset_texture_set_grad"


class Kit:
    def __init__(self, ctx):
        self.ctx = ctx
        self.fs = ctx.frameset([texsetref.three_frame(2), texsetref.three_frame(5)])
        fs = self.fs
        self.vis = render_visibility(fs)
        self.uv = torch.rand(fs.interpolate_shape(2), dtype=torch.float32, device="cuda")
        self.gout = torch.rand(fs.interpolate_shape(NCH), dtype=torch.float32, device="cuda")
        self.tex = [torch.rand((7, 5, NCH), dtype=torch.float32, device="cuda"), torch.rand((2, 1, 33, NCH), dtype=torch.float32, device="cuda")]
        self.map = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
        # outputs, each with room behind it for a shifted pointer
        self.out = filled((fs.interpolate_bytes(NCH) // 4 + 4,), SENTINEL)
        self.guv = filled((fs.interpolate_bytes(2) // 4 + 4,), SENTINEL)
        self.gtex = [filled((t.numel() + 4,), SENTINEL) for t in self.tex]

    def outputs(self):
        return [self.out, self.guv] + self.gtex

    def args(self, entry):
        """the valid call's arguments by name"""
        a = dict(d_vis=self.vis.data_ptr(), d_uv=self.uv.data_ptr(), n_slots=2, d_batch_slot=self.map.data_ptr(), n_batch_slot=3, n_ch=NCH, flags=F,
                 slots=[dict(d_tex=self.tex[0].data_ptr(), d_gtex=None, tex_w=5, tex_h=7, tex_frames=1, mode=abi.TEX_CLAMP),
                        dict(d_tex=self.tex[1].data_ptr(), d_gtex=None, tex_w=33, tex_h=1, tex_frames=2, mode=abi.TEX_WRAP)], fs=self.fs.h)
        if entry == FWD:
            a.update(d_out=self.out.data_ptr(), out_bytes=self.fs.interpolate_bytes(NCH))
        else:
            a.update(d_gout=self.gout.data_ptr(), d_guv=self.guv.data_ptr())
            for s in range(2):
                a["slots"][s]["d_gtex"] = self.gtex[s].data_ptr()
        return a

    def call(self, entry, a):
        L = srz.lib()
        arr = None
        if a["slots"] is not None:
            arr = abi.texset_slots_array([(s["d_tex"], s["d_gtex"], s["tex_w"], s["tex_h"], s["tex_frames"], s["mode"]) for s in a["slots"]])
        vp = lambda x: C.c_void_p(x or None)  # noqa: E731
        if entry == FWD:
            return L.srz_frameset_texture_set(self.ctx.h, a["fs"], vp(a["d_vis"]), vp(a["d_uv"]), arr, a["n_slots"], vp(a["d_batch_slot"]),
                                              a["n_batch_slot"], a["n_ch"], vp(a["d_out"]), a["out_bytes"], a["flags"], None)
        return L.srz_frameset_texture_set_grad(self.ctx.h, a["fs"], vp(a["d_vis"]), vp(a["d_uv"]), vp(a["d_gout"]), arr, a["n_slots"],
                                               vp(a["d_batch_slot"]), a["n_batch_slot"], a["n_ch"], vp(a["d_guv"]), a["flags"], None)


@pytest.fixture(scope="module")
def kit(ctx):
    k = Kit(ctx)
    yield k
    k.fs.close()


def top(name, value):
    return lambda k, a: a.__setitem__(name, value(k, a) if callable(value) else value)


def slot(s, name, value):
    return lambda k, a: a["slots"][s].__setitem__(name, value(k, a) if callable(value) else value)


def both(*faults):
    def apply(k, a):
        for f in faults:
            f(k, a)
    return apply


def plus(name, n):
    return lambda k, a: a[name] + n


ALL = (FWD, BWD)
# (what, the entries it applies to, the fault)
CASES = [
    ("null set", ALL, top("fs", None)), ("null d_vis", ALL, top("d_vis", None)), ("null d_uv", ALL, top("d_uv", None)),
    ("null slots", ALL, top("slots", None)), ("null d_batch_slot", ALL, top("d_batch_slot", None)), ("null d_out", (FWD,), top("d_out", None)),
    ("null d_gout", (BWD,), top("d_gout", None)), ("null d_tex in a slot", (FWD,), slot(1, "d_tex", None)),
    ("d_guv with a null d_tex", (BWD,), slot(0, "d_tex", None)),
    ("nothing asked for", (BWD,), both(top("d_guv", None), slot(0, "d_gtex", None), slot(1, "d_gtex", None))),
    ("n_slots 0", ALL, top("n_slots", 0)), ("n_slots 9", ALL, top("n_slots", abi.TEXSET_MAX + 1)),
    ("n_batch_slot 0", ALL, top("n_batch_slot", 0)), ("n_batch_slot 65537", ALL, top("n_batch_slot", 65537)),
    ("n_ch 0", ALL, top("n_ch", 0)), ("n_ch 65", ALL, top("n_ch", abi.ATTR_MAX_CH + 1)),
    ("tex_w 0", ALL, slot(0, "tex_w", 0)), ("tex_w too large", ALL, slot(1, "tex_w", abi.TEX_MAX_SIZE + 1)), ("tex_h 0", ALL, slot(1, "tex_h", 0)),
    ("tex_h too large", ALL, slot(0, "tex_h", abi.TEX_MAX_SIZE + 1)), ("mode 2", ALL, slot(1, "mode", 2)),
    ("tex_frames 3", ALL, slot(0, "tex_frames", 3)), ("tex_frames 0", ALL, slot(1, "tex_frames", 0)),
    ("short out_bytes", (FWD,), top("out_bytes", plus("out_bytes", -1))),
    ("d_vis off by 4", ALL, top("d_vis", plus("d_vis", 4))), ("d_uv off by 8", ALL, top("d_uv", plus("d_uv", 8))),
    ("d_out off by 4", (FWD,), top("d_out", plus("d_out", 4))), ("d_gout off by 4", (BWD,), top("d_gout", plus("d_gout", 4))),
    ("d_guv off by 12", (BWD,), top("d_guv", plus("d_guv", 12))), ("d_tex off by 2", ALL, slot(0, "d_tex", lambda k, a: a["slots"][0]["d_tex"] + 2)),
    ("d_gtex off by 1", (BWD,), slot(1, "d_gtex", lambda k, a: a["slots"][1]["d_gtex"] + 1)),
    ("flags UNIFIED", ALL, top("flags", abi.UNIFIED)), ("flags 0x10", ALL, top("flags", F | 0x10)),
    ("d_out is d_uv", (FWD,), top("d_out", lambda k, a: a["d_uv"])), ("d_out is d_vis", (FWD,), top("d_out", lambda k, a: a["d_vis"])),
    ("d_out is a texture", (FWD,), slot(0, "d_tex", lambda k, a: a["d_out"])),
    ("d_out holds the map", (FWD,), top("d_batch_slot", lambda k, a: a["d_out"] + 64)),
    ("d_guv is d_uv", (BWD,), top("d_guv", lambda k, a: a["d_uv"])), ("d_guv is d_gout", (BWD,), top("d_guv", lambda k, a: a["d_gout"])),
    ("d_guv holds the map", (BWD,), top("d_batch_slot", lambda k, a: a["d_guv"] + 33)),
    ("d_gtex is its d_tex", (BWD,), slot(0, "d_gtex", lambda k, a: a["slots"][0]["d_tex"])),
    ("d_gtex is the other slot's d_tex", (BWD,), slot(0, "d_gtex", lambda k, a: a["slots"][1]["d_tex"])),
    ("two slots' d_gtex overlap", (BWD,), slot(1, "d_gtex", lambda k, a: a["slots"][0]["d_gtex"] + 16)),
    ("d_gtex inside d_guv", (BWD,), slot(1, "d_gtex", lambda k, a: a["d_guv"] + 64)),
    ("d_gtex holds the map", (BWD,), top("d_batch_slot", lambda k, a: a["slots"][0]["d_gtex"] + 5)),
]


@pytest.mark.parametrize("entry,what,fault", [(e, w, f) for (w, es, f) in CASES for e in es], ids=lambda x: x if isinstance(x, str) else "")
def test_refusal(kit, entry, what, fault):
    a = kit.args(entry)
    fault(kit, a)
    before = [t.clone() for t in kit.outputs()]
    assert kit.call(entry, a) == E, what
    msg = srz.lib().srz_last_error(kit.ctx.h).decode()
    assert msg.startswith(entry + ":") or msg.startswith(entry + " ("), (what, msg)
    torch.cuda.synchronize()
    for t, b in zip(kit.outputs(), before):
        assert torch.equal(t, b), what


def test_a_null_ctx_is_refused(kit):
    L = srz.lib()
    assert L.srz_frameset_texture_set(None, kit.fs.h, None, None, None, 1, None, 1, 3, None, 0, 0, None) == E
    assert L.srz_frameset_texture_set_grad(None, kit.fs.h, None, None, None, None, 1, None, 1, 3, None, 0, None) == E


def test_the_valid_calls_and_what_may_alias_are_accepted(kit):
    for entry in ALL:
        assert kit.call(entry, kit.args(entry)) == abi.SRZ_OK, entry
    a = kit.args(FWD)  # two slots MAY share one d_tex, with different modes
    a["slots"][1] = dict(a["slots"][0], mode=abi.TEX_WRAP)
    assert kit.call(FWD, a) == abi.SRZ_OK
    b = kit.args(BWD)  # gtex alone: no d_guv, no d_tex
    b["d_guv"] = None
    b["slots"][0]["d_tex"] = b["slots"][1]["d_tex"] = None
    b["slots"][1]["d_gtex"] = None
    assert kit.call(BWD, b) == abi.SRZ_OK
    torch.cuda.synchronize()
    assert (words(kit.out)[:-4] != SENTINEL).any()


def test_the_visibility_layers_value_errors(kit):
    """the torch layer's own refusals come from the one-place checks of srz/visibility.py (_tex_dims, _lead_frames, _plane, _gout,
    _vis_ptr, _on_device) and from zip(strict=True) over the per-texture flags; the counts are the library's to refuse"""
    fs, vis, uv = kit.fs, kit.vis, kit.uv
    t = torch.rand((7, 5, NCH), dtype=torch.float32, device="cuda")
    bad = [
        dict(texs=[], batch_slot=[0]),  # no texture
        dict(texs=[t, torch.rand((4, 4, 2), device="cuda")], batch_slot=[0, 1]),  # the channel counts differ
        dict(texs=[t.cpu()], batch_slot=[0]), dict(texs=[t.double()], batch_slot=[0]), dict(texs=[t[0]], batch_slot=[0]),
        dict(texs=[torch.rand((3, 7, 5, NCH), device="cuda")], batch_slot=[0]),  # three texture frames, two frames
        dict(texs=[t], batch_slot=torch.zeros(3, dtype=torch.uint8)),  # a map on the host
        dict(texs=[t, t], batch_slot=[0, 1], wrap=[True]), dict(texs=[t], batch_slot=[0], wrap=[True, False]),  # one wrap per texture
        dict(texs=[t], batch_slot=[0], uv=uv[:, :1]), dict(texs=[t], batch_slot=[0], uv=uv.cpu()), dict(texs=[t], batch_slot=[0], vis=vis[:1]),
    ]
    for kw in bad:
        kw = dict(kw)
        u, v = kw.pop("uv", uv), kw.pop("vis", vis)
        with pytest.raises(ValueError):
            visibility.texture_set(fs, v, kw.pop("texs"), u, kw.pop("batch_slot"), **kw)
    for texs, batch_slot in (([t] * 9, [0]), ([t], [])):  # the counts: the library's refusal
        with pytest.raises(srz.SrzError):
            visibility.texture_set(fs, vis, texs, uv, batch_slot)
    g = torch.rand(fs.interpolate_shape(NCH), dtype=torch.float32, device="cuda")
    for kw in (dict(want_gtex=[True, False]), dict(gout=g[:, :2]), dict(gout=g.cpu())):
        kw = dict(kw)
        with pytest.raises(ValueError):
            visibility.texture_set_grad(fs, vis, [t], uv, kw.pop("gout", g), [0, 0, 0], **kw)
    with pytest.raises(srz.SrzError):  # nothing asked for
        visibility.texture_set_grad(fs, vis, [t], uv, g, [0, 0, 0], want_gtex=False, want_guv=False)
    out = visibility.texture_set(fs, vis, [t, t], uv, [0, None, 1], wrap=[False, True])  # and the valid calls go through
    assert tuple(out.shape) == tuple(fs.interpolate_shape(NCH))
    m = torch.tensor([0, abi.TEXSET_NONE, 1], dtype=torch.int32, device="cuda")  # (a map of another integer type is converted)
    assert torch.equal(visibility.texture_set(fs, vis, [t, t], uv, m, wrap=[False, True]), out)
    none = visibility.texture_set(fs, vis, [t], uv, [None, None, None])
    for batch_slot in ([256, -1, 4096], [255, 1, 8]):  # an int that is no index of texs is "no slot", whatever its low byte says
        assert torch.equal(visibility.texture_set(fs, vis, [t], uv, batch_slot), none) and not bool(none.any())
    torch.cuda.synchronize()
