"""-m gpu: what srz_frameset_texture and srz_frameset_texture_grad refuse.  One call per row: every argument is valid but the one the
row names, so the call has exactly one fault; it must return SRZ_E_INVALID and touch no buffer — every output word is still the
sentinel, every input word what it was.  Nothing reaches a kernel: every call is refused on the host.  The valid calls are accepted."""
import numpy as np
import pytest
import torch

import srz
from srz import abi
from support import SENTINEL, ctx, filled, frame, soup, visibility  # noqa: F401

pytestmark = pytest.mark.gpu

F, E = abi.FUSED_CLEAR, abi.SRZ_E_INVALID
W, H, C, TW, TH = 64, 64, 4, 5, 7
UV_BYTES = 2 * 2 * H * W * 4  # bytes of the uv planes (and of guv) of the two-frame set


def test_refusals_leave_every_buffer_untouched(ctx):
    L = srz.lib()
    t = soup(1, 60, W, H, np.float32([1, 2, 3, 4]))
    fs = ctx.frameset([frame(t, W, H), frame(t[:50], W, H)])
    vis = visibility(fs)
    vis_before = vis.clone()
    uv = torch.full(fs.interpolate_shape(2), 0.25, dtype=torch.float32, device="cuda")
    tex = torch.ones((2, TH, TW, C), dtype=torch.float32, device="cuda")
    gout = torch.ones(fs.interpolate_shape(C), dtype=torch.float32, device="cuda")
    big = filled((2 * 8 * H * W + 64,))  # the outputs are carved from this
    nb, h = fs.interpolate_bytes(C), ctx.h
    v, u, x, g, o = vis.data_ptr(), uv.data_ptr(), tex.data_ptr(), gout.data_ptr(), big.data_ptr()
    o2 = o + UV_BYTES + 64  # a second output behind a guv-sized first one
    tex_bytes = 2 * TH * TW * C * 4

    def f(vis=v, uv=u, tex=x, tw=TW, th=TH, n_ch=C, tf=2, mode=abi.TEX_CLAMP, out=o, ob=nb, flags=F, ctxh=h, fsh=fs.h):
        return L.srz_frameset_texture(ctxh, fsh, vis, uv, tex, tw, th, n_ch, tf, mode, out, ob, flags, None)

    def b(vis=v, uv=u, gout=g, tex=x, tw=TW, th=TH, n_ch=C, tf=2, mode=abi.TEX_WRAP, gtex=o2, guv=o, flags=F, ctxh=h, fsh=fs.h):
        return L.srz_frameset_texture_grad(ctxh, fsh, vis, uv, gout, tex, tw, th, n_ch, tf, mode, gtex, guv, flags, None)
    big_size = abi.TEX_MAX_SIZE + 1
    bad_f = [dict(ctxh=None), dict(fsh=None), dict(vis=None), dict(uv=None), dict(tex=None), dict(out=None),       # null arguments
             dict(tw=0), dict(th=0), dict(tw=big_size), dict(th=big_size), dict(n_ch=0), dict(n_ch=abi.ATTR_MAX_CH + 1),  # sizes, n_ch
             dict(tf=0), dict(tf=3), dict(mode=2), dict(mode=0xffffffff),                                           # tex_frames, mode
             dict(ob=nb - 4), dict(ob=0),                                                                           # a short out_bytes
             dict(vis=v + 4), dict(uv=u + 8), dict(out=o + 4), dict(tex=x + 2),                                     # misaligned pointers
             dict(out=v), dict(out=v + H * W * 4), dict(out=u), dict(out=u + UV_BYTES - 16), dict(out=x), dict(tex=o + 16)]  # overlaps
    bad_b = [dict(ctxh=None), dict(fsh=None), dict(vis=None), dict(uv=None), dict(gout=None), dict(tex=None), dict(gtex=None, guv=None),
             dict(tw=0), dict(th=0), dict(tw=big_size), dict(th=big_size), dict(n_ch=0), dict(n_ch=abi.ATTR_MAX_CH + 1),
             dict(tf=0), dict(tf=3), dict(mode=2), dict(mode=0xffffffff),
             dict(vis=v + 4), dict(uv=u + 8), dict(gout=g + 4), dict(guv=o + 4), dict(gtex=o2 + 2), dict(tex=x + 2),
             dict(guv=v), dict(gtex=v + 32), dict(guv=u), dict(gtex=u + 32), dict(guv=g), dict(gtex=g + 32), dict(gtex=x), dict(guv=x),
             dict(gtex=x + tex_bytes - 4), dict(gtex=o + 32), dict(gtex=o + UV_BYTES - 4)]                          # ... and the other output
    for flag in (abi.UNIFIED, abi.ORDERED_RASTER, abi.NO_Z_READBACK, 16, F | abi.UNIFIED):
        bad_f.append(dict(flags=flag)), bad_b.append(dict(flags=flag))
    for kw in bad_f:
        assert f(**kw) == E, kw
    for kw in bad_b:
        assert b(**kw) == E, kw
    torch.cuda.synchronize()
    sentinel = SENTINEL - (1 << 32)
    assert (big == sentinel).all() and (tex == 1).all() and (gout == 1).all() and (uv == 0.25).all() and torch.equal(vis, vis_before)
    # the valid calls, and the arguments that may be null
    assert f() == 0 and f(tf=1) == 0 and f(mode=abi.TEX_WRAP) == 0 and f(tw=1, th=1) == 0
    assert b() == 0 and b(tex=None, guv=None) == 0 and b(gtex=None) == 0 and b(tf=1) == 0 and b(mode=abi.TEX_CLAMP) == 0
    torch.cuda.synchronize()
    assert (big != sentinel).any()
    fs.close()
