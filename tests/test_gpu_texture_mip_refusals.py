"""-m gpu: what srz_texture_mip_build, srz_texture_mip_fold, srz_frameset_interpolate_deriv, srz_frameset_texture_mip and
srz_frameset_texture_mip_grad refuse.  One call per row: every argument is valid but the one the row names, so the call has exactly
one fault; it must return SRZ_E_INVALID, name its function in the error text and touch no buffer — every output word is still the
sentinel, every input word what it was.  Nothing reaches a kernel: every call is refused on the host.  The valid calls are accepted."""
import numpy as np
import pytest
import torch

import srz
from srz import abi
from support import SENTINEL, ctx, filled, frame, soup, visibility  # noqa: F401

pytestmark = pytest.mark.gpu

F, E = abi.FUSED_CLEAR, abi.SRZ_E_INVALID
W, H, C, TW, TH, NL = 64, 64, 4, 32, 8, 6  # (a 32 x 8 texture has 6 levels)
PLANE = H * W * 4
UV_BYTES = 2 * 2 * PLANE    # bytes of the uv planes (and of guv) of the two-frame set
UVD_BYTES = 2 * 4 * PLANE
TEX_BYTES = 2 * TH * TW * C * 4
SENT = SENTINEL - (1 << 32)


def refused(c, rc, name, kw):
    assert rc == E, (name, kw)
    if kw.get("ctxh", 1) is not None:
        assert name in srz.lib().srz_last_error(c.h).decode(), (name, kw)


def test_build_and_fold_refusals(ctx):
    L = srz.lib()
    mip_bytes = srz.mip_bytes(TW, TH, C, 2, NL)
    assert mip_bytes == 2 * C * 4 * (16 * 4 + 8 * 2 + 4 + 2 + 1)
    tex = torch.ones((2, TH, TW, C), dtype=torch.float32, device="cuda")
    big = filled((TEX_BYTES // 4 + mip_bytes // 4 + 64,))
    x, o = tex.data_ptr(), big.data_ptr()

    def build(tex=x, tw=TW, th=TH, n_ch=C, tf=2, nl=NL, mip=o, mb=mip_bytes, ctxh=ctx.h):
        return L.srz_texture_mip_build(ctxh, tex, tw, th, n_ch, tf, nl, mip, mb, None)

    def fold(gmip=x, mb=mip_bytes, tw=TW, th=TH, n_ch=C, tf=1, nl=NL, gtex=o, ctxh=ctx.h):  # (tex stands for a gradient pyramid of one frame)
        return L.srz_texture_mip_fold(ctxh, gmip, mb, tw, th, n_ch, tf, nl, gtex, None)
    big_size = abi.TEX_MAX_SIZE + 1
    bad = [dict(ctxh=None), dict(tex=None), dict(mip=None), dict(tw=0), dict(th=0), dict(tw=big_size), dict(th=big_size), dict(n_ch=0),
           dict(n_ch=abi.ATTR_MAX_CH + 1), dict(tf=0), dict(tf=65537), dict(nl=0), dict(nl=NL + 1), dict(tw=5, th=7, nl=2), dict(mb=mip_bytes - 4),
           dict(mb=0), dict(tex=x + 2), dict(mip=o + 2), dict(mip=x), dict(mip=x + TEX_BYTES - 4), dict(tex=o + 16)]
    for kw in bad:
        refused(ctx, build(**kw), "srz_texture_mip_build", kw)
    fold_bytes = srz.mip_bytes(TW, TH, C, 1, NL)
    bad = [dict(ctxh=None), dict(gmip=None), dict(gtex=None), dict(tw=0), dict(th=big_size), dict(n_ch=0), dict(n_ch=abi.ATTR_MAX_CH + 1), dict(tf=0),
           dict(nl=0), dict(nl=NL + 1), dict(mb=fold_bytes - 4), dict(gmip=x + 2), dict(gtex=o + 2), dict(gtex=x), dict(gtex=x + fold_bytes - 4),
           dict(gmip=o + 16)]
    for kw in bad:
        refused(ctx, fold(mb=kw.pop("mb", fold_bytes), **kw), "srz_texture_mip_fold", kw)
    torch.cuda.synchronize()
    assert (big == SENT).all() and (tex == 1).all()
    # the valid calls; one level launches nothing and needs no pyramid
    assert build(nl=1, mip=None, mb=0) == 0 and fold(nl=1, gmip=None, mb=0) == 0
    torch.cuda.synchronize()
    assert (big == SENT).all()
    assert build() == 0 and build(nl=2) == 0 and build(tf=1) == 0
    torch.cuda.synchronize()
    assert (big[:mip_bytes // 4].view(torch.float32) == 1).all() and (big[mip_bytes // 4:] == SENT).all()  # the mean of ones, and not a word more
    assert fold(mb=fold_bytes) == 0
    torch.cuda.synchronize()


def test_deriv_refusals(ctx):
    L = srz.lib()
    t = soup(1, 60, W, H, np.float32([1, 2, 3, 4]))
    fs = ctx.frameset([frame(t, W, H), frame(t[:50], W, H)])
    vis = visibility(fs)
    vis_before = vis.clone()
    attr = torch.ones((2, 60, 3, C), dtype=torch.float32, device="cuda")
    big = filled((2 * 2 * C * H * W + 64,))
    nb = fs.interpolate_bytes(2 * C)
    v, a, o = vis.data_ptr(), attr.data_ptr(), big.data_ptr()

    def f(vis=v, attr=a, n_ch=C, af=2, at=60, out=o, ob=nb, flags=F, ctxh=ctx.h, fsh=fs.h):
        return L.srz_frameset_interpolate_deriv(ctxh, fsh, vis, attr, n_ch, af, at, out, ob, flags, None)
    bad = [dict(ctxh=None), dict(fsh=None), dict(vis=None), dict(attr=None), dict(out=None), dict(n_ch=0), dict(n_ch=abi.ATTR_MAX_CH // 2 + 1),
           dict(n_ch=abi.ATTR_MAX_CH), dict(af=0), dict(af=3), dict(at=59), dict(ob=nb - 4), dict(ob=0), dict(vis=v + 4), dict(out=o + 4),
           dict(attr=a + 2), dict(out=v), dict(out=a), dict(attr=o + 16)]
    for flag in (abi.UNIFIED, abi.ORDERED_RASTER, 16, F | abi.UNIFIED):
        bad.append(dict(flags=flag))
    for kw in bad:
        refused(ctx, f(**kw), "srz_frameset_interpolate_deriv", kw)
    torch.cuda.synchronize()
    assert (big == SENT).all() and (attr == 1).all() and torch.equal(vis, vis_before)
    assert f() == 0 and f(af=1) == 0 and f(n_ch=1) == 0 and f(flags=0) == 0
    torch.cuda.synchronize()
    assert (big != SENT).any()
    fs.close()


def test_texture_mip_refusals_leave_every_buffer_untouched(ctx):
    L = srz.lib()
    t = soup(1, 60, W, H, np.float32([1, 2, 3, 4]))
    fs = ctx.frameset([frame(t, W, H), frame(t[:50], W, H)])
    vis = visibility(fs)
    vis_before = vis.clone()
    uv = torch.full(fs.interpolate_shape(2), 0.25, dtype=torch.float32, device="cuda")
    uvd = torch.full(fs.interpolate_shape(4), 0.125, dtype=torch.float32, device="cuda")
    tex = torch.ones((2, TH, TW, C), dtype=torch.float32, device="cuda")
    mip_bytes = srz.mip_bytes(TW, TH, C, 2, NL)
    mip = torch.ones((mip_bytes // 4,), dtype=torch.float32, device="cuda")
    gout = torch.ones(fs.interpolate_shape(C), dtype=torch.float32, device="cuda")
    big = filled((2 * 8 * H * W + 64 + (TEX_BYTES + mip_bytes) // 4 + 64,))  # the outputs are carved from this
    nb, h = fs.interpolate_bytes(C), ctx.h
    v, u, d, x, m, g, o = vis.data_ptr(), uv.data_ptr(), uvd.data_ptr(), tex.data_ptr(), mip.data_ptr(), gout.data_ptr(), big.data_ptr()
    o2 = o + UV_BYTES + 64           # gtex behind a guv-sized first output
    o3 = o2 + TEX_BYTES + 64         # gmip behind gtex

    def f(vis=v, uv=u, uvd=d, tex=x, tw=TW, th=TH, n_ch=C, tf=2, mode=abi.TEX_CLAMP, mip=m, nl=NL, out=o, ob=nb, flags=F, ctxh=h, fsh=fs.h):
        return L.srz_frameset_texture_mip(ctxh, fsh, vis, uv, uvd, tex, tw, th, n_ch, tf, mode, mip, nl, out, ob, flags, None)

    def b(vis=v, uv=u, uvd=d, gout=g, tex=x, mip=m, tw=TW, th=TH, n_ch=C, tf=2, mode=abi.TEX_WRAP, nl=NL, gtex=o2, gmip=o3, guv=o, flags=F, ctxh=h,
          fsh=fs.h):
        return L.srz_frameset_texture_mip_grad(ctxh, fsh, vis, uv, uvd, gout, tex, mip, tw, th, n_ch, tf, mode, nl, gtex, gmip, guv, flags, None)
    big_size = abi.TEX_MAX_SIZE + 1
    bad_f = [dict(ctxh=None), dict(fsh=None), dict(vis=None), dict(uv=None), dict(tex=None), dict(out=None), dict(uvd=None), dict(mip=None),  # null arguments
             dict(tw=0), dict(th=0), dict(tw=big_size), dict(th=big_size), dict(n_ch=0), dict(n_ch=abi.ATTR_MAX_CH + 1),      # sizes, n_ch
             dict(tf=0), dict(tf=3), dict(mode=2), dict(mode=0xffffffff), dict(nl=0), dict(nl=NL + 1), dict(nl=abi.TEX_MAX_LEVELS + 1),
             dict(tw=5, th=7, nl=2),                                                                                            # levels that do not exist
             dict(ob=nb - 4), dict(ob=0),                                                                                       # a short out_bytes
             dict(vis=v + 4), dict(uv=u + 8), dict(uvd=d + 4), dict(out=o + 4), dict(tex=x + 2), dict(mip=m + 2),              # misaligned pointers
             dict(out=v), dict(out=v + PLANE), dict(out=u), dict(out=u + UV_BYTES - 16), dict(out=d), dict(out=d + UVD_BYTES - 16), dict(out=x),
             dict(out=m), dict(tex=o + 16), dict(mip=o + 16), dict(uvd=o + 16)]                                                 # overlaps
    bad_b = [dict(ctxh=None), dict(fsh=None), dict(vis=None), dict(uv=None), dict(gout=None), dict(tex=None), dict(mip=None), dict(uvd=None),
             dict(gtex=None, gmip=None, guv=None), dict(gtex=None), dict(gmip=None),                                            # one of the pair alone
             dict(tw=0), dict(th=0), dict(tw=big_size), dict(th=big_size), dict(n_ch=0), dict(n_ch=abi.ATTR_MAX_CH + 1),
             dict(tf=0), dict(tf=3), dict(mode=2), dict(mode=0xffffffff), dict(nl=0), dict(nl=NL + 1), dict(tw=5, th=7, nl=2),
             dict(vis=v + 4), dict(uv=u + 8), dict(uvd=d + 4), dict(gout=g + 4), dict(guv=o + 4), dict(gtex=o2 + 2), dict(gmip=o3 + 2), dict(tex=x + 2),
             dict(mip=m + 2),
             dict(guv=v), dict(gtex=v + 32), dict(gmip=v + 64), dict(guv=u), dict(gtex=u + 32), dict(gmip=u + 64), dict(guv=d), dict(gtex=d + 32),
             dict(gmip=d + UVD_BYTES - 4), dict(guv=g), dict(gtex=g + 32), dict(gmip=g + 64), dict(gtex=x), dict(guv=x), dict(gmip=x),
             dict(gtex=m), dict(guv=m), dict(gmip=m), dict(gmip=m + mip_bytes - 4),
             dict(gtex=o + 32), dict(gtex=o + UV_BYTES - 4), dict(gmip=o + 32), dict(gmip=o2 + 32), dict(gmip=o2 + TEX_BYTES - 4)]  # ... and the other outputs
    for flag in (abi.UNIFIED, abi.ORDERED_RASTER, abi.NO_Z_READBACK, 16, F | abi.UNIFIED):
        bad_f.append(dict(flags=flag)), bad_b.append(dict(flags=flag))
    for kw in bad_f:
        refused(ctx, f(**kw), "srz_frameset_texture_mip", kw)
    for kw in bad_b:
        refused(ctx, b(**kw), "srz_frameset_texture_mip_grad", kw)
    torch.cuda.synchronize()
    assert (big == SENT).all() and (tex == 1).all() and (mip == 1).all() and (gout == 1).all() and (uv == 0.25).all() and (uvd == 0.125).all()
    assert torch.equal(vis, vis_before)
    # the valid calls, and the arguments that may be null
    assert f() == 0 and f(tf=1) == 0 and f(mode=abi.TEX_WRAP) == 0 and f(nl=2) == 0 and f(nl=1, uvd=None, mip=None) == 0 and f(nl=1) == 0
    assert f(tw=1, th=1, nl=1) == 0
    assert b() == 0 and b(tex=None, mip=None, guv=None) == 0 and b(gtex=None, gmip=None) == 0 and b(tf=1) == 0 and b(mode=abi.TEX_CLAMP) == 0
    assert b(nl=1, uvd=None, mip=None, gmip=None) == 0 and b(nl=1, gtex=None, gmip=None) == 0 and b(nl=2) == 0
    torch.cuda.synchronize()
    assert (big != SENT).any()
    fs.close()
