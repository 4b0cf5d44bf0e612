"""The visibility buffer of FrameSet.render_visibility taken apart in torch (layout: include/srz.h, srz_frameset_render_visibility).

    z        float32  the owner's depth (+inf where nobody owns the pixel in a fused-clear frame)
    tri      int64    the owner's index in the frame's own triangle stream, -1 = nobody
    s_class  bool     the pixel lies in the scalar-tail ("S") columns of its owner's bounding box
    alpha, beta, gamma  float32  the barycentrics exactly as the shaders use them; gamma = 1 - (alpha + beta) for V pixels,
                      (1 - alpha) - beta for S pixels (float32 ops, one rounding each: the shaders' bits); 0 where nobody owns the pixel

Any per-vertex attribute a of the owner interpolates as alpha * a0 + beta * a1 + gamma * a2.
"""
import contextlib
import math
from collections import namedtuple

import torch

from . import abi

Visibility = namedtuple("Visibility", "z tri s_class alpha beta gamma")

S_CLASS_BIT = 0x80000000


def decode(out):
    """out: a render_visibility buffer as a torch tensor [..., 4, rows, W] of any 4-byte dtype (planes on dim -3)."""
    if out.element_size() != 4 or out.dim() < 3 or out.shape[-3] != 4:
        raise ValueError(f"decode: expected a [..., 4, rows, W] tensor of 4-byte words, got {tuple(out.shape)} {out.dtype}")
    f = out.view(torch.float32) if out.dtype != torch.float32 else out
    words = out.view(torch.int32)[..., 1, :, :].to(torch.int64) & 0xffffffff
    z, alpha, beta = f[..., 0, :, :], f[..., 2, :, :], f[..., 3, :, :]
    owned = words != 0
    s_class = (words & S_CLASS_BIT) != 0
    tri = torch.where(owned, (words & 0x7fffffff) - 1, torch.full_like(words, -1))
    one = torch.ones((), dtype=torch.float32, device=f.device)
    gamma = torch.where(s_class, (one - alpha) - beta, one - (alpha + beta))
    gamma = torch.where(owned, gamma, torch.zeros_like(gamma))
    return Visibility(z, tri, s_class, alpha, beta, gamma)


# ------------------------------------------------------------------------------------------------ the argument checks, each once
# Every tensor whose address goes to the library is checked by one of these, on the host, before the call.  Their texts are pinned
# word for word by tests/visrefusals.py, so a caller passes its own name and the few words its refusal has always had.
def _ptr(t):
    return None if t is None else t.data_ptr()


def _got(t, form):
    """the tail of a refusal: "" says nothing, "plain" the shape and the dtype, "pair" the two as a tuple, "shape" the shape alone"""
    if not form:
        return ""
    if t is None:
        return ", got None"
    return ", got " + {"plain": f"{tuple(t.shape)} {t.dtype}", "pair": f"{(tuple(t.shape), t.dtype)}", "shape": f"{tuple(t.shape)}"}[form]


def _on_device(t, who):
    if not t.is_cuda:
        raise ValueError(f"{who} must be on the device, got {t.device}")
    return t


def _vis_arg(fs, t, name):
    """a visibility buffer of the set: a contiguous CUDA float32 tensor of fs.out_shape, as it is (no copy)"""
    if t is None or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(fs.out_shape):
        raise ValueError(f"{name}: expected a contiguous CUDA float32 tensor {tuple(fs.out_shape)}" + _got(t, "plain"))
    return t


def _vis_ptr(fs, vis, fn):
    """the address of `vis` for the library: there is no way to it past the check"""
    return _vis_arg(fs, vis, f"{fn}: vis").data_ptr()


def _plane(fs, t, n_planes, who, must="a CUDA float32 tensor {shape}", got="plain", ok=True):
    """a plane tensor of the set: a float32 tensor of fs.interpolate_shape(n_planes) → it, contiguous.  who: "<function>: <argument>";
    must: the refusal's words — one that names CUDA refuses a host tensor in them, the others leave that to _on_device —; ok: a
    further condition of the caller's, refused in the same words"""
    shape = tuple(fs.interpolate_shape(n_planes))
    if t is None or t.dtype != torch.float32 or ("CUDA" in must and not t.is_cuda) or tuple(t.shape) != shape or not ok:
        raise ValueError(f"{who} must be {must.format(shape=shape)}" + _got(t, got))
    return t.contiguous()


def _gout(fs, gout, n_planes, fn):
    """the incoming gradient of a *_grad function: float32 of the set's shape, then on the device"""
    return _on_device(_plane(fs, gout, n_planes, f"{fn}: gout", "float32 {shape}"), f"{fn}: gout")


def _pos_handle(fs, pos, fn):
    """the graph handle on the triangles' screen positions, float32 [n_frames, T, 3, 3] of any device: its values are never read"""
    if pos is None or pos.dtype != torch.float32 or pos.dim() != 4 or pos.shape[0] != fs.n_frames or tuple(pos.shape[2:]) != (3, 3):
        raise ValueError(f"{fn}: pos must be float32 [n_frames, T, 3, 3]" + _got(pos, "plain"))
    return pos.shape


def _lead_frames(fs, t, dims, who, must, ok=lambda t: True, cuda=True):
    """the "[tail] or [n_frames, tail]" rule: `t` has dims[0] dimensions (one array for every frame) or more (one per frame of the
    set) → its frame count.  must: the refusal's words; ok: the caller's own conditions on the shape, refused in the same words"""
    if t is None or t.dtype != torch.float32 or (cuda and not t.is_cuda) or t.dim() not in dims or not ok(t):
        raise ValueError(f"{who} must be {must}" + _got(t, "plain"))
    if t.dim() > dims[0] and t.shape[0] != fs.n_frames:
        raise ValueError(f"{who} has {t.shape[0]} frames, the set {fs.n_frames}")
    return t.shape[0] if t.dim() > dims[0] else 1


def _backward(ctx, k, grad, optional=None):
    """the backward of a pass whose first k inputs are the differentiable ones: one grad(*need) call asking only for what is needed
    (none when nothing is), None for every other input.  optional: (index, given) of an input that may have been None"""
    need = list(ctx.needs_input_grad[:k])
    if optional is not None:
        need[optional[0]] = need[optional[0]] and optional[1]
    grads = grad(*need) if any(need) else (None,) * k
    return (*grads, *[None] * (len(ctx.needs_input_grad) - k))


def _reduced(par, work_bytes):
    """(the gradient of a parameter block, the scratch its fixed-tree reduction takes)"""
    return torch.empty_like(par), torch.empty(max(work_bytes // 4, 1), dtype=torch.float32, device=par.device)


def first_prev(fs):
    """the buffer that lies in front of every fragment of frames of finite depths: (z = -inf, id = 1, 0, 0) at every pixel.  peel()
    of it is layer 1, bit for bit FrameSet.render_visibility's buffer."""
    t = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    t[:, 0] = float("-inf")
    t.view(torch.int32)[:, 1] = 1
    return t


def peel(fs, prev, out=None, flags=abi.FUSED_CLEAR, stream=None):
    """depth peeling (FrameSet.peel_visibility; the rule: include/srz.h): the layer behind the visibility buffer `prev` of this set
    ([n_frames, 4, local_rows, W] float32: a render_visibility buffer, or a layer this call returned) -> that layer as a tensor in the
    same layout (`out`, or a new one), every word of it written.  Asynchronous on `stream` (default: torch's current stream)."""
    _vis_arg(fs, prev, "peel: prev")
    out = torch.empty(fs.out_shape, dtype=torch.float32, device=prev.device) if out is None else _vis_arg(fs, out, "peel: out")
    fs.peel_visibility(prev.data_ptr(), out.data_ptr(), fs.out_bytes, flags, _stream_ptr(stream))
    return out


def layers(fs, n, flags=abi.FUSED_CLEAR, stream=None):
    """the first n depth layers of the set, nearest first: layer 1 by render_visibility, the others by peel() — a list of n buffers
    [n_frames, 4, local_rows, W], each of which every pass over a visibility buffer takes.  A pixel with fewer than k fragments is
    nobody's from layer k on.  No host synchronisation."""
    if n < 1:
        raise ValueError(f"layers: n = {n}, expected at least 1")
    first = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render_visibility(first.data_ptr(), fs.out_bytes, flags | abi.FUSED_CLEAR, _stream_ptr(stream))
    out = [first]
    while len(out) < n:
        out.append(peel(fs, out[-1], flags=flags, stream=stream))
    return out


def composite(colors, alphas):
    """front-to-back "over" of depth layers, nearest first: colors[k] is [n, C, rows, W], alphas[k] [n, 1 or C, rows, W] (0 where
    nobody owns the pixel: decode(layer).tri >= 0 times the surface's opacity) -> sum_k colors[k] * alphas[k] * prod_{j<k} (1 -
    alphas[j]).  Plain torch ops: autograd goes through it, into the colours and the opacities of every layer.
    composite_layers does the same in one pass on the device (one alpha per layer, coverage from the layers' own ids)."""
    colors, alphas = list(colors), list(alphas)
    if not colors or len(colors) != len(alphas):
        raise ValueError(f"composite: {len(colors)} colour layers, {len(alphas)} alpha layers")
    acc, through = None, None
    for c, a in zip(colors, alphas):
        term = c * a if through is None else c * (a * through)
        acc = term if acc is None else acc + term
        through = (1 - a) if through is None else through * (1 - a)
    return acc


def _composite_args(fs, layers, colors, alphas, background):
    """→ (layer tuples for FrameSet.composite, n_ch, colours, alpha planes or None, opacities, background or None), checked, contiguous"""
    layers, colors, alphas = list(layers), list(colors), list(alphas)
    n = len(layers)
    if not 1 <= n <= abi.COMPOSITE_MAX or len(colors) != n or len(alphas) != n:
        raise ValueError(f"composite_layers: {n} layers (1 .. {abi.COMPOSITE_MAX}), {len(colors)} colour buffers, {len(alphas)} alphas")
    n_ch = colors[0].shape[1] if isinstance(colors[0], torch.Tensor) and colors[0].dim() == 4 else 0
    cols, planes, opac, tup = [], [], [], []
    for k in range(n):
        _vis_arg(fs, layers[k], f"composite_layers: layers[{k}]")
        c, a = _plane(fs, colors[k], n_ch, f"composite_layers: colors[{k}]", ok=1 <= n_ch <= abi.ATTR_MAX_CH), alphas[k]
        if isinstance(a, torch.Tensor) and a.dim() != 0:
            planes.append(_plane(fs, a, 1, f"composite_layers: alphas[{k}]", "a CUDA float32 tensor {shape} or a scalar")), opac.append(0.0)
        else:
            planes.append(None), opac.append(float(a))
        cols.append(c)
        tup.append((layers[k].data_ptr(), c.data_ptr(), _ptr(planes[k]), opac[k]))
    if background is not None:
        background = _plane(fs, background, n_ch, "composite_layers: background", got="shape")
    return tup, n_ch, cols, planes, opac, background


def composite_grad(fs, layers, colors, alphas, gout, background=None, through=False, want_gcolor=True, want_galpha=True, want_gbg=None,
                   stream=None):
    """the backward of composite_layers(fs, layers, colors, alphas, background, through) by one FrameSet.composite_grad call: gout
    [n_frames, C (+ 1), rows, W] → (gcolors, galphas, gbg): two lists with one entry per layer and the background's gradient, an
    entry None where not wanted.  want_gcolor and want_galpha are a bool or one bool per layer; want_gbg defaults to "there is a
    background".  galphas[k] is a plane [n_frames, 1, rows, W] also where alphas[k] is a scalar (its gradient is the plane's sum).  +0
    where the layer does not cover the pixel; per pixel, deterministic.  stream: a raw stream handle, None = torch's current stream."""
    tup, n_ch, cols, planes, opac, bg = _composite_args(fs, layers, colors, alphas, background)
    n = len(tup)
    want_gcolor = [bool(want_gcolor)] * n if isinstance(want_gcolor, bool) else [bool(w) for w in want_gcolor]
    want_galpha = [bool(want_galpha)] * n if isinstance(want_galpha, bool) else [bool(w) for w in want_galpha]
    want_gbg = bg is not None if want_gbg is None else bool(want_gbg)
    if len(want_gcolor) != n or len(want_galpha) != n:
        raise ValueError(f"composite_grad: want_gcolor / want_galpha must be a bool or {n} bools")
    if want_gbg and bg is None:
        raise ValueError("composite_grad: gbg without a background")
    if not (any(want_gcolor) or any(want_galpha) or want_gbg):
        raise ValueError("composite_grad: no gradient is asked for")
    gout = _plane(fs, gout, n_ch + (1 if through else 0), "composite_grad: gout")
    dev = gout.device
    gcol = [torch.empty(fs.interpolate_shape(n_ch), dtype=torch.float32, device=dev) if w else None for w in want_gcolor]
    galpha = [torch.empty(fs.interpolate_shape(1), dtype=torch.float32, device=dev) if w else None for w in want_galpha]
    gbg = torch.empty(fs.interpolate_shape(n_ch), dtype=torch.float32, device=dev) if want_gbg else None
    fs.composite_grad(tup, n_ch, _ptr(bg), bool(through), gout.data_ptr(), [_ptr(t) for t in gcol], [_ptr(t) for t in galpha], _ptr(gbg),
                      abi.FUSED_CLEAR, _stream_ptr(stream))
    return gcol, galpha, gbg


class _CompositeLayers(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fs, layers, through, stream, n, has_bg, *tensors):
        colors, alphas, bg = tensors[:n], tensors[n:2 * n], tensors[2 * n] if has_bg else None
        tup, n_ch, cols, planes, opac, bg = _composite_args(fs, layers, colors, alphas, bg)
        planes_out = n_ch + (1 if through else 0)
        out = torch.empty(fs.interpolate_shape(planes_out), dtype=torch.float32, device=cols[0].device)
        fs.composite(tup, n_ch, _ptr(bg), bool(through), out.data_ptr(), out.numel() * 4, abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.layers, ctx.through, ctx.stream, ctx.n, ctx.has_bg = fs, list(layers), through, stream, n, has_bg
        ctx.scalar = [p is None for p in planes]
        ctx.alpha_meta = [(a.dtype, a.device) if isinstance(a, torch.Tensor) else None for a in alphas]
        ctx.save_for_backward(*cols, *[torch.as_tensor(o) if p is None else p for p, o in zip(planes, opac)], *([bg] if has_bg else []))
        return out

    @staticmethod
    def backward(ctx, gout):
        n, saved = ctx.n, ctx.saved_tensors
        cols, alphas, bg = saved[:n], saved[n:2 * n], saved[2 * n] if ctx.has_bg else None
        alphas = [float(a) if s else a for a, s in zip(alphas, ctx.scalar)]
        need = ctx.needs_input_grad[6:]
        need_c, need_a, need_bg = list(need[:n]), list(need[n:2 * n]), bool(ctx.has_bg and need[2 * n])
        grads = [None] * (2 * n + (1 if ctx.has_bg else 0))
        if any(need_c) or any(need_a) or need_bg:  # one call, asking only for what is needed
            gcol, galpha, gbg = composite_grad(ctx.fs, ctx.layers, cols, alphas, gout, bg, ctx.through, need_c, need_a, need_bg, ctx.stream)
            for k in range(n):
                grads[k] = gcol[k]
                if galpha[k] is not None:  # (a scalar opacity: the plane's sum, in the scalar's dtype and on its device)
                    grads[n + k] = galpha[k].sum().to(dtype=ctx.alpha_meta[k][0], device=ctx.alpha_meta[k][1]) if ctx.scalar[k] else galpha[k]
            if ctx.has_bg:
                grads[2 * n] = gbg
        return (None, None, None, None, None, None, *grads)


def composite_layers(fs, layers, colors, alphas, background=None, through=False, stream=None):
    """front-to-back "over" of depth layers in ONE pass on the device (FrameSet.composite; include/srz.h states the rule): layers is
    layers(fs, n)'s list (or any 1 .. 8 visibility buffers of `fs`, nearest first), colors[k] [n_frames, C, rows, W] float32,
    alphas[k] a plane [n_frames, 1, rows, W] or a scalar (a Python float or a 0-dim tensor: the layer's opacity), background
    [n_frames, C, rows, W] or None → [n_frames, C, rows, W]: sum_k colors[k] alphas[k] T_k (+ background T_n), T the product of (1 -
    alpha) over the covering layers in front; with through=True the final T is appended as plane C.  A layer counts at a pixel only
    where its own id word names an owner — no alpha * coverage tensor is needed, and colours and alphas may hold anything (NaN) where
    it does not.  Differentiable with respect to every colour, alpha (a scalar that requires grad gets the sum of its plane) and the
    background; backward is one composite_grad call that asks only for what some input needs, and nothing but the inputs is kept for
    it.  stream: a raw stream handle, None = torch's current stream."""
    layers, colors, alphas = list(layers), list(colors), list(alphas)
    if not (len(layers) == len(colors) == len(alphas)):
        raise ValueError(f"composite_layers: {len(layers)} layers, {len(colors)} colour buffers, {len(alphas)} alphas")
    extra = [] if background is None else [background]
    return _CompositeLayers.apply(fs, layers, through, stream, len(layers), background is not None, *colors, *alphas, *extra)


def batch_of(frame, tri):
    """The batch (a Frame) or draw (a SceneFrame's draws: pass their face counts as a sequence) each triangle index of `tri` belongs
    to; -1 where tri is -1.  Empty batches own no index."""
    sizes = [len(t) for t in frame.tris] if hasattr(frame, "tris") else [int(n) for n in frame]
    tri = torch.as_tensor(tri)
    ends = torch.cumsum(torch.tensor(sizes, dtype=torch.int64, device=tri.device), 0)
    total = int(ends[-1]) if len(sizes) else 0
    if bool(((tri < -1) | (tri >= total)).any()):
        raise IndexError(f"batch_of: a triangle index outside the frame's {total} triangles")
    b = torch.searchsorted(ends, tri.to(torch.int64), right=True)
    return torch.where(tri < 0, torch.full_like(b, -1), b)


_GB_GROUPS = ((abi.GB_NORMAL, ("nx", "ny", "nz")), (abi.GB_UV, ("u", "v")), (abi.GB_BATCH, ("batch",)),
              (abi.GB_ALBEDO, ("albedo0", "albedo1", "albedo2")))


def gbuffer_planes(what):
    """the plane names of a G-buffer of the groups in `what` (abi.GB_*), in buffer order (include/srz.h, srz_frameset_gbuffer)"""
    if what == 0 or what & ~abi.GB_ALL:
        raise ValueError(f"gbuffer_planes: what = {what:#x} names no group or an unknown one")
    return tuple(name for bit, names in _GB_GROUPS if what & bit for name in names)


def gbuffer_decode(buf, what):
    """buf: a FrameSet.gbuffer buffer as a torch tensor [..., planes, rows, W] of any 4-byte dtype → a dict of VIEWS (no copy) with the
    groups of `what`: "normal" [..., 3, rows, W] and "uv" [..., 2, rows, W] float32, "batch" [..., rows, W] int32 (the owner's batch
    index in its frame, -1 = nobody: the stored word is index + 1, so this one entry is computed) and "albedo" [..., 3, rows, W]
    float32 in the order of the colour planes."""
    n = len(gbuffer_planes(what))
    if buf.element_size() != 4 or buf.dim() < 3 or buf.shape[-3] != n:
        raise ValueError(f"gbuffer_decode: expected a [..., {n}, rows, W] tensor of 4-byte words, got {tuple(buf.shape)} {buf.dtype}")
    f = buf.view(torch.float32) if buf.dtype != torch.float32 else buf
    out, at = {}, 0
    for bit, key, k in ((abi.GB_NORMAL, "normal", 3), (abi.GB_UV, "uv", 2), (abi.GB_BATCH, "batch", 1), (abi.GB_ALBEDO, "albedo", 3)):
        if not what & bit:
            continue
        if key == "batch":
            out[key] = buf.view(torch.int32)[..., at, :, :] - 1
        else:
            out[key] = f[..., at:at + k, :, :]
        at += k
    return out


_MV_GROUPS = ((abi.MV_FLOW, ("dx", "dy")), (abi.MV_DEPTH, ("depth",)), (abi.MV_TARGET, ("target_id", "target_z")))


def motion_planes(what):
    """the plane names of a motion buffer of the groups in `what` (abi.MV_*), in buffer order (include/srz.h, srz_frameset_motion)"""
    if what == 0 or what & ~abi.MV_ALL:
        raise ValueError(f"motion_planes: what = {what:#x} names no group or an unknown one")
    return tuple(name for bit, names in _MV_GROUPS if what & bit for name in names)


def motion_decode(buf, what):
    """buf: a FrameSet.motion buffer as a torch tensor [..., planes, rows, W] of any 4-byte dtype → a dict with the groups of `what`:
    "flow" [..., 2, rows, W] (dx, dy), "depth" [..., rows, W] and "target_z" [..., rows, W] float32 — VIEWS, no copy — and, computed
    from the target's id word, "target_index" [..., rows, W] int64 (the index in the target frame's triangle stream of the owner of
    the nearest sample there; -1 = nobody there, the sample outside the frame, or no owner here) and "target_s_class" bool."""
    n = len(motion_planes(what))
    if buf.element_size() != 4 or buf.dim() < 3 or buf.shape[-3] != n:
        raise ValueError(f"motion_decode: expected a [..., {n}, rows, W] tensor of 4-byte words, got {tuple(buf.shape)} {buf.dtype}")
    f = buf.view(torch.float32) if buf.dtype != torch.float32 else buf
    out, at = {}, 0
    if what & abi.MV_FLOW:
        out["flow"] = f[..., at:at + 2, :, :]
        at += 2
    if what & abi.MV_DEPTH:
        out["depth"] = f[..., at, :, :]
        at += 1
    if what & abi.MV_TARGET:
        words = buf.view(torch.int32)[..., at, :, :].to(torch.int64) & 0xffffffff
        out["target_index"] = (words & 0x7fffffff) - 1
        out["target_s_class"] = (words & S_CLASS_BIT) != 0
        out["target_z"] = f[..., at + 1, :, :]
    return out


def _attr_dims(fs, attr):
    attr_frames = _lead_frames(fs, attr, (3, 4), "interpolate: attr", "a CUDA float32 tensor [T, 3, C] or [n_frames, T, 3, C]",
                               lambda t: t.shape[-2] == 3)
    return attr_frames, attr.shape[-3], attr.shape[-1]


def _stream_ptr(stream):
    return torch.cuda.current_stream().cuda_stream if stream is None else stream


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, fs, vis, stream):
        attr_frames, tris, n_ch = _attr_dims(fs, attr)
        attr = attr.contiguous()
        out = torch.empty(fs.interpolate_shape(n_ch), dtype=torch.float32, device=attr.device)
        fs.interpolate(_vis_ptr(fs, vis, "interpolate"), attr.data_ptr(), n_ch, attr_frames, tris, out.data_ptr(), fs.interpolate_bytes(n_ch),
                       abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.stream, ctx.attr_shape = fs, vis, stream, attr.shape
        return out

    @staticmethod
    def backward(ctx, gout):
        fs, shape = ctx.fs, ctx.attr_shape
        gout = gout.contiguous()
        gattr = torch.zeros(shape, dtype=torch.float32, device=gout.device)
        attr_frames = shape[0] if len(shape) == 4 else 1
        fs.interpolate_grad(ctx.vis.data_ptr(), gout.data_ptr(), None, shape[-1], attr_frames, shape[-3], gattr.data_ptr(), None,
                            abi.FUSED_CLEAR, _stream_ptr(ctx.stream))
        return gattr, None, None, None


def interpolate(fs, vis, attr, stream=None):
    """per-vertex attributes of the caller's own under a visibility buffer `vis` of FrameSet `fs` (a torch tensor of fs.out_shape):
    attr is a CUDA float32 tensor [T, 3, C] (one array for every frame: poses of one mesh) or [n_frames, T, 3, C], T at least every
    frame's triangle count, C <= abi.ATTR_MAX_CH, triangle and corner order those of the frame's stream → [n_frames, C, rows, W]
    float32, zeros where nobody owns the pixel; each channel interpolated exactly as the owner's class interpolates uv
    (FrameSet.interpolate).  Differentiable with respect to attr (FrameSet.interpolate_grad into a zeroed tensor: float atomics, so
    attr.grad is not bit-reproducible between runs); vis is not differentiated — interpolate_bary_grad gives the planes to chain
    into alpha and beta.  stream: a raw stream handle, None = torch's current stream."""
    return _Interpolate.apply(attr, fs, vis, stream)


def interpolate_bary_grad(fs, vis, attr, gout, stream=None):
    """the gradient of interpolate(fs, vis, attr) with respect to alpha and beta, given gout [n_frames, C, rows, W] →
    [n_frames, 2, rows, W] float32 (dalpha, dbeta; zeros where nobody owns the pixel).  gamma's share is folded in: the planes are the
    sums over the channels of gout * (a - c) and gout * (b - c).  Deterministic."""
    attr_frames, tris, n_ch = _attr_dims(fs, attr)
    attr, gout = attr.contiguous(), _gout(fs, gout, n_ch, "interpolate_bary_grad")
    out = torch.empty(fs.interpolate_shape(2), dtype=torch.float32, device=attr.device)
    fs.interpolate_grad(_vis_ptr(fs, vis, "interpolate_bary_grad"), gout.data_ptr(), attr.data_ptr(), n_ch, attr_frames, tris, None, out.data_ptr(),
                        abi.FUSED_CLEAR, _stream_ptr(stream))
    return out


def _pos_tris(fs, pos_tris):
    if pos_tris is not None:
        return int(pos_tris)
    if not all(hasattr(f, "n_tris") for f in fs.frames):
        raise ValueError("position_grad: pos_tris must be given for a sceneset (at least every frame's triangle count)")
    return max(f.n_tris for f in fs.frames)


def position_grad(fs, vis, gbary=None, gz=None, pos_tris=None, want_pix=False, stream=None):
    """the gradient of a loss with respect to the SCREEN POSITIONS of FrameSet `fs`'s triangles, through a visibility buffer `vis` of
    it, owners held fixed (FrameSet.position_grad, include/srz.h): gbary [n_frames, 2, rows, W] is the loss gradient with respect to
    each pixel's alpha and beta (interpolate_bary_grad's planes), gz [n_frames, 1, rows, W] the one with respect to depth plane 0; at
    least one is given.  → gpos [n_frames, T, 3, 3] float32 (triangle, corner, (x, y, z)), T = pos_tris (default: the largest
    triangle count of the set's frames; a sceneset must name it); with want_pix also gpix [n_frames, 2, rows, W], the gradient with
    respect to each pixel's sample point (zeros where nobody owns the pixel).  gpos is a sum of float atomics: not bit-reproducible
    between runs; gpix is deterministic.  stream: a raw stream handle, None = torch's current stream."""
    if gbary is None and gz is None:
        raise ValueError("position_grad: neither gbary nor gz is given")
    gbary = None if gbary is None else _plane(fs, gbary, 2, "position_grad: gbary")
    gz = None if gz is None else _plane(fs, gz, 1, "position_grad: gz")
    T = _pos_tris(fs, pos_tris)
    dev = _vis_arg(fs, vis, "position_grad: vis").device
    gpos = torch.zeros((fs.n_frames, T, 3, 3), dtype=torch.float32, device=dev)
    gpix = torch.empty(fs.interpolate_shape(2), dtype=torch.float32, device=dev) if want_pix else None
    fs.position_grad(vis.data_ptr(), _ptr(gbary), _ptr(gz), T, gpos.data_ptr(), _ptr(gpix), abi.FUSED_CLEAR, _stream_ptr(stream))
    return (gpos, gpix) if want_pix else gpos


class _InterpolateGeo(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, pos, fs, vis, stream):
        attr_frames, tris, n_ch = _attr_dims(fs, attr)
        attr, ctx.pos_shape = attr.contiguous(), _pos_handle(fs, pos, "interpolate_geo")
        out = torch.empty(fs.interpolate_shape(n_ch), dtype=torch.float32, device=attr.device)
        fs.interpolate(_vis_ptr(fs, vis, "interpolate_geo"), attr.data_ptr(), n_ch, attr_frames, tris, out.data_ptr(), fs.interpolate_bytes(n_ch),
                       abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.stream = fs, vis, stream
        ctx.save_for_backward(attr)
        return out

    @staticmethod
    def backward(ctx, gout):
        fs, vis, (attr,) = ctx.fs, ctx.vis, ctx.saved_tensors
        need_attr, need_pos = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gout = gout.contiguous()
        attr_frames, tris, n_ch = _attr_dims(fs, attr)
        sp = _stream_ptr(ctx.stream)
        # one interpolate_grad call for both of its outputs, then one position_grad call
        gattr = torch.zeros_like(attr) if need_attr else None
        gbary = torch.empty(fs.interpolate_shape(2), dtype=torch.float32, device=gout.device) if need_pos else None
        if need_attr or need_pos:
            fs.interpolate_grad(vis.data_ptr(), gout.data_ptr(), attr.data_ptr(), n_ch, attr_frames, tris, _ptr(gattr), _ptr(gbary), abi.FUSED_CLEAR, sp)
        gpos = None
        if need_pos:
            gpos = torch.zeros(ctx.pos_shape, dtype=torch.float32, device=gout.device)
            fs.position_grad(vis.data_ptr(), gbary.data_ptr(), None, ctx.pos_shape[1], gpos.data_ptr(), None, abi.FUSED_CLEAR, sp)
        return gattr, gpos, None, None, None


def interpolate_geo(fs, vis, attr, pos, stream=None):
    """interpolate(fs, vis, attr), differentiable with respect to the triangles' screen positions too: pos is a CUDA float32 tensor
    [n_frames, T, 3, 3] (triangle, corner, (x, y, z); T at least every frame's triangle count).  ITS VALUES ARE NEVER READ: the
    barycentrics are those of `vis` and the positions the set's own, and the caller warrants that pos holds the same positions (it
    is the graph's handle on them: what the caller's parameters produced and the set was made from).  Backward: attr.grad as
    interpolate's; pos.grad from one interpolate_grad call (asking for both the attribute gradient and the alpha / beta planes) and
    one position_grad call.  Owners are held fixed: this is the interior term; antialias(fs, vis, interpolate_geo(...), pos) adds the
    silhouette term.  The z column of pos.grad is zero (depth() is the function of
    z).  Both gradients are sums of float atomics: not bit-reproducible between runs."""
    return _InterpolateGeo.apply(attr, pos, fs, vis, stream)


class _Depth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, fs, vis, stream):
        ctx.pos_shape = _pos_handle(fs, pos, "depth")
        ctx.fs, ctx.vis, ctx.stream = fs, _vis_arg(fs, vis, "depth: vis"), stream
        return vis[:, 0:1].clone()

    @staticmethod
    def backward(ctx, gz):
        fs = ctx.fs
        gz = gz.contiguous()
        gpos = torch.zeros(ctx.pos_shape, dtype=torch.float32, device=gz.device)
        fs.position_grad(ctx.vis.data_ptr(), None, gz.data_ptr(), ctx.pos_shape[1], gpos.data_ptr(), None, abi.FUSED_CLEAR,
                         _stream_ptr(ctx.stream))
        return gpos, None, None, None


def depth(fs, vis, pos, stream=None):
    """plane 0 of the visibility buffer `vis` [n_frames, 1, rows, W] as a differentiable function of the triangles' screen positions
    pos [n_frames, T, 3, 3] (see interpolate_geo: the values of pos are never read, the caller warrants they are the set's):
    backward is one position_grad call with the incoming gradient as gz — z's own share into the z column, and x, y through the
    barycentrics.  Words of the incoming gradient at nobody's pixels (depth +inf there in a fused-clear buffer) reach nothing."""
    return _Depth.apply(pos, fs, vis, stream)


def _color_arg(fs, t, name):
    n_ch = t.shape[1] if isinstance(t, torch.Tensor) and t.dim() == 4 else 0
    t = _plane(fs, t, n_ch, f"antialias: {name}", "a CUDA float32 tensor [n_frames, C, rows, W] of the set")
    if not 1 <= n_ch <= abi.ATTR_MAX_CH:
        raise ValueError(f"antialias: {name} has {n_ch} channels, 1 .. {abi.ATTR_MAX_CH} are supported")
    return t


def antialias_grad(fs, vis, color, gout, pos_tris=None, want_gin=True, want_gpos=True, stream=None):
    """the backward of antialias(fs, vis, color) by one FrameSet.antialias_grad call: gout [n_frames, C, rows, W] → (gin, gpos), each
    None when not wanted (not both): gin has color's shape (deterministic); gpos [n_frames, T, 3, 3] float32 (triangle, corner,
    (x, y, z)), T = pos_tris (default: the largest triangle count of the set's frames; a sceneset must name it), is the SILHOUETTE
    term of the gradient with respect to the triangles' screen positions — a sum of float atomics into zeros, not bit-reproducible
    between runs; its z column is zero.  stream: a raw stream handle, None = torch's current stream."""
    if not want_gin and not want_gpos:
        raise ValueError("antialias_grad: neither gin nor gpos is asked for")
    color, gout = _color_arg(fs, color, "color"), _color_arg(fs, gout, "gout")
    if gout.shape != color.shape:
        raise ValueError(f"antialias_grad: gout {tuple(gout.shape)} is not of color's shape {tuple(color.shape)}")
    T = _pos_tris(fs, pos_tris) if want_gpos else 0
    gin = torch.empty_like(color) if want_gin else None
    gpos = torch.zeros((fs.n_frames, T, 3, 3), dtype=torch.float32, device=color.device) if want_gpos else None
    fs.antialias_grad(_vis_ptr(fs, vis, "antialias_grad"), color.data_ptr(), gout.data_ptr(), color.shape[1], _ptr(gin), T, _ptr(gpos),
                      abi.FUSED_CLEAR, _stream_ptr(stream))
    return gin, gpos


class _Antialias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, pos, fs, vis, stream):
        color = _color_arg(fs, color, "color")
        ctx.pos_shape = None if pos is None else _pos_handle(fs, pos, "antialias")
        n_ch = color.shape[1]
        out = torch.empty_like(color)
        fs.antialias(_vis_ptr(fs, vis, "antialias"), color.data_ptr(), n_ch, out.data_ptr(), fs.interpolate_bytes(n_ch), abi.FUSED_CLEAR,
                     _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.stream = fs, vis, stream
        ctx.save_for_backward(color)
        return out

    @staticmethod
    def backward(ctx, gout):
        fs, (color,) = ctx.fs, ctx.saved_tensors
        need_color, need_pos = ctx.needs_input_grad[0], ctx.pos_shape is not None and ctx.needs_input_grad[1]
        gin = gpos = None
        if need_color or need_pos:  # one call, asking only for what is needed
            gout = gout.contiguous()
            gin = torch.empty_like(color) if need_color else None
            gpos = torch.zeros(ctx.pos_shape, dtype=torch.float32, device=gout.device) if need_pos else None
            fs.antialias_grad(ctx.vis.data_ptr(), color.data_ptr(), gout.data_ptr(), color.shape[1], _ptr(gin), ctx.pos_shape[1] if need_pos else 0,
                              _ptr(gpos), abi.FUSED_CLEAR, _stream_ptr(ctx.stream))
        return gin, gpos, None, None, None


def antialias(fs, vis, color, pos=None, stream=None):
    """color [n_frames, C, rows, W] (CUDA float32: a shaded image, interpolate's planes, ...) blended across the silhouettes of the
    visibility buffer `vis` of FrameSet `fs` (FrameSet.antialias; include/srz.h states the rule) → the same shape.  The words of
    color at nobody's pixels are the background the outlines blend with.  Differentiable with respect to color (deterministic) and,
    when pos is given, to the triangles' screen positions: pos is the never-read graph handle interpolate_geo takes,
    [n_frames, T, 3, 3], and pos.grad receives the SILHOUETTE term (its z column is zero; a sum of float atomics: not
    bit-reproducible between runs).  antialias(fs, vis, interpolate_geo(fs, vis, attr, pos), pos) is the full chain: pos.grad is then
    the sum of the interior and the silhouette term — together the derivative, to first order, of the loss over frames rendered
    again while no pixel changes its owner; across an owner change the antialiased image itself jumps (DESIGN.md has both
    measured).  Backward is one antialias_grad call that asks only for the outputs some input
    needs, and no call when none does.  Needs an unsharded context.  stream: a raw stream handle, None = torch's current stream."""
    return _Antialias.apply(color, pos, fs, vis, stream)


def _tex_dims(fs, tex):
    tex_frames = _lead_frames(fs, tex, (3, 4), "texture: tex", "a CUDA float32 tensor [H, W, C] or [n_frames, H, W, C]")
    h, w, n_ch = tex.shape[-3:]
    if not (1 <= w <= abi.TEX_MAX_SIZE and 1 <= h <= abi.TEX_MAX_SIZE and 1 <= n_ch <= abi.ATTR_MAX_CH):
        raise ValueError(f"texture: tex is {w} x {h} texels of {n_ch} channels; 1 .. {abi.TEX_MAX_SIZE} and 1 .. {abi.ATTR_MAX_CH} are supported")
    return tex_frames, h, w, n_ch


def texture_grad(fs, vis, tex, uv, gout, wrap=False, want_gtex=True, want_guv=True, stream=None):
    """the backward of texture(fs, vis, tex, uv, wrap) by one FrameSet.texture_grad call: gout [n_frames, C, rows, W] → (gtex, guv),
    each None when not wanted (not both): gtex has tex's shape — a sum of float atomics into zeros, not bit-reproducible between
    runs; guv [n_frames, 2, rows, W] is deterministic, zeros where nobody owns the pixel or its uv is not finite, and is what
    interpolate's backward takes for a two-channel attribute.  stream: a raw stream handle, None = torch's current stream."""
    if not want_gtex and not want_guv:
        raise ValueError("texture_grad: neither gtex nor guv is asked for")
    uv = _plane(fs, uv, 2, "texture: uv")
    tex_frames, h, w, n_ch = _tex_dims(fs, tex)
    tex, gout = tex.contiguous(), _gout(fs, gout, n_ch, "texture_grad")
    gtex = torch.zeros_like(tex) if want_gtex else None
    guv = torch.empty_like(uv) if want_guv else None
    fs.texture_grad(_vis_ptr(fs, vis, "texture_grad"), uv.data_ptr(), gout.data_ptr(), tex.data_ptr(), w, h, n_ch, tex_frames,
                    abi.TEX_WRAP if wrap else abi.TEX_CLAMP, _ptr(gtex), _ptr(guv), abi.FUSED_CLEAR, _stream_ptr(stream))
    return gtex, guv


class _Texture(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv, fs, vis, wrap, stream):
        uv = _plane(fs, uv, 2, "texture: uv")
        tex_frames, h, w, n_ch = _tex_dims(fs, tex)
        tex = tex.contiguous()
        out = torch.empty(fs.interpolate_shape(n_ch), dtype=torch.float32, device=tex.device)
        fs.texture(_vis_ptr(fs, vis, "texture"), uv.data_ptr(), tex.data_ptr(), w, h, n_ch, tex_frames, abi.TEX_WRAP if wrap else abi.TEX_CLAMP,
                   out.data_ptr(), fs.interpolate_bytes(n_ch), abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.wrap, ctx.stream = fs, vis, wrap, stream
        ctx.save_for_backward(tex, uv)
        return out

    @staticmethod
    def backward(ctx, gout):
        tex, uv = ctx.saved_tensors
        return _backward(ctx, 2, lambda *need: texture_grad(ctx.fs, ctx.vis, tex, uv, gout, ctx.wrap, *need, ctx.stream))


def texture(fs, vis, tex, uv, wrap=False, stream=None):
    """a float texture of the caller's own sampled bilinearly under a visibility buffer `vis` of FrameSet `fs`: tex is a CUDA float32
    tensor [H, W, C] (one texture for every frame) or [n_frames, H, W, C], channels last, C <= abi.ATTR_MAX_CH, H and W <=
    abi.TEX_MAX_SIZE; uv is [n_frames, 2, rows, W] — interpolate(fs, vis, uv_attr) of a [T, 3, 2] attribute, or the uv group of a
    G-buffer → [n_frames, C, rows, W] float32, zeros where nobody owns the pixel or its uv is not finite (FrameSet.texture;
    include/srz.h states the rule).  wrap: repeat the texture instead of clamping to its border texels.  Differentiable with
    respect to tex (float atomics into a zeroed tensor: tex.grad is not bit-reproducible between runs) and to uv (deterministic), so
    texture(fs, vis, tex, interpolate(fs, vis, uv_attr)) backpropagates to tex and to uv_attr.  Backward is one texture_grad call that
    asks only for the outputs some input needs.  stream: a raw stream handle, None = torch's current stream."""
    return _Texture.apply(tex, uv, fs, vis, wrap, stream)


def _each(flag, n):
    """a bool for every one of n textures, or one bool per texture (zip below refuses another count)"""
    return [bool(flag)] * n if isinstance(flag, bool) else [bool(f) for f in flag]


def _slot_map(batch_slot, device):
    """the batch → slot map of texture_set as a uint8 tensor: a uint8 tensor as it is (it must be on the device), else a sequence of
    ints on `device` — None, and an entry that is no index at all (negative, beyond a byte), is "no slot" """
    if isinstance(batch_slot, torch.Tensor) and batch_slot.dtype == torch.uint8:
        return _on_device(batch_slot, "texture_set: batch_slot").reshape(-1).contiguous()
    seq = batch_slot.tolist() if isinstance(batch_slot, torch.Tensor) else list(batch_slot)
    return torch.tensor([int(s) if s is not None and 0 <= int(s) < abi.TEXSET_NONE else abi.TEXSET_NONE for s in seq], dtype=torch.uint8).to(device)


def _texset_args(fs, texs, wrap):
    """→ (the textures, contiguous; per texture (tex_frames, h, w); n_ch; per texture its mode).  texs[0] (None: no texture at all)
    and, for its channel count, every other texture go through _lead_frames in texture_set's name, each through _tex_dims; the
    counts (1 .. abi.TEXSET_MAX textures, 1 .. 65536 map entries) are the library's to refuse"""
    texs = list(texs)
    _lead_frames(fs, texs[0] if texs else None, (3, 4), "texture_set: texs[0]", "a CUDA float32 tensor [H, W, C] or [n_frames, H, W, C]")
    dims = [_tex_dims(fs, t) for t in texs]
    n_ch = dims[0][3]
    for k, t in enumerate(texs[1:], 1):
        _lead_frames(fs, t, (3, 4), f"texture_set: texs[{k}]", f"a CUDA float32 tensor [H, W, {n_ch}] or [n_frames, H, W, {n_ch}]: texs[0]'s channels",
                     lambda t: t.shape[-1] == n_ch)
    modes = [abi.TEX_WRAP if w else abi.TEX_CLAMP for _, w in zip(texs, _each(wrap, len(texs)), strict=True)]
    return [t.contiguous() for t in texs], [d[:3] for d in dims], n_ch, modes


def texture_set_grad(fs, vis, texs, uv, gout, batch_slot, wrap=False, want_gtex=True, want_guv=True, stream=None):
    """the backward of texture_set(fs, vis, texs, uv, batch_slot, wrap) by one FrameSet.texture_set_grad call: gout [n_frames, C,
    rows, W] → (gtexs, guv): a list with one entry per texture, of its shape — a sum of float atomics into zeros, not
    bit-reproducible between runs — and guv [n_frames, 2, rows, W], deterministic; an entry None where not wanted (the library
    refuses a call that wants nothing).  want_gtex is a bool or one bool per texture.  stream: a raw stream handle, None = torch's
    current stream."""
    uv = _plane(fs, uv, 2, "texture_set: uv")
    texs, dims, n_ch, modes = _texset_args(fs, texs, wrap)
    slot_map = _slot_map(batch_slot, uv.device)
    gout = _gout(fs, gout, n_ch, "texture_set_grad")
    gtexs = [torch.zeros_like(t) if w else None for t, w in zip(texs, _each(want_gtex, len(texs)), strict=True)]
    guv = torch.empty_like(uv) if want_guv else None
    slots = [(t.data_ptr(), _ptr(g), w, h, frames, m) for t, g, (frames, h, w), m in zip(texs, gtexs, dims, modes)]
    fs.texture_set_grad(_vis_ptr(fs, vis, "texture_set_grad"), uv.data_ptr(), gout.data_ptr(), slots, slot_map.data_ptr(), slot_map.numel(),
                        n_ch, _ptr(guv), abi.FUSED_CLEAR, _stream_ptr(stream))
    return gtexs, guv


class _TextureSet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fs, vis, slot_map, wrap, stream, uv, *texs):
        uv = _plane(fs, uv, 2, "texture_set: uv")
        texs, dims, n_ch, modes = _texset_args(fs, texs, wrap)
        out = torch.empty(fs.interpolate_shape(n_ch), dtype=torch.float32, device=texs[0].device)
        slots = [(t.data_ptr(), None, w, h, frames, m) for t, (frames, h, w), m in zip(texs, dims, modes)]
        fs.texture_set(_vis_ptr(fs, vis, "texture_set"), uv.data_ptr(), slots, slot_map.data_ptr(), slot_map.numel(), n_ch, out.data_ptr(),
                       fs.interpolate_bytes(n_ch), abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.slot_map, ctx.wrap, ctx.stream = fs, vis, slot_map, wrap, stream
        ctx.save_for_backward(uv, *texs)
        return out

    @staticmethod
    def backward(ctx, gout):
        uv, *texs = ctx.saved_tensors
        need_uv, need_tex = ctx.needs_input_grad[5], list(ctx.needs_input_grad[6:])
        gtexs, guv = [None] * len(texs), None
        if need_uv or any(need_tex):  # one call, asking only for what is needed
            gtexs, guv = texture_set_grad(ctx.fs, ctx.vis, texs, uv, gout, ctx.slot_map, ctx.wrap, need_tex, need_uv, ctx.stream)
        return (None, None, None, None, None, guv, *gtexs)


def texture_set(fs, vis, texs, uv, batch_slot, wrap=False, stream=None):
    """texture() for a scene of several materials in ONE pass: the texture of each pixel is picked by its owner's batch
    (FrameSet.texture_set; include/srz.h states the rule).  texs is a sequence of 1 .. 8 CUDA float32 tensors [H, W, C] or
    [n_frames, H, W, C], each of its own size, C common; batch_slot maps a batch of a frame (a sceneset: a draw) to an index into
    texs — a sequence of ints (None, or an int that is no index: no slot) or a uint8 CUDA tensor (abi.TEXSET_NONE: no slot), one
    map of 1 .. 65536 entries for every frame; wrap is a bool or one per texture; uv as texture() takes it → [n_frames, C, rows, W] float32: per pixel texture(fs, vis,
    texs[batch_slot[batch]], uv, wrap), zeros where nobody owns the pixel, its uv is not finite, or its batch has no slot (beyond
    the map, None, an index outside texs).  Differentiable with respect to every texture that requires grad (float atomics into a
    zeroed tensor: not bit-reproducible between runs) and to uv (deterministic); backward is one texture_set_grad call that asks only
    for the gradients some input needs.  stream: a raw stream handle, None = torch's current stream."""
    slot_map = _slot_map(batch_slot, uv.device if isinstance(uv, torch.Tensor) else "cuda")  # (everything else is checked in forward, once)
    return _TextureSet.apply(fs, vis, slot_map, wrap, stream, uv, *texs)


def cube_dirs(n, device=None):
    """the unit direction of every texel centre of an n x n cube map → [6, n, n, 3] float32 (face, row, column; faces +X -X +Y -Y +Z
    -Z, a face's point n + s su + t sv with s = (2 x + 1) / n - 1, t = (2 y + 1) / n - 1: include/srz.h has the table): what a caller
    evaluates an environment on to fill a cube for texture_cube, or to read one back."""
    c = (2.0 * torch.arange(n, dtype=torch.float64, device=device) + 1.0) / n - 1.0
    t, s = torch.meshgrid(c, c, indexing="ij")  # rows are t, columns s
    one = torch.ones_like(s)
    faces = ((one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one))  # n + s su + t sv, per face
    p = torch.stack([torch.stack(f, -1) for f in faces])
    return (p / p.norm(dim=-1, keepdim=True)).to(torch.float32)


def _cube_dims(fs, cube):
    tex_frames = _lead_frames(fs, cube, (4, 5), "texture_cube: cube", "a CUDA float32 tensor [6, N, N, C] or [n_frames, 6, N, N, C]",
                              lambda t: t.shape[-4] == 6 and t.shape[-3] == t.shape[-2])
    n, n_ch = cube.shape[-2], cube.shape[-1]
    if not (1 <= n <= abi.TEX_MAX_SIZE and 1 <= n_ch <= abi.ATTR_MAX_CH):
        raise ValueError(f"texture_cube: faces of {n} x {n} texels, {n_ch} channels; 1 .. {abi.TEX_MAX_SIZE} and 1 .. {abi.ATTR_MAX_CH} are supported")
    return tex_frames, n, n_ch


def texture_cube_grad(fs, vis, cube, dirs, gout, want_gtex=True, want_gdir=True, stream=None):
    """the backward of texture_cube(fs, vis, cube, dirs) by one FrameSet.texture_cube_grad call: gout [n_frames, C, rows, W] → (gtex,
    gdir), each None when not wanted (not both): gtex has cube's shape — a sum of float atomics into zeros, not bit-reproducible
    between runs; gdir [n_frames, 3, rows, W] is deterministic, zeros where nobody owns the pixel or its direction is not sampled, and
    is what interpolate's backward takes for a three-channel attribute.  stream: a raw stream handle, None = torch's current stream."""
    if not want_gtex and not want_gdir:
        raise ValueError("texture_cube_grad: neither gtex nor gdir is asked for")
    dirs = _plane(fs, dirs, 3, "texture_cube: dirs")
    tex_frames, n, n_ch = _cube_dims(fs, cube)
    cube, gout = cube.contiguous(), _gout(fs, gout, n_ch, "texture_cube_grad")
    gtex = torch.zeros_like(cube) if want_gtex else None
    gdir = torch.empty_like(dirs) if want_gdir else None
    fs.texture_cube_grad(_vis_ptr(fs, vis, "texture_cube_grad"), dirs.data_ptr(), gout.data_ptr(), cube.data_ptr(), n, n_ch, tex_frames, _ptr(gtex),
                         _ptr(gdir), abi.FUSED_CLEAR, _stream_ptr(stream))
    return gtex, gdir


class _TextureCube(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cube, dirs, fs, vis, stream):
        dirs = _plane(fs, dirs, 3, "texture_cube: dirs")
        tex_frames, n, n_ch = _cube_dims(fs, cube)
        cube = cube.contiguous()
        out = torch.empty(fs.interpolate_shape(n_ch), dtype=torch.float32, device=cube.device)
        fs.texture_cube(_vis_ptr(fs, vis, "texture_cube"), dirs.data_ptr(), cube.data_ptr(), n, n_ch, tex_frames, out.data_ptr(),
                        fs.interpolate_bytes(n_ch), abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.stream = fs, vis, stream
        ctx.save_for_backward(cube, dirs)
        return out

    @staticmethod
    def backward(ctx, gout):
        cube, dirs = ctx.saved_tensors
        return _backward(ctx, 2, lambda *need: texture_cube_grad(ctx.fs, ctx.vis, cube, dirs, gout, *need, ctx.stream))


def texture_cube(fs, vis, cube, dirs, stream=None):
    """a float cube map of the caller's own looked up by direction under a visibility buffer `vis` of FrameSet `fs`: cube is a CUDA
    float32 tensor [6, N, N, C] (one cube for every frame) or [n_frames, 6, N, N, C], faces +X -X +Y -Y +Z -Z, channels last, C <=
    abi.ATTR_MAX_CH, N <= abi.TEX_MAX_SIZE; dirs is [n_frames, 3, rows, W] — interpolate(fs, vis, attr) of a [T, 3, 3] attribute such
    as corner_attr's normals, of any length → [n_frames, C, rows, W] float32, bilinear and seamless across the cube's edges, zeros
    where nobody owns the pixel or its direction is not finite or zero (FrameSet.texture_cube; include/srz.h states the rule).
    Differentiable with respect to cube (float atomics into a zeroed tensor: cube.grad is not bit-reproducible between runs) and to
    dirs (deterministic), so texture_cube(fs, vis, cube, interpolate(fs, vis, corner_attr(fs, {slot: mesh_normals(ctx, slot,
    verts)}))) backpropagates to the cube and to the vertices.  Backward is one texture_cube_grad call that asks only for the
    outputs some input needs.  stream: a raw stream handle, None = torch's current stream."""
    return _TextureCube.apply(cube, dirs, fs, vis, stream)


def view_rays(screen_from_world, front=1.0, dtype=torch.float32):
    """the ray block of background from a camera, with differentiable torch ops: screen_from_world is the 4 x 4 matrix S a draw's
    ndc_mvp has in front of its model matrix (screen <- NDC <- projection <- view), [4, 4] or [n_frames, 4, 4], mathematical layout
    (S @ (P, 1) = (x w, y w, z w, w): a draw's column-major 16 floats reshaped [4, 4] and transposed) → [1, 9] or [n_frames, 9]
    float32 on S's device, a row r0[3] rx[3] ry[3] with r0 + x rx + y ry a direction of the world points that project onto the
    screen point (x, y).  With B the rows X, Y, W of S's first three columns, B (P - eye) = w (x, y, 1), so (rx, ry, r0) are the
    columns of B^-1, times `front`: the sign of w in FRONT of the camera — +1 for the reference's camera (lookAtLH with
    perspectiveLH_NO, srz.host.Scene and srz.scenes: w is the view-space depth), and for an OpenGL-style one (w = -z_view) too; -1
    for a projection whose w is negative in front.  Inverted in float64 and rounded once to float32 (dtype: torch.float64 keeps the
    binary64 block, for checks; background takes float32)."""
    S = screen_from_world
    if S.dim() not in (2, 3) or tuple(S.shape[-2:]) != (4, 4):
        raise ValueError(f"view_rays: screen_from_world must be [4, 4] or [n_frames, 4, 4], got {tuple(S.shape)}")
    if front not in (1, -1):
        raise ValueError(f"view_rays: front must be +1 or -1, got {front}")
    B = S.reshape(-1, 4, 4).to(torch.float64)[:, [0, 1, 3], :3]
    # the inverse by cofactors (its columns are the cross products of B's rows over the determinant): plain differentiable ops
    bx, by, bw = B[:, 0], B[:, 1], B[:, 2]
    cx, cy, cw = torch.linalg.cross(by, bw), torch.linalg.cross(bw, bx), torch.linalg.cross(bx, by)
    det = (bx * cx).sum(-1, keepdim=True)
    rows = torch.cat([cw, cx, cy], dim=1) / (det * float(front))  # r0, rx, ry
    return rows.to(dtype).contiguous()


_BG_WHERE = {"nobody": abi.BG_NOBODY, "all": abi.BG_ALL}


def _background_args(fs, vis, cube, rays, where):
    """→ (cube, rays, tex_frames, n, n_ch, ray_frames, where word), checked and contiguous"""
    if where not in _BG_WHERE:
        raise ValueError(f"background: where must be 'nobody' or 'all', got {where!r}")
    tex_frames, n, n_ch = _cube_dims(fs, cube)
    if rays is None or rays.dtype != torch.float32 or not rays.is_cuda or rays.dim() != 2 or rays.shape[1] != 9 or rays.shape[0] not in (1, fs.n_frames):
        raise ValueError(f"background: rays must be a CUDA float32 tensor [1 or {fs.n_frames}, 9]" + _got(rays, "plain"))
    if vis is None and where != "all":
        raise ValueError("background: vis may be None only with where='all'")
    return cube.contiguous(), rays.contiguous(), tex_frames, n, n_ch, rays.shape[0], _BG_WHERE[where]


def background_grad(fs, vis, cube, rays, gout, where="nobody", want_gtex=True, want_gray=True, stream=None):
    """the backward of background(fs, vis, cube, rays, where) by one FrameSet.background_grad call: gout [n_frames, C, rows, W] →
    (gtex, gray), each None when not wanted (not both): gtex has cube's shape — a sum of float atomics into zeros, not
    bit-reproducible between runs; gray has rays' shape, summed in a fixed tree (bit-reproducible for a shard layout).  stream: a raw
    stream handle, None = torch's current stream."""
    if not want_gtex and not want_gray:
        raise ValueError("background_grad: neither gtex nor gray is asked for")
    cube, rays, tex_frames, n, n_ch, ray_frames, w = _background_args(fs, vis, cube, rays, where)
    gout = _gout(fs, gout, n_ch, "background_grad")
    gtex = torch.zeros_like(cube) if want_gtex else None
    work_bytes = fs.background_work_bytes() if want_gray else 0
    gray, work = _reduced(rays, work_bytes) if want_gray else (None, None)
    fs.background_grad(None if vis is None else _vis_ptr(fs, vis, "background_grad"), rays.data_ptr(), ray_frames, gout.data_ptr(), cube.data_ptr(),
                       n, n_ch, tex_frames, w, _ptr(gtex), _ptr(gray), _ptr(work), work_bytes, abi.FUSED_CLEAR, _stream_ptr(stream))
    return gtex, gray


class _Background(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cube, rays, fs, vis, where, stream):
        cube, rays, tex_frames, n, n_ch, ray_frames, w = _background_args(fs, vis, cube, rays, where)
        out = torch.empty(fs.interpolate_shape(n_ch), dtype=torch.float32, device=cube.device)
        fs.background(None if vis is None else _vis_ptr(fs, vis, "background"), rays.data_ptr(), ray_frames, cube.data_ptr(), n, n_ch, tex_frames, w,
                      out.data_ptr(), fs.interpolate_bytes(n_ch), abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.where, ctx.stream = fs, vis, where, stream
        ctx.save_for_backward(cube, rays)
        return out

    @staticmethod
    def backward(ctx, gout):
        cube, rays = ctx.saved_tensors
        return _backward(ctx, 2, lambda *need: background_grad(ctx.fs, ctx.vis, cube, rays, gout, ctx.where, *need, ctx.stream))


def background(fs, vis, cube, rays, where="nobody", stream=None):
    """the environment behind a visibility buffer `vis` of FrameSet `fs`, by view ray: cube is texture_cube's cube ([6, N, N, C] or
    [n_frames, 6, N, N, C]), rays is view_rays' block [1, 9] or [n_frames, 9] → [n_frames, C, rows, W] float32: at the pixels nobody
    owns (where="nobody") or at every pixel (where="all"; vis may be None) the cube looked up along the pixel's ray r0 + x rx + y ry
    by texture_cube's rule, zeros at the owned pixels and where the ray is not finite or zero (FrameSet.background; include/srz.h
    states the rule).  So antialias(fs, vis, shaded + background(fs, vis, env, view_rays(S)), pos) blends an outline with what is
    behind it.  Differentiable with respect to cube (float atomics into a zeroed tensor: cube.grad is not bit-reproducible between
    runs) and to rays (a fixed tree: bit-reproducible), and through view_rays to the camera.  Backward is one background_grad call
    that asks only for the outputs some input needs.  stream: a raw stream handle, None = torch's current stream."""
    return _Background.apply(cube, rays, fs, vis, where, stream)


def _map_dims(fs, map):
    """map [H, W], [n_frames, H, W] or depth()'s [n_frames, 1, H, W] → (map_frames, H, W)"""
    map_frames = _lead_frames(fs, map, (2, 3, 4), "shadow: map", "a float32 tensor [H, W], [n_frames, H, W] or [n_frames, 1, H, W]",
                              lambda t: t.dim() < 4 or t.shape[1] == 1, cuda=False)
    h, w = map.shape[-2:]
    if not (1 <= w <= abi.TEX_MAX_SIZE and 1 <= h <= abi.TEX_MAX_SIZE):
        raise ValueError(f"shadow: map is {w} x {h} texels; 1 .. {abi.TEX_MAX_SIZE} are supported")
    _on_device(map, "shadow: map")
    return map_frames, h, w


def _sc_arg(fs, sc):
    return _on_device(_plane(fs, sc, 3, "shadow: sc", "a float32 tensor {shape}"), "shadow: sc")


def _ramp_args(bias, width):
    bias, width = float(bias), float(width)
    if not (math.isfinite(bias) and math.isfinite(width) and width >= 0.0):
        raise ValueError(f"shadow: bias and width must be finite and width >= 0, got bias {bias}, width {width}")
    return bias, width


def shadow_grad(fs, vis, map, sc, gout, bias, width, want_gmap=True, want_gsc=True, stream=None):
    """the backward of shadow(fs, vis, map, sc, bias, width) by one FrameSet.shadow_grad call: gout [n_frames, 1, rows, W] → (gmap,
    gsc), each None when not wanted (not both): gmap has map's shape — a sum of float atomics into zeros, not bit-reproducible
    between runs, all zeros with width == 0; gsc [n_frames, 3, rows, W] is deterministic, zeros where nobody owns the pixel or its
    coordinates are not finite, and is what interpolate's backward takes for a three-channel attribute.  bias and width get no
    gradient.  stream: a raw stream handle, None = torch's current stream."""
    if not want_gmap and not want_gsc:
        raise ValueError("shadow_grad: neither gmap nor gsc is asked for")
    bias, width = _ramp_args(bias, width)
    map_frames, h, w = _map_dims(fs, map)
    map, sc, gout = map.contiguous(), _sc_arg(fs, sc), _gout(fs, gout, 1, "shadow_grad")
    gmap = torch.zeros_like(map) if want_gmap else None
    gsc = torch.empty_like(sc) if want_gsc else None
    fs.shadow_grad(_vis_ptr(fs, vis, "shadow_grad"), sc.data_ptr(), gout.data_ptr(), map.data_ptr(), w, h, map_frames, bias, width, _ptr(gmap),
                   _ptr(gsc), abi.FUSED_CLEAR, _stream_ptr(stream))
    return gmap, gsc


class _Shadow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, map, sc, fs, vis, bias, width, stream):
        bias, width = _ramp_args(bias, width)
        map_frames, h, w = _map_dims(fs, map)
        map, sc = map.contiguous(), _sc_arg(fs, sc)
        out = torch.empty(fs.interpolate_shape(1), dtype=torch.float32, device=sc.device)
        fs.shadow(_vis_ptr(fs, vis, "shadow"), sc.data_ptr(), map.data_ptr(), w, h, map_frames, bias, width, out.data_ptr(),
                  fs.interpolate_bytes(1), abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.bias, ctx.width, ctx.stream = fs, vis, bias, width, stream
        ctx.save_for_backward(map, sc)
        return out

    @staticmethod
    def backward(ctx, gout):
        map, sc = ctx.saved_tensors
        return _backward(ctx, 2, lambda *need: shadow_grad(ctx.fs, ctx.vis, map, sc, gout, ctx.bias, ctx.width, *need, ctx.stream))


def shadow(fs, vis, map, sc, bias=0.0, width=0.0, stream=None):
    """a shadow-map lookup under a visibility buffer `vis` of FrameSet `fs` (the CAMERA's set): percentage-closer filtering of the
    depth map `map` — a CUDA float32 tensor [H, W] (one map for every frame), [n_frames, H, W] or depth()'s [n_frames, 1, H, W]; a
    non-contiguous view such as vis_l[:, 0] is made contiguous; on a sharded context the WHOLE map, gathered — at the coordinates sc
    [n_frames, 3, rows, W]: sx, sy in map texels with the texel centres on the integers (a depth plane's texel (x, y) is the depth at
    screen (x, y)), sd in the map's depth units → [n_frames, 1, rows, W] float32, 1 lit .. 0 shadowed, 1 where the coordinates are not
    finite or beyond the map, zeros where nobody owns the pixel (FrameSet.shadow; include/srz.h states the rule).  The four texels
    around (sx, sy) each pass (map + bias) - sd >= 0 or fail it — width == 0, the hard test — or, width > 0, are ramped linearly over
    that width in depth, and the four results are blended bilinearly.  Differentiable with respect to map (float atomics into a
    zeroed tensor: map.grad is not bit-reproducible between runs; zero with width == 0) and to sc (deterministic); bias and width get
    no gradient.  THE CHAIN, a light's view being just another set fs_l of the same triangles with its own matrices:
        pos_l = scene_positions(fs_l, ...)                     # [n, T, 3, 3]: the light set's screen positions
        lit = shadow(fs_cam, vis_cam, depth(fs_l, vis_l, pos_l), interpolate(fs_cam, vis_cam, pos_l.view(n, T, 3, 3)), bias, width)
    depth() is plane 0 of the light's visibility buffer (+inf where nobody is: lit) as a function of the occluders' positions, and
    the light set's positions interpolated over the CAMERA set are every camera pixel's (sx, sy, sd): pos_l.grad gets the receiver's
    share through interpolate and the occluder's through depth.  With SEVERAL LIGHTS each shadowed light takes its own light() call,
    and its factor is multiplied in torch: light() sums its lights before it returns.  Screen-linear interpolation of light-space
    positions is exact ONLY WHEN NEITHER VIEW DIVIDES BY w (orthographic camera and light); otherwise interpolate the world positions
    and transform them in torch, or use interpolate_persp.  Backward is one shadow_grad call that asks only for the outputs some
    input needs.  stream: a raw stream handle, None = torch's current stream."""
    return _Shadow.apply(map, sc, fs, vis, bias, width, stream)


def _params(fs, what, lights, pieces):
    """the parameter block of `what`: the three-vector pieces [(name, [3] or [n_frames, 3])] in order, then the lights' rows"""
    if lights is None or lights.dim() not in (2, 3) or lights.shape[-1] != 6 or not 1 <= lights.shape[-2] <= abi.LIGHT_MAX:
        raise ValueError(f"{what}: lights must be [L, 6] or [n_frames, L, 6] with 1 <= L <= {abi.LIGHT_MAX}" + _got(lights, "shape"))
    for name, t in pieces:
        if t is None or t.dim() not in (1, 2) or t.shape[-1] != 3:
            raise ValueError(f"{what}: {name} must be [3] or [n_frames, 3]" + _got(t, "shape"))
    per_frame = lights.dim() == 3 or any(t.dim() == 2 for _, t in pieces)
    n = fs.n_frames if per_frame else 1
    n_l = lights.shape[-2]
    rows = [t.reshape(-1, 3) for _, t in pieces] + [lights.reshape(-1, 6 * n_l)]
    for (name, _), r in zip(pieces + [("lights", lights)], rows):
        if r.shape[0] not in (1, n):
            raise ValueError(f"{what}: {name} has {r.shape[0]} frames, the set {fs.n_frames}")
    return torch.cat([r.expand(n, r.shape[1]) for r in rows], dim=1).to(torch.float32).contiguous()


def light_params(fs, lights, eye, ka, ks):
    """the parameter block of light / light_grad from its pieces, with torch ops (so gradients of the block flow back to the pieces):
    lights [L, 6] or [n_frames, L, 6] (a light: pos[3], intensity[3]), eye, ka, ks [3] or [n_frames, 3] → [1, 9 + 6 L] when every piece
    is shared by the frames, else [n_frames, 9 + 6 L] (per frame as soon as one of them is)"""
    return _params(fs, "light", lights, [("eye", eye), ("ka", ka), ("ks", ks)])


def _light_args(fs, nrm, pos, kd, par, p):
    """→ (nrm, pos, kd or None, par, n_lights, par_frames), checked and contiguous"""
    nrm, pos = _plane(fs, nrm, 3, "light: nrm"), _plane(fs, pos, 3, "light: pos")
    kd = None if kd is None else _plane(fs, kd, 3, "light: kd")
    if par is None or par.dtype != torch.float32 or not par.is_cuda or par.dim() != 2 or par.shape[1] < 15 or (par.shape[1] - 9) % 6:
        raise ValueError("light: par must be a CUDA float32 tensor [1 or n_frames, 9 + 6 L]" + _got(par, "plain"))
    n_l = (par.shape[1] - 9) // 6
    if n_l > abi.LIGHT_MAX or par.shape[0] not in (1, fs.n_frames):
        raise ValueError(f"light: par of {par.shape[0]} frames and {n_l} lights; 1 or {fs.n_frames} frames and 1 .. {abi.LIGHT_MAX} lights are supported")
    if int(p) != p or not 1 <= p <= 256:
        raise ValueError(f"light: p must be an integer in 1 .. 256, got {p}")
    return nrm, pos, kd, par.contiguous(), n_l, par.shape[0]


def light_grad(fs, vis, nrm, pos, kd, par, p, gout, want_gnrm=True, want_gpos=True, want_gkd=True, want_gpar=True, stream=None):
    """the backward of light by one FrameSet.light_grad call: par is light_params' block, gout [n_frames, 3, rows, W] → (gnrm, gpos,
    gkd, gpar), each None when not wanted (not all; gkd is None without kd): the planes are deterministic, zeros where nobody owns
    the pixel or its normal is not lit; gpar has par's shape, reduced in a fixed tree (bit-reproducible for a shard layout).
    stream: a raw stream handle, None = torch's current stream."""
    want_gkd = want_gkd and kd is not None
    if not (want_gnrm or want_gpos or want_gkd or want_gpar):
        raise ValueError("light_grad: no gradient is asked for")
    nrm, pos, kd, par, n_l, par_frames = _light_args(fs, nrm, pos, kd, par, p)
    gout = _gout(fs, gout, 3, "light_grad")
    gnrm, gpos, gkd = (torch.empty_like(nrm) if w else None for w in (want_gnrm, want_gpos, want_gkd))
    work_bytes = fs.light_work_bytes(n_l) if want_gpar else 0
    gpar, work = _reduced(par, work_bytes) if want_gpar else (None, None)
    fs.light_grad(_vis_ptr(fs, vis, "light_grad"), nrm.data_ptr(), pos.data_ptr(), _ptr(kd), par.data_ptr(), n_l, par_frames, int(p), gout.data_ptr(),
                  _ptr(gnrm), _ptr(gpos), _ptr(gkd), _ptr(gpar), _ptr(work), work_bytes, abi.FUSED_CLEAR, _stream_ptr(stream))
    return gnrm, gpos, gkd, gpar


class _Light(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nrm, pos, kd, par, fs, vis, p, stream):
        nrm, pos, kd, par, n_l, par_frames = _light_args(fs, nrm, pos, kd, par, p)
        out = torch.empty(fs.interpolate_shape(3), dtype=torch.float32, device=nrm.device)
        fs.light(_vis_ptr(fs, vis, "light"), nrm.data_ptr(), pos.data_ptr(), _ptr(kd), par.data_ptr(), n_l, par_frames, int(p), out.data_ptr(),
                 fs.interpolate_bytes(3), abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.p, ctx.stream, ctx.has_kd = fs, vis, int(p), stream, kd is not None
        ctx.save_for_backward(nrm, pos, par, *([kd] if kd is not None else []))
        return out

    @staticmethod
    def backward(ctx, gout):
        nrm, pos, par = ctx.saved_tensors[:3]
        kd = ctx.saved_tensors[3] if ctx.has_kd else None
        return _backward(ctx, 4, lambda *need: light_grad(ctx.fs, ctx.vis, nrm, pos, kd, par, ctx.p, gout, *need, ctx.stream), (2, ctx.has_kd))


def light(fs, vis, nrm, pos, kd, lights, eye, ka, ks, p, stream=None):
    """Blinn-Phong under point lights for the caller's own planes under a visibility buffer `vis` of FrameSet `fs`: nrm, pos and kd (or
    None: albedo ones) are [n_frames, 3, rows, W] CUDA float32 — interpolate's normals and positions, texture's albedo —, lights is
    [L, 6] or [n_frames, L, 6] (pos[3], intensity[3]; L <= abi.LIGHT_MAX), eye, ka, ks [3] or [n_frames, 3], p an integer exponent in
    1 .. 256 → [n_frames, 3, rows, W] float32: true 1 / r² attenuation, a normalised half vector, no clamp, zeros where nobody owns the
    pixel or its normal has no finite positive length (FrameSet.light; include/srz.h states the rule — nothing of the built-in
    shaders).  Differentiable with respect to nrm, pos, kd (deterministic planes) and to lights, eye, ka, ks (sums over the pixels in
    a fixed tree: bit-reproducible), not to p.  Backward is one light_grad call that asks only for the outputs some input needs.
    stream: a raw stream handle, None = torch's current stream."""
    return _Light.apply(nrm, pos, kd, light_params(fs, lights, eye, ka, ks), fs, vis, p, stream)


def microfacet_params(fs, lights, eye, amb):
    """the parameter block of microfacet / microfacet_grad from its pieces, with torch ops (so gradients of the block flow back to the
    pieces): lights [L, 6] or [n_frames, L, 6] (a light: pos[3], intensity[3]), eye, amb [3] or [n_frames, 3] → [1, 6 + 6 L] when every
    piece is shared by the frames, else [n_frames, 6 + 6 L] (per frame as soon as one of them is)"""
    return _params(fs, "microfacet", lights, [("eye", eye), ("amb", amb)])


def _microfacet_args(fs, nrm, pos, base, mat, par):
    """→ (nrm, pos, base or None, mat, par, n_lights, par_frames), checked and contiguous"""
    nrm, pos = _plane(fs, nrm, 3, "microfacet: nrm", got="pair"), _plane(fs, pos, 3, "microfacet: pos", got="pair")
    base = None if base is None else _plane(fs, base, 3, "microfacet: base", got="pair")
    mat = _plane(fs, mat, 2, "microfacet: mat", got="pair")
    if par is None or par.dtype != torch.float32 or not par.is_cuda or par.dim() != 2 or par.shape[1] < 12 or (par.shape[1] - 6) % 6:
        raise ValueError("microfacet: par must be a CUDA float32 tensor [1 or n_frames, 6 + 6 L]" + _got(par, "plain"))
    n_l = (par.shape[1] - 6) // 6
    if n_l > abi.LIGHT_MAX or par.shape[0] not in (1, fs.n_frames):
        raise ValueError(f"microfacet: par of {par.shape[0]} frames and {n_l} lights; 1 or {fs.n_frames} frames and 1 .. {abi.LIGHT_MAX} "
                         "lights are supported")
    return nrm, pos, base, mat, par.contiguous(), n_l, par.shape[0]


def microfacet_grad(fs, vis, nrm, pos, base, mat, par, gout, want_gnrm=True, want_gpos=True, want_gbase=True, want_gmat=True, want_gpar=True,
                    stream=None):
    """the backward of microfacet by one FrameSet.microfacet_grad call: par is microfacet_params' block, gout [n_frames, 3, rows, W] →
    (gnrm, gpos, gbase, gmat, gpar), each None when not wanted (not all; gbase is None without base): the planes are deterministic,
    zeros where nobody owns the pixel or its normal is not lit, gmat [n_frames, 2, rows, W] zero where a clamp holds; gpar has par's
    shape, reduced in a fixed tree (bit-reproducible for a shard layout).  stream: a raw stream handle, None = torch's current stream."""
    want_gbase = want_gbase and base is not None
    if not (want_gnrm or want_gpos or want_gbase or want_gmat or want_gpar):
        raise ValueError("microfacet_grad: no gradient is asked for")
    nrm, pos, base, mat, par, n_l, par_frames = _microfacet_args(fs, nrm, pos, base, mat, par)
    gout = _gout(fs, gout, 3, "microfacet_grad")
    gnrm, gpos, gbase = (torch.empty_like(nrm) if w else None for w in (want_gnrm, want_gpos, want_gbase))
    gmat = torch.empty_like(mat) if want_gmat else None
    work_bytes = fs.microfacet_work_bytes(n_l) if want_gpar else 0
    gpar, work = _reduced(par, work_bytes) if want_gpar else (None, None)
    fs.microfacet_grad(_vis_ptr(fs, vis, "microfacet_grad"), nrm.data_ptr(), pos.data_ptr(), _ptr(base), mat.data_ptr(), par.data_ptr(), n_l,
                       par_frames, gout.data_ptr(), _ptr(gnrm), _ptr(gpos), _ptr(gbase), _ptr(gmat), _ptr(gpar), _ptr(work), work_bytes,
                       abi.FUSED_CLEAR, _stream_ptr(stream))
    return gnrm, gpos, gbase, gmat, gpar


class _Microfacet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nrm, pos, base, mat, par, fs, vis, stream):
        nrm, pos, base, mat, par, n_l, par_frames = _microfacet_args(fs, nrm, pos, base, mat, par)
        out = torch.empty(fs.interpolate_shape(3), dtype=torch.float32, device=nrm.device)
        fs.microfacet(_vis_ptr(fs, vis, "microfacet"), nrm.data_ptr(), pos.data_ptr(), _ptr(base), mat.data_ptr(), par.data_ptr(), n_l,
                      par_frames, out.data_ptr(), fs.interpolate_bytes(3), abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.stream, ctx.has_base = fs, vis, stream, base is not None
        ctx.save_for_backward(nrm, pos, mat, par, *([base] if base is not None else []))
        return out

    @staticmethod
    def backward(ctx, gout):
        nrm, pos, mat, par = ctx.saved_tensors[:4]
        base = ctx.saved_tensors[4] if ctx.has_base else None
        return _backward(ctx, 5, lambda *need: microfacet_grad(ctx.fs, ctx.vis, nrm, pos, base, mat, par, gout, *need, ctx.stream), (2, ctx.has_base))


def microfacet(fs, vis, nrm, pos, base, mat, lights, eye, amb, stream=None):
    """Cook-Torrance shading under point lights for the caller's own planes under a visibility buffer `vis` of FrameSet `fs`: nrm, pos
    and base (or None: base colour ones) are [n_frames, 3, rows, W] CUDA float32 — interpolate's or normal_map's normals, interpolate's
    positions, texture's base colour —, mat [n_frames, 2, rows, W] the roughness (clamped to [1 / 16, 1]) and the metallic (clamped to
    [0, 1]) — a two-channel texture's output —, lights [L, 6] or [n_frames, L, 6] (pos[3], intensity[3]; L <= abi.LIGHT_MAX), eye, amb [3]
    or [n_frames, 3] → [n_frames, 3, rows, W] float32: a GGX distribution, Schlick-Smith visibility and Schlick Fresnel over the
    metallic-roughness parametrisation, true 1 / r² attenuation, amb * base added, no clamp, zeros where nobody owns the pixel or its
    normal has no finite positive length (FrameSet.microfacet; include/srz.h states the rule).  Differentiable with respect to nrm, pos,
    base, mat (deterministic planes; mat's gradient is zero where a clamp holds) and to lights, eye, amb (sums over the pixels in a
    fixed tree: bit-reproducible).  Backward is one microfacet_grad call that asks only for the outputs some input needs.  stream: a raw
    stream handle, None = torch's current stream."""
    return _Microfacet.apply(nrm, pos, base, mat, microfacet_params(fs, lights, eye, amb), fs, vis, stream)


def _reflect_args(fs, nrm, pos, eye):
    """→ (nrm, pos, eye [1 or n_frames, 3]), checked and contiguous"""
    nrm, pos = _plane(fs, nrm, 3, "reflect: nrm", got="pair"), _plane(fs, pos, 3, "reflect: pos", got="pair")
    if eye is None or eye.dtype != torch.float32 or not eye.is_cuda or eye.dim() not in (1, 2) or eye.shape[-1] != 3 or \
            (eye.dim() == 2 and eye.shape[0] not in (1, fs.n_frames)):
        raise ValueError(f"reflect: eye must be a CUDA float32 tensor [3] or [1 or {fs.n_frames}, 3]" + _got(eye, "plain"))
    return nrm, pos, eye.reshape(-1, 3).contiguous()


def reflect_grad(fs, vis, nrm, pos, eye, gout, want_gnrm=True, want_gpos=True, stream=None):
    """the backward of reflect by one FrameSet.reflect_grad call: gout [n_frames, 4, rows, W] → (gnrm, gpos), each [n_frames, 3, rows,
    W] or None when not wanted (not both): per pixel, deterministic, zeros where nobody owns the pixel, its normal is not lit or it has
    no view.  The eye's gradient is minus gpos summed over a frame.  stream: a raw stream handle, None = torch's current stream."""
    if not (want_gnrm or want_gpos):
        raise ValueError("reflect_grad: no gradient is asked for")
    nrm, pos, eye = _reflect_args(fs, nrm, pos, eye)
    gout = _plane(fs, gout, 4, "reflect_grad: gout", got="pair")
    gnrm, gpos = (torch.empty_like(nrm) if w else None for w in (want_gnrm, want_gpos))
    fs.reflect_grad(_vis_ptr(fs, vis, "reflect_grad"), nrm.data_ptr(), pos.data_ptr(), eye.data_ptr(), eye.shape[0], gout.data_ptr(), _ptr(gnrm),
                    _ptr(gpos), abi.FUSED_CLEAR, _stream_ptr(stream))
    return gnrm, gpos


class _Reflect(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nrm, pos, eye, fs, vis, stream):
        eye_shape = None if eye is None else tuple(eye.shape)
        nrm, pos, eye = _reflect_args(fs, nrm, pos, eye)
        ctx.eye_shape = eye_shape
        out = torch.empty(fs.interpolate_shape(4), dtype=torch.float32, device=nrm.device)
        fs.reflect(_vis_ptr(fs, vis, "reflect"), nrm.data_ptr(), pos.data_ptr(), eye.data_ptr(), eye.shape[0], out.data_ptr(),
                   fs.interpolate_bytes(4), abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.stream = fs, vis, stream
        ctx.save_for_backward(nrm, pos, eye)
        return out

    @staticmethod
    def backward(ctx, gout):
        nrm, pos, eye = ctx.saved_tensors
        need_n, need_p, need_e = ctx.needs_input_grad[:3]
        gnrm = gpos = geye = None
        if need_n or need_p or need_e:
            gnrm, gpos = reflect_grad(ctx.fs, ctx.vis, nrm, pos, eye, gout, need_n, need_p or need_e, ctx.stream)
        if need_e:  # R and nv depend on eye - P only: the eye's gradient is minus the owned pixels' gpos, summed (nobody's are zeros)
            per_frame = -gpos.sum(dim=(2, 3))
            geye = (per_frame if eye.shape[0] != 1 else per_frame.sum(0, keepdim=True)).reshape(ctx.eye_shape)
        return gnrm, gpos if need_p else None, geye, None, None, None


def reflect(fs, vis, nrm, pos, eye, stream=None):
    """the reflection vector and n.v for image-based lighting under a visibility buffer `vis` of FrameSet `fs`: nrm, pos
    [n_frames, 3, rows, W] CUDA float32, eye [3] or [n_frames, 3] on the device → [n_frames, 4, rows, W]: planes 0..2 R = 2 (N.Vd) N -
    Vd — the direction texture_cube_mip takes —, plane 3 the RAW N.Vd — what ibl takes, and clamps — (FrameSet.reflect; include/srz.h
    states the rule).  Four zeros where nobody owns the pixel, its normal has no finite positive length or the eye lies on it: a zero
    direction is texture_cube's "unsampled".  Differentiable with respect to nrm, pos (one reflect_grad call, deterministic planes) and
    eye (minus the sum of pos's gradient, a torch reduction).  stream: a raw stream handle, None = torch's current stream."""
    return _Reflect.apply(nrm, pos, eye, fs, vis, stream)


def brdf_table(ctx_or_fs, n, m=64, stream=None, device=None):
    """the split-sum table [n, n, 2] CUDA float32 (A, B) of microfacet's own specular lobe, for ibl: rows over n.v in [0, 1], columns
    over the roughness in [1 / 16, 1], nodes on the clamp edges; m rings of 2 m samples (Context.brdf_table; include/srz.h states the
    quadrature).  Deterministic.  Build it once.  ctx_or_fs: the Context, or a FrameSet of it."""
    ctx = getattr(ctx_or_fs, "ctx", ctx_or_fs)
    if not 2 <= int(n) <= abi.BRDF_TABLE_MAX or not 1 <= int(m) <= 256:
        raise ValueError(f"brdf_table: 2 <= n <= {abi.BRDF_TABLE_MAX} and 1 <= m <= 256, got n {n}, m {m}")
    tab = _on_device(torch.empty((int(n), int(n), 2), dtype=torch.float32, device=device or "cuda"), "brdf_table: tab")
    ctx.brdf_table(tab.data_ptr(), tab.numel() * 4, int(n), int(m), _stream_ptr(stream))
    return tab


def _ibl_args(fs, base, mat, nv, irr, spec, tab):
    """→ (base or None, mat, nv, irr, spec, tab, n), checked and contiguous"""
    base = None if base is None else _plane(fs, base, 3, "ibl: base", got="pair")
    mat, nv = _plane(fs, mat, 2, "ibl: mat", got="pair"), _plane(fs, nv, 1, "ibl: nv", got="pair")
    irr, spec = _plane(fs, irr, 3, "ibl: irr", got="pair"), _plane(fs, spec, 3, "ibl: spec", got="pair")
    if tab is None or tab.dtype != torch.float32 or not tab.is_cuda or tab.dim() != 3 or tab.shape[0] != tab.shape[1] or tab.shape[2] != 2 or \
            not 2 <= tab.shape[0] <= abi.BRDF_TABLE_MAX:
        raise ValueError(f"ibl: tab must be a CUDA float32 tensor [n, n, 2] with 2 <= n <= {abi.BRDF_TABLE_MAX}" + _got(tab, "pair"))
    return base, mat, nv, irr, spec, tab.contiguous(), tab.shape[0]


def ibl_grad(fs, vis, base, mat, nv, irr, spec, tab, gout, want_gbase=True, want_gmat=True, want_gnv=True, want_girr=True, want_gspec=True,
             want_gtab=True, stream=None):
    """the backward of ibl by one FrameSet.ibl_grad call: gout [n_frames, 3, rows, W] → (gbase, gmat, gnv, girr, gspec, gtab), each None
    when not wanted (not all; gbase is None without base): the planes per pixel and deterministic, gmat and gnv zero where a clamp
    holds; gtab [n, n, 2] summed with float adds (not bit-reproducible).  stream: a raw stream handle, None = torch's current stream."""
    want_gbase = want_gbase and base is not None
    if not (want_gbase or want_gmat or want_gnv or want_girr or want_gspec or want_gtab):
        raise ValueError("ibl_grad: no gradient is asked for")
    base, mat, nv, irr, spec, tab, n = _ibl_args(fs, base, mat, nv, irr, spec, tab)
    gout = _plane(fs, gout, 3, "ibl_grad: gout", got="pair")
    gbase, gmat, gnv, girr, gspec = (torch.empty_like(t) if w else None for t, w in
                                     ((irr, want_gbase), (mat, want_gmat), (nv, want_gnv), (irr, want_girr), (spec, want_gspec)))
    gtab = torch.zeros_like(tab) if want_gtab else None
    fs.ibl_grad(_vis_ptr(fs, vis, "ibl_grad"), _ptr(base), mat.data_ptr(), nv.data_ptr(), irr.data_ptr(), spec.data_ptr(), tab.data_ptr(), n,
                gout.data_ptr(), _ptr(gbase), _ptr(gmat), _ptr(gnv), _ptr(girr), _ptr(gspec), _ptr(gtab), abi.FUSED_CLEAR, _stream_ptr(stream))
    return gbase, gmat, gnv, girr, gspec, gtab


class _Ibl(torch.autograd.Function):
    @staticmethod
    def forward(ctx, base, mat, nv, irr, spec, tab, fs, vis, stream):
        base, mat, nv, irr, spec, tab, n = _ibl_args(fs, base, mat, nv, irr, spec, tab)
        out = torch.empty(fs.interpolate_shape(3), dtype=torch.float32, device=mat.device)
        fs.ibl(_vis_ptr(fs, vis, "ibl"), _ptr(base), mat.data_ptr(), nv.data_ptr(), irr.data_ptr(), spec.data_ptr(), tab.data_ptr(), n,
               out.data_ptr(), fs.interpolate_bytes(3), abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.stream, ctx.has_base = fs, vis, stream, base is not None
        ctx.save_for_backward(mat, nv, irr, spec, tab, *([base] if base is not None else []))
        return out

    @staticmethod
    def backward(ctx, gout):
        mat, nv, irr, spec, tab = ctx.saved_tensors[:5]
        base = ctx.saved_tensors[5] if ctx.has_base else None
        return _backward(ctx, 6, lambda *need: ibl_grad(ctx.fs, ctx.vis, base, mat, nv, irr, spec, tab, gout, *need, ctx.stream), (0, ctx.has_base))


def ibl(fs, vis, base, mat, nv, irr, spec, tab, stream=None):
    """image-based lighting's split-sum combine for the caller's own planes under a visibility buffer `vis` of FrameSet `fs`: base (or
    None: ones), irr — texture_cube of cube_irradiance at the normal —, spec — texture_cube_mip of cube_prefilter_pyramid at reflect's R
    and roughness * (levels - 1) — [n_frames, 3, rows, W] CUDA float32, mat [n_frames, 2, rows, W] (roughness, metallic: microfacet's
    clamps), nv [n_frames, 1, rows, W] (reflect's plane 3; clamped to [0, 1] here), tab brdf_table's [n, n, 2] →
    [n_frames, 3, rows, W]: base (1 - metallic) irr + spec (F0 A + B), (A, B) bilinear in the table, no pi, no clamp of the result,
    zeros where nobody owns the pixel (FrameSet.ibl; include/srz.h states the rule).  Differentiable with respect to base, mat, nv,
    irr, spec (deterministic planes) and tab (float adds).  Backward is one ibl_grad call that asks only for the outputs some input
    needs.  Add microfacet(...) for the point lights.  stream: a raw stream handle, None = torch's current stream."""
    return _Ibl.apply(base, mat, nv, irr, spec, tab, fs, vis, stream)


def _normal_map_args(fs, nrm, tan, m):
    """→ (nrm, tan, m), checked and contiguous"""
    return _plane(fs, nrm, 3, "normal_map: nrm"), _plane(fs, tan, 4, "normal_map: tan"), _plane(fs, m, 3, "normal_map: m")


def normal_map_grad(fs, vis, nrm, tan, m, gout, want_gnrm=True, want_gtan=True, want_gm=True, stream=None):
    """the backward of normal_map by one FrameSet.normal_map_grad call: gout [n_frames, 3, rows, W] → (gnrm, gtan, gm), each None when
    not wanted (not all): gnrm and gm [n_frames, 3, rows, W], gtan [n_frames, 4, rows, W] with a zero w plane; per pixel,
    deterministic, zeros where nobody owns the pixel.  stream: a raw stream handle, None = torch's current stream."""
    if not (want_gnrm or want_gtan or want_gm):
        raise ValueError("normal_map_grad: no gradient is asked for")
    nrm, tan, m = _normal_map_args(fs, nrm, tan, m)
    gout = _gout(fs, gout, 3, "normal_map_grad")
    gnrm, gtan, gm = (torch.empty_like(t) if w else None for t, w in ((nrm, want_gnrm), (tan, want_gtan), (m, want_gm)))
    fs.normal_map_grad(_vis_ptr(fs, vis, "normal_map_grad"), nrm.data_ptr(), tan.data_ptr(), m.data_ptr(), gout.data_ptr(), _ptr(gnrm), _ptr(gtan),
                       _ptr(gm), abi.FUSED_CLEAR, _stream_ptr(stream))
    return gnrm, gtan, gm


class _NormalMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nrm, tan, m, fs, vis, stream):
        nrm, tan, m = _normal_map_args(fs, nrm, tan, m)
        out = torch.empty(fs.interpolate_shape(3), dtype=torch.float32, device=nrm.device)
        fs.normal_map(_vis_ptr(fs, vis, "normal_map"), nrm.data_ptr(), tan.data_ptr(), m.data_ptr(), out.data_ptr(), fs.interpolate_bytes(3),
                      abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.stream = fs, vis, stream
        ctx.save_for_backward(nrm, tan, m)
        return out

    @staticmethod
    def backward(ctx, gout):
        nrm, tan, m = ctx.saved_tensors
        return _backward(ctx, 3, lambda *need: normal_map_grad(ctx.fs, ctx.vis, nrm, tan, m, gout, *need, ctx.stream))


def normal_map(fs, vis, nrm, tan, m, stream=None):
    """tangent-space normal mapping under a visibility buffer `vis` of FrameSet `fs`: nrm [n_frames, 3, rows, W] (interpolate's normals
    of any length), tan [n_frames, 4, rows, W] (interpolate's of mesh_tangents' 4-channel corner_attr: tangent and handedness) and m
    [n_frames, 3, rows, W] (the tangent-space normal as the caller decoded it: texture's output, or a learned signed map) →
    [n_frames, 3, rows, W] float32, the unit shading normal light and texture_cube take: m.x T + m.y B + m.z N normalised, T the
    tangent made orthogonal to N, B = cross(N, T) * sign(w); zeros where nobody owns the pixel or the normal has no finite positive
    length, the unperturbed unit normal where there is no tangent frame (FrameSet.normal_map; include/srz.h states the rule).
    Differentiable with respect to nrm, tan and m (per pixel, deterministic; no gradient to the handedness).  Backward is one
    normal_map_grad call that asks only for the outputs some input needs.  stream: a raw stream handle, None = torch's current stream."""
    return _NormalMap.apply(nrm, tan, m, fs, vis, stream)


def interpolate_deriv(fs, vis, attr, stream=None):
    """the screen-space derivatives of interpolate(fs, vis, attr): attr as interpolate takes it with C <= abi.ATTR_MAX_CH // 2 →
    [n_frames, 2 C, rows, W] float32, plane 2 ch the change of channel ch per one-pixel step in x, plane 2 ch + 1 in y — constants of
    each pixel's owner, from the set's own positions (FrameSet.interpolate_deriv); zeros where nobody owns the pixel.  For a [T, 3, 2]
    uv attribute these are the planes ux, uy, vx, vy texture_mip takes.  Not differentiable: the planes only select a mip level.
    stream: a raw stream handle, None = torch's current stream."""
    attr_frames, tris, n_ch = _attr_dims(fs, attr)
    attr = attr.detach().contiguous()
    if n_ch > abi.ATTR_MAX_CH // 2:
        raise ValueError(f"interpolate_deriv: {n_ch} channels; at most {abi.ATTR_MAX_CH // 2} are supported")
    out = torch.empty(fs.interpolate_shape(2 * n_ch), dtype=torch.float32, device=attr.device)
    fs.interpolate_deriv(_vis_ptr(fs, vis, "interpolate_deriv"), attr.data_ptr(), n_ch, attr_frames, tris, out.data_ptr(),
                         fs.interpolate_bytes(2 * n_ch), abi.FUSED_CLEAR, _stream_ptr(stream))
    return out


def _mip_dims(tex_shape, n_levels):
    """(tex_frames, h, w, n_ch, n_levels) of a texture shape [H, W, C] or [frames, H, W, C]; n_levels None: every level there is"""
    from . import mip_levels
    tex_frames = tex_shape[0] if len(tex_shape) == 4 else 1
    h, w, n_ch = tex_shape[-3:]
    most = mip_levels(w, h)
    n_levels = most if n_levels is None else n_levels
    if most == 0 or not 1 <= n_levels <= most:
        raise ValueError(f"mip: a {w} x {h} texture has {most} levels, {n_levels} asked for")
    return tex_frames, h, w, n_ch, n_levels


def mip_build(ctx_or_fs, tex, n_levels=None, stream=None):
    """the mip pyramid of a CUDA float32 texture [H, W, C] or [frames, H, W, C]: the levels 1 .. n_levels - 1 (None: every level
    srz.mip_levels counts) as ONE flat float32 tensor, level-major (mip_views takes it apart); each level the box filter of the level
    above it, deterministic (Context.mip_build).  ctx_or_fs: the Context, or a FrameSet of it."""
    from . import mip_bytes
    ctx = getattr(ctx_or_fs, "ctx", ctx_or_fs)
    if tex is None or tex.dtype != torch.float32 or not tex.is_cuda or tex.dim() not in (3, 4):
        raise ValueError("mip_build: tex must be a CUDA float32 tensor [H, W, C] or [frames, H, W, C]" + _got(tex, "plain"))
    tex = tex.contiguous()
    tex_frames, h, w, n_ch, n_levels = _mip_dims(tuple(tex.shape), n_levels)
    nbytes = mip_bytes(w, h, n_ch, tex_frames, n_levels)
    mip = torch.empty((nbytes // 4,), dtype=torch.float32, device=tex.device)
    if n_levels > 1:
        ctx.mip_build(tex.data_ptr(), w, h, n_ch, tex_frames, n_levels, mip.data_ptr(), nbytes, _stream_ptr(stream))
    return mip


def mip_views(mip, tex_shape, n_levels=None):
    """the levels 1 .. n_levels - 1 of a flat pyramid (mip_build's, or a gradient pyramid) as views [h_l, w_l, C] or
    [frames, h_l, w_l, C], in level order; tex_shape: the shape of level 0"""
    tex_frames, h, w, n_ch, n_levels = _mip_dims(tuple(tex_shape), n_levels)
    views, off = [], 0
    for l in range(1, n_levels):
        hl, wl = max(1, h >> l), max(1, w >> l)
        n = tex_frames * hl * wl * n_ch
        views.append(mip[off:off + n].view((tex_frames, hl, wl, n_ch) if len(tex_shape) == 4 else (hl, wl, n_ch)))
        off += n
    return views


def _uvd_arg(fs, uvd, n_levels):
    if n_levels == 1 and uvd is None:
        return None
    return _plane(fs, uvd, 4, "texture_mip: uvd", got="").detach()


def texture_mip_grad(fs, vis, tex, uv, uvd, gout, wrap=False, n_levels=None, mip=None, want_gtex=True, want_guv=True, fold=True, stream=None):
    """the backward of texture_mip(fs, vis, tex, uv, uvd, wrap, n_levels) by one FrameSet.texture_mip_grad call, the level held fixed:
    gout [n_frames, C, rows, W] → (gtex, guv), each None when not wanted (not both).  gtex has tex's shape: the adds to level 0 and,
    with fold (one Context.mip_fold call), the gradient pyramid folded into it — float atomics into zeros, not bit-reproducible;
    fold=False returns (gtex, gmip, guv) with the level-0 adds and the flat gradient pyramid apart.  guv is deterministic.  mip: the
    pyramid mip_build made of tex (built here when guv needs it and none is given)."""
    if not want_gtex and not want_guv:
        raise ValueError("texture_mip_grad: neither gtex nor guv is asked for")
    from . import mip_bytes
    uv = _plane(fs, uv, 2, "texture: uv")
    tex_frames, h, w, n_ch = _tex_dims(fs, tex)
    tex = tex.detach().contiguous()
    n_levels = _mip_dims(tuple(tex.shape), n_levels)[4]
    uvd = _uvd_arg(fs, uvd, n_levels)
    gout = _gout(fs, gout, n_ch, "texture_mip_grad")
    s = _stream_ptr(stream)
    nbytes = mip_bytes(w, h, n_ch, tex_frames, n_levels)
    if n_levels > 1 and mip is not None and (mip.dtype != torch.float32 or not mip.is_cuda or mip.dim() != 1 or mip.numel() * 4 != nbytes):
        raise ValueError(f"texture_mip_grad: mip must be a flat CUDA float32 tensor of {nbytes // 4} elements (mip_build's layout)")
    vis_ptr = _vis_ptr(fs, vis, "texture_mip_grad")  # (before the pyramid is built: a refused call launches nothing)
    if want_guv and n_levels > 1 and mip is None:
        mip = mip_build(fs, tex, n_levels, stream)
    gtex = torch.zeros_like(tex) if want_gtex else None
    gmip = torch.zeros((nbytes // 4,), dtype=torch.float32, device=tex.device) if want_gtex and n_levels > 1 else None
    guv = torch.empty_like(uv) if want_guv else None
    fs.texture_mip_grad(vis_ptr, uv.data_ptr(), _ptr(uvd), gout.data_ptr(), tex.data_ptr(), _ptr(mip) if n_levels > 1 else None, w, h, n_ch,
                        tex_frames, abi.TEX_WRAP if wrap else abi.TEX_CLAMP, n_levels, _ptr(gtex), _ptr(gmip), _ptr(guv), abi.FUSED_CLEAR, s)
    if not fold:
        return gtex, gmip, guv
    if gmip is not None:
        fs.ctx.mip_fold(gmip.data_ptr(), nbytes, w, h, n_ch, tex_frames, n_levels, gtex.data_ptr(), s)
    return gtex, guv


class _TextureMip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv, fs, vis, uvd, wrap, n_levels, stream):
        uv = _plane(fs, uv, 2, "texture: uv")
        tex_frames, h, w, n_ch = _tex_dims(fs, tex)
        tex = tex.contiguous()
        n_levels = _mip_dims(tuple(tex.shape), n_levels)[4]
        uvd, vis_ptr = _uvd_arg(fs, uvd, n_levels), _vis_ptr(fs, vis, "texture_mip")  # (before the pyramid is built)
        mip = mip_build(fs, tex, n_levels, stream) if n_levels > 1 else None
        out = torch.empty(fs.interpolate_shape(n_ch), dtype=torch.float32, device=tex.device)
        fs.texture_mip(vis_ptr, uv.data_ptr(), _ptr(uvd), tex.data_ptr(), w, h, n_ch, tex_frames, abi.TEX_WRAP if wrap else abi.TEX_CLAMP, _ptr(mip),
                       n_levels, out.data_ptr(), fs.interpolate_bytes(n_ch), abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.wrap, ctx.n_levels, ctx.stream, ctx.uvd, ctx.mip = fs, vis, wrap, n_levels, stream, uvd, mip
        ctx.save_for_backward(tex, uv)
        return out

    @staticmethod
    def backward(ctx, gout):
        tex, uv = ctx.saved_tensors  # (one texture_mip_grad call, then its one fold into tex.grad)
        return _backward(ctx, 2, lambda *need: texture_mip_grad(ctx.fs, ctx.vis, tex, uv, ctx.uvd, gout, ctx.wrap, ctx.n_levels, ctx.mip, *need, True,
                                                                ctx.stream))


def texture_mip(fs, vis, tex, uv, uvd, wrap=False, n_levels=None, stream=None):
    """texture(fs, vis, tex, uv, wrap) with a mip pyramid: the trilinear lookup whose level each pixel takes from uvd
    [n_frames, 4, rows, W] — interpolate_deriv(fs, vis, uv_attr) of the [T, 3, 2] attribute uv came from (ux, uy, vx, vy) — by the
    piecewise-linear rule include/srz.h states; n_levels None: every level srz.mip_levels(W, H) counts; 1: texture() itself (uvd may
    be None).  The forward builds the pyramid (mip_build) and samples (FrameSet.texture_mip).  Differentiable with respect to tex
    (float atomics per level, then mip_fold: tex.grad is not bit-reproducible between runs) and to uv (deterministic); the level is
    held fixed: uvd gets no gradient.  Backward is one texture_mip_grad call that asks only for the outputs some input needs, and one
    fold when tex needs a gradient.  stream: a raw stream handle, None = torch's current stream."""
    return _TextureMip.apply(tex, uv, fs, vis, uvd, wrap, n_levels, stream)


def _cube_mip_dims(cube_shape, n_levels):
    """(tex_frames, n, n_ch, n_levels) of a cube shape [6, N, N, C] or [frames, 6, N, N, C]; n_levels None: every level there is"""
    from . import cube_mip_levels
    if len(cube_shape) not in (4, 5) or cube_shape[-4] != 6 or cube_shape[-3] != cube_shape[-2]:
        raise ValueError(f"cube_mip: a cube is [6, N, N, C] or [frames, 6, N, N, C], got {tuple(cube_shape)}")
    tex_frames = cube_shape[0] if len(cube_shape) == 5 else 1
    n, n_ch = cube_shape[-2], cube_shape[-1]
    most = cube_mip_levels(n)
    n_levels = most if n_levels is None else n_levels
    if most == 0 or not 1 <= n_levels <= most:
        raise ValueError(f"cube_mip: a cube of {n} x {n} faces has {most} levels, {n_levels} asked for")
    return tex_frames, n, n_ch, n_levels


def cube_mip_build(ctx_or_fs, cube, n_levels=None, stream=None):
    """the mip pyramid of a CUDA float32 cube [6, N, N, C] or [frames, 6, N, N, C]: the levels 1 .. n_levels - 1 (None: every level
    srz.cube_mip_levels counts) as ONE flat float32 tensor, level-major (cube_mip_views takes it apart); every face box-filtered on
    its own, deterministic (Context.cube_mip_build).  ctx_or_fs: the Context, or a FrameSet of it."""
    from . import cube_mip_bytes
    ctx = getattr(ctx_or_fs, "ctx", ctx_or_fs)
    if cube is None or cube.dtype != torch.float32 or not cube.is_cuda:
        raise ValueError("cube_mip_build: cube must be a CUDA float32 tensor" + _got(cube, "plain"))
    cube = cube.contiguous()
    tex_frames, n, n_ch, n_levels = _cube_mip_dims(tuple(cube.shape), n_levels)
    nbytes = cube_mip_bytes(n, n_ch, tex_frames, n_levels)
    mip = torch.empty((nbytes // 4,), dtype=torch.float32, device=cube.device)
    if n_levels > 1:
        ctx.cube_mip_build(cube.data_ptr(), n, n_ch, tex_frames, n_levels, mip.data_ptr(), nbytes, _stream_ptr(stream))
    return mip


def cube_mip_views(mip, cube_shape, n_levels=None):
    """the levels 1 .. n_levels - 1 of a cube's flat pyramid (cube_mip_build's, a caller's own, or a gradient pyramid) as views
    [6, n_l, n_l, C] or [frames, 6, n_l, n_l, C], in level order; cube_shape: the shape of level 0"""
    tex_frames, n, n_ch, n_levels = _cube_mip_dims(tuple(cube_shape), n_levels)
    views, off = [], 0
    for l in range(1, n_levels):
        nl = n >> l
        k = tex_frames * 6 * nl * nl * n_ch
        views.append(mip[off:off + k].view((tex_frames, 6, nl, nl, n_ch) if len(cube_shape) == 5 else (6, nl, nl, n_ch)))
        off += k
    return views


def _lam_arg(fs, lam, n_levels):
    if n_levels == 1 and lam is None:
        return None
    return _plane(fs, lam, 1, "texture_cube_mip: lam", got="")


def _cube_mip_arg(mip, n, n_ch, tex_frames, n_levels):
    from . import cube_mip_bytes
    nbytes = cube_mip_bytes(n, n_ch, tex_frames, n_levels)
    if n_levels > 1 and (mip.dtype != torch.float32 or not mip.is_cuda or mip.dim() != 1 or mip.numel() * 4 != nbytes):
        raise ValueError(f"texture_cube_mip: mip must be a flat CUDA float32 tensor of {nbytes // 4} elements (cube_mip_build's layout)")
    return mip.contiguous()


def cube_level(fs, vis, dirs, dird, n, n_levels, stream=None):
    """the level of detail of texture_cube_mip from the lookup's screen-space footprint: dirs [n_frames, 3, rows, W] and dird
    [n_frames, 6, rows, W] = interpolate_deriv(fs, vis, attr) (or interpolate_deriv_persp) of the [T, 3, 3] attribute dirs came from,
    for a cube of n x n faces with n_levels levels → lam [n_frames, 1, rows, W] float32 (FrameSet.cube_level; include/srz.h states
    the rule), zeros where nobody owns the pixel or its direction is not sampled.  Not differentiable: the footprint level is held
    fixed.  stream: a raw stream handle, None = torch's current stream."""
    dirs, dird = _plane(fs, dirs, 3, "texture_cube: dirs").detach(), _plane(fs, dird, 6, "cube_level: dird").detach()
    out = torch.empty(fs.interpolate_shape(1), dtype=torch.float32, device=dirs.device)
    fs.cube_level(_vis_ptr(fs, vis, "cube_level"), dirs.data_ptr(), dird.data_ptr(), n, n_levels, out.data_ptr(), fs.interpolate_bytes(1),
                  abi.FUSED_CLEAR, _stream_ptr(stream))
    return out


def texture_cube_mip_grad(fs, vis, cube, dirs, lam, gout, n_levels=None, mip=None, want_gtex=True, want_gdir=True, want_glam=True, fold=True,
                          stream=None):
    """the backward of texture_cube_mip(fs, vis, cube, dirs, lam, n_levels, mip) by one FrameSet.texture_cube_mip_grad call: gout
    [n_frames, C, rows, W] → (gtex, gdir, glam), each None when not wanted (not all).  gtex has cube's shape: the adds to level 0
    and, with fold (one Context.cube_mip_fold call — right for a box-built pyramid), the gradient pyramid folded into it — float
    atomics into zeros, not bit-reproducible; fold=False returns (gtex, gmip, gdir, glam) with the level-0 adds and the flat
    gradient pyramid apart: a caller-made pyramid's own gradient.  gdir [n_frames, 3, rows, W] and glam [n_frames, 1, rows, W] are
    deterministic.  mip: the pyramid the forward read (built here with cube_mip_build when gdir or glam needs it and none is
    given)."""
    if not want_gtex and not want_gdir and not want_glam:
        raise ValueError("texture_cube_mip_grad: no gradient is asked for")
    from . import cube_mip_bytes
    dirs = _plane(fs, dirs, 3, "texture_cube: dirs").detach()
    tex_frames, n, n_ch = _cube_dims(fs, cube)
    cube = cube.detach().contiguous()
    n_levels = _cube_mip_dims(tuple(cube.shape), n_levels)[3]
    lam = _lam_arg(fs, None if lam is None else lam.detach(), n_levels)
    gout = _plane(fs, gout, n_ch, "texture_cube_mip_grad: gout", "float32 {shape}")
    s = _stream_ptr(stream)
    nbytes = cube_mip_bytes(n, n_ch, tex_frames, n_levels)
    if n_levels > 1 and mip is not None:
        mip = _cube_mip_arg(mip.detach(), n, n_ch, tex_frames, n_levels)
    # (gout's home and vis after the caller's pyramid, whose check came first, and before one is built: a refused call launches nothing)
    _on_device(gout, "texture_cube_mip_grad: gout")
    vis_ptr = _vis_ptr(fs, vis, "texture_cube_mip_grad")
    if n_levels > 1 and mip is None and (want_gdir or want_glam):
        mip = cube_mip_build(fs, cube, n_levels, stream)
    gtex = torch.zeros_like(cube) if want_gtex else None
    gmip = torch.zeros((nbytes // 4,), dtype=torch.float32, device=cube.device) if want_gtex and n_levels > 1 else None
    gdir = torch.empty_like(dirs) if want_gdir else None
    glam = torch.empty(fs.interpolate_shape(1), dtype=torch.float32, device=cube.device) if want_glam else None
    fs.texture_cube_mip_grad(vis_ptr, dirs.data_ptr(), _ptr(lam), gout.data_ptr(), cube.data_ptr(), _ptr(mip) if n_levels > 1 else None, n, n_ch,
                             tex_frames, n_levels, _ptr(gtex), _ptr(gmip), _ptr(gdir), _ptr(glam), abi.FUSED_CLEAR, s)
    if not fold:
        return gtex, gmip, gdir, glam
    if gmip is not None:
        fs.ctx.cube_mip_fold(gmip.data_ptr(), nbytes, n, n_ch, tex_frames, n_levels, gtex.data_ptr(), s)
    return gtex, gdir, glam


class _TextureCubeMip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cube, dirs, lam, mip, fs, vis, n_levels, stream):
        dirs = _plane(fs, dirs, 3, "texture_cube: dirs")
        tex_frames, n, n_ch = _cube_dims(fs, cube)
        cube = cube.contiguous()
        n_levels = _cube_mip_dims(tuple(cube.shape), n_levels)[3]
        lam = _lam_arg(fs, lam, n_levels)
        own_mip = mip is not None  # the caller's pyramid: an input with a gradient of its own, no fold
        mip_ = _cube_mip_arg(mip, n, n_ch, tex_frames, n_levels) if own_mip and n_levels > 1 else None
        vis_ptr = _vis_ptr(fs, vis, "texture_cube_mip")  # (before the pyramid is built: a refused call launches nothing)
        if n_levels > 1 and not own_mip:
            mip_ = cube_mip_build(fs, cube, n_levels, stream)
        out = torch.empty(fs.interpolate_shape(n_ch), dtype=torch.float32, device=cube.device)
        fs.texture_cube_mip(vis_ptr, dirs.data_ptr(), _ptr(lam), cube.data_ptr(), n, n_ch, tex_frames, _ptr(mip_), n_levels, out.data_ptr(),
                            fs.interpolate_bytes(n_ch), abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.n_levels, ctx.stream, ctx.own_mip, ctx.mip, ctx.lam = fs, vis, n_levels, stream, own_mip, mip_, lam
        ctx.save_for_backward(cube, dirs)
        return out

    @staticmethod
    def backward(ctx, gout):
        cube, dirs = ctx.saved_tensors
        need_cube, need_dir, need_lam, need_mip = ctx.needs_input_grad[:4]
        need_lam = need_lam and ctx.lam is not None
        need_mip = need_mip and ctx.own_mip and ctx.n_levels > 1
        gtex = gmip = gdir = glam = None
        if need_cube or need_mip or need_dir or need_lam:  # one call, asking only for what is needed; the fold for a pyramid built inside
            if ctx.own_mip:
                gtex, gmip, gdir, glam = texture_cube_mip_grad(ctx.fs, ctx.vis, cube, dirs, ctx.lam, gout, ctx.n_levels, ctx.mip,
                                                               need_cube or need_mip, need_dir, need_lam, False, ctx.stream)
            else:
                gtex, gdir, glam = texture_cube_mip_grad(ctx.fs, ctx.vis, cube, dirs, ctx.lam, gout, ctx.n_levels, ctx.mip, need_cube, need_dir,
                                                         need_lam, True, ctx.stream)
        return (gtex if need_cube else None, gdir, glam, gmip if need_mip else None, None, None, None, None)


def texture_cube_mip(fs, vis, cube, dirs, lam, n_levels=None, mip=None, stream=None):
    """texture_cube(fs, vis, cube, dirs) over a mip pyramid of the cube, blended between the two levels around lam
    [n_frames, 1, rows, W] — the caller's per-pixel level of detail: a roughness scaled to levels for a prefiltered probe, or
    cube_level's footprint level — by the rule include/srz.h states; n_levels None: every level srz.cube_mip_levels(N) counts; 1:
    texture_cube itself (lam may be None).  mip None: the forward builds the box-filtered pyramid (cube_mip_build) and the backward
    folds its gradient into cube.grad; a caller's mip (cube_mip_build's layout, e.g. GGX-prefiltered levels): cube and mip are
    separate differentiable inputs, no fold.  Differentiable with respect to cube and mip (float atomics: not bit-reproducible
    between runs), to dirs and to lam (deterministic; lam's is the right-hand derivative c_(l0+1) - c_l0, zero outside
    [0, n_levels - 1)).  Backward is one texture_cube_mip_grad call that asks only for the outputs some input needs.  stream: a raw
    stream handle, None = torch's current stream."""
    return _TextureCubeMip.apply(cube, dirs, lam, mip, fs, vis, n_levels, stream)


def _prefilter_dims(cube, what):
    if cube is None or cube.dtype != torch.float32 or not cube.is_cuda or cube.dim() not in (4, 5) or cube.shape[-4] != 6 or \
            cube.shape[-3] != cube.shape[-2]:
        raise ValueError(f"{what}: a cube is a CUDA float32 tensor [6, N, N, C] or [frames, 6, N, N, C]" + _got(cube, "plain"))
    return (cube.shape[0] if cube.dim() == 5 else 1), cube.shape[-2], cube.shape[-1]


def _prefilter_call(ctx, src, n_dst, kind, roughness, cmin, dst, den, stream):
    """one Context.cube_prefilter call on contiguous tensors (dst, den: written) with scratch of its own"""
    frames, n_src, n_ch = _prefilter_dims(src, "cube_prefilter")
    nbytes = ctx.cube_prefilter_work_bytes(n_src, n_dst, n_ch, frames)
    work = torch.empty((max(nbytes, 16) // 4,), dtype=torch.float32, device=src.device)
    ctx.cube_prefilter(src.data_ptr(), n_src, dst.data_ptr(), n_dst, n_ch, frames, kind, roughness, cmin, _ptr(den), work.data_ptr(), nbytes,
                       _stream_ptr(stream))


def cube_prefilter_grad(ctx_or_fs, gdst, den, n_src, kind, roughness=1.0, cmin=0.0, stream=None, out=None):
    """the backward of cube_prefilter by one Context.cube_prefilter_grad call: gdst, the forward's output shape, and den
    [6, n_out, n_out] as the forward kept it → the gradient of the source cube, [..., 6, n_src, n_src, C] — the exact transpose as a
    gather, bit-reproducible.  out: a contiguous tensor of that shape to write instead of a fresh one."""
    ctx = getattr(ctx_or_fs, "ctx", ctx_or_fs)
    frames, n_dst, n_ch = _prefilter_dims(gdst, "cube_prefilter_grad")
    if den is None or den.dtype != torch.float32 or not den.is_cuda or tuple(den.shape) != (6, n_dst, n_dst):
        raise ValueError(f"cube_prefilter_grad: den must be a CUDA float32 tensor {(6, n_dst, n_dst)}" + _got(den, "plain"))
    gdst, den = gdst.contiguous(), den.contiguous()
    shape = tuple(gdst.shape[:-3]) + (n_src, n_src, n_ch)
    gsrc = torch.empty(shape, dtype=torch.float32, device=gdst.device) if out is None else out
    if tuple(gsrc.shape) != shape or gsrc.dtype != torch.float32 or not gsrc.is_contiguous():
        raise ValueError(f"cube_prefilter_grad: out must be a contiguous float32 tensor {shape}")
    _on_device(gsrc, "cube_prefilter_grad: out")
    nbytes = ctx.cube_prefilter_work_bytes(n_src, n_dst, n_ch, frames)
    work = torch.empty((max(nbytes, 16) // 4,), dtype=torch.float32, device=gdst.device)
    ctx.cube_prefilter_grad(gdst.data_ptr(), den.data_ptr(), n_src, n_dst, n_ch, frames, kind, roughness, cmin, gsrc.data_ptr(), work.data_ptr(),
                            nbytes, _stream_ptr(stream))
    return gsrc


class _CubePrefilter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cube, c, n_out, kind, roughness, cmin, stream):
        _, n_src, n_ch = _prefilter_dims(cube, "cube_prefilter")
        cube = cube.contiguous()
        out = torch.empty(tuple(cube.shape[:-3]) + (n_out, n_out, n_ch), dtype=torch.float32, device=cube.device)
        den = torch.empty((6, n_out, n_out), dtype=torch.float32, device=cube.device)
        _prefilter_call(c, cube, n_out, kind, roughness, cmin, out, den, stream)
        ctx.c, ctx.n_src, ctx.kind, ctx.roughness, ctx.cmin, ctx.stream, ctx.den = c, n_src, kind, roughness, cmin, stream, den
        return out

    @staticmethod
    def backward(ctx, gout):
        g = None
        if ctx.needs_input_grad[0]:
            g = cube_prefilter_grad(ctx.c, gout, ctx.den, ctx.n_src, ctx.kind, ctx.roughness, ctx.cmin, ctx.stream)
        return g, None, None, None, None, None, None


def cube_prefilter(ctx_or_fs, cube, n_out, kind, roughness=1.0, cmin=0.0, stream=None):
    """a CUDA float32 cube [6, N, N, C] or [frames, 6, N, N, C] convolved with the cosine lobe (kind abi.PREFILTER_COSINE) or the GGX
    lobe at `roughness` in [0, 1] (abi.PREFILTER_GGX) → the cube of n_out x n_out faces, every output texel the normalised sum over
    the source texels whose cosine with it exceeds cmin in [0, 1) (Context.cube_prefilter; include/srz.h states the rule).  All
    pairs, O(n_out² N²): deterministic, no atomics.  Differentiable with respect to cube — the backward is the exact transpose, one
    cube_prefilter_grad call with the normaliser the forward kept, bit-reproducible —, not to roughness or cmin.  ctx_or_fs: the
    Context, or a FrameSet of it.  stream: a raw stream handle, None = torch's current stream."""
    return _CubePrefilter.apply(cube, getattr(ctx_or_fs, "ctx", ctx_or_fs), int(n_out), int(kind), float(roughness), float(cmin), stream)


def cube_irradiance(ctx_or_fs, cube, n_out, stream=None):
    """the irradiance cube of an environment cube, n_out x n_out faces, for texture_cube by the normal: cube_prefilter with the cosine
    lobe over the whole hemisphere.  Differentiable with respect to cube."""
    return cube_prefilter(ctx_or_fs, cube, n_out, abi.PREFILTER_COSINE, 1.0, 0.0, stream)


class _OwnFrames:
    """what _lead_frames asks of a set, for an array whose frame count is its own — a cube's, not a set's: any count agrees"""

    def __init__(self, t):
        self.n_frames = t.shape[0] if t is not None and t.dim() else 0


def _cube_sh_work(ctx, n, n_ch, frames, device):
    nbytes = ctx.cube_sh_work_bytes(n, n_ch, frames)
    return torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=device), nbytes


def cube_sh_grad(ctx_or_fs, gsh, den, n, stream=None):
    """the backward of cube_sh by one Context.cube_sh_grad call: gsh [9, C] or [frames, 9, C] and den [1] as the forward kept it →
    the gradient of the source cube, [..., 6, n, n, C] — a gather per texel, bit-reproducible."""
    ctx = getattr(ctx_or_fs, "ctx", ctx_or_fs)
    frames = _lead_frames(_OwnFrames(gsh), gsh, (2, 3), "cube_sh_grad: gsh", "a CUDA float32 tensor [9, C] or [frames, 9, C]",
                          lambda t: t.shape[-2] == 9)
    _lead_frames(_OwnFrames(den), den, (1,), "cube_sh_grad: den", "a CUDA float32 tensor [1]", lambda t: t.shape[0] == 1)
    gsh, den, n_ch = gsh.contiguous(), den.contiguous(), gsh.shape[-1]
    gsrc = torch.empty(tuple(gsh.shape[:-2]) + (6, n, n, n_ch), dtype=torch.float32, device=gsh.device)
    work, nbytes = _cube_sh_work(ctx, n, n_ch, frames, gsh.device)
    ctx.cube_sh_grad(gsh.data_ptr(), den.data_ptr(), n, n_ch, frames, gsrc.data_ptr(), work.data_ptr(), nbytes, _stream_ptr(stream))
    return gsrc


class _CubeSh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cube, c, stream):
        frames, n, n_ch = _prefilter_dims(cube, "cube_sh")
        cube = cube.contiguous()
        sh = torch.empty(tuple(cube.shape[:-4]) + (9, n_ch), dtype=torch.float32, device=cube.device)
        den = torch.empty((1,), dtype=torch.float32, device=cube.device)
        work, nbytes = _cube_sh_work(c, n, n_ch, frames, cube.device)
        c.cube_sh(cube.data_ptr(), n, n_ch, frames, sh.data_ptr(), den.data_ptr(), work.data_ptr(), nbytes, _stream_ptr(stream))
        ctx.c, ctx.n, ctx.stream, ctx.den = c, n, stream, den
        return sh

    @staticmethod
    def backward(ctx, gsh):
        g = cube_sh_grad(ctx.c, gsh, ctx.den, ctx.n, ctx.stream) if ctx.needs_input_grad[0] else None
        return g, None, None


def cube_sh(ctx_or_fs, cube, stream=None):
    """a CUDA float32 cube [6, N, N, C] or [frames, 6, N, N, C], C <= abi.SH_MAX_CH, projected to its nine order-2 spherical-harmonic
    coefficients per channel → [9, C] or [frames, 9, C] (Context.cube_sh; include/srz.h states the rule): one O(N²) pass summed in a
    fixed tree, deterministic, no atomics — the environment's diffuse term without the all-pairs prefilter.  Differentiable with
    respect to cube: the backward is one cube_sh_grad call, bit-reproducible.  ctx_or_fs: the Context, or a FrameSet of it.
    stream: a raw stream handle, None = torch's current stream."""
    return _CubeSh.apply(cube, getattr(ctx_or_fs, "ctx", ctx_or_fs), stream)


_SH_KINDS = {"irradiance": abi.SH_IRRADIANCE, "radiance": abi.SH_RADIANCE}


def _sh_args(fs, sh, nrm, kind):
    """→ (sh, nrm, n_ch, sh_frames, kind), checked and contiguous"""
    nrm = _plane(fs, nrm, 3, "sh_light: nrm")
    sh_frames = _lead_frames(fs, sh, (2, 3), "sh_light: sh", "a CUDA float32 tensor [9, C] or [n_frames, 9, C]", lambda t: t.shape[-2] == 9)
    return sh.contiguous(), nrm, sh.shape[-1], sh_frames, _SH_KINDS.get(kind, len(_SH_KINDS))  # (an unknown kind is the library's to refuse)


def sh_light_grad(fs, vis, sh, nrm, gout, kind="irradiance", want_gsh=True, want_gnrm=True, stream=None):
    """the backward of sh_light by one FrameSet.sh_grad call: gout [n_frames, C, rows, W] → (gsh, gnrm), each None when not wanted
    (not both: the library refuses that): gnrm is deterministic, zeros where nobody owns the pixel or its normal is not lit; gsh has sh's shape, reduced in a
    fixed tree (bit-reproducible for a shard layout).  stream: a raw stream handle, None = torch's current stream."""
    sh, nrm, n_ch, sh_frames, k = _sh_args(fs, sh, nrm, kind)
    gout = _gout(fs, gout, n_ch, "sh_light_grad")
    gnrm = torch.empty_like(nrm) if want_gnrm else None
    work_bytes = fs.sh_work_bytes(n_ch) if want_gsh else 0
    gsh, work = _reduced(sh, work_bytes) if want_gsh else (None, None)
    fs.sh_grad(_vis_ptr(fs, vis, "sh_light_grad"), nrm.data_ptr(), sh.data_ptr(), n_ch, sh_frames, k, gout.data_ptr(), _ptr(gnrm), _ptr(gsh),
               _ptr(work), work_bytes, abi.FUSED_CLEAR, _stream_ptr(stream))
    return gsh, gnrm


class _ShLight(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sh, nrm, fs, vis, kind, stream):
        sh, nrm, n_ch, sh_frames, k = _sh_args(fs, sh, nrm, kind)
        out = torch.empty(fs.interpolate_shape(n_ch), dtype=torch.float32, device=nrm.device)
        fs.sh(_vis_ptr(fs, vis, "sh_light"), nrm.data_ptr(), sh.data_ptr(), n_ch, sh_frames, k, out.data_ptr(), fs.interpolate_bytes(n_ch),
              abi.FUSED_CLEAR, _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.kind, ctx.stream = fs, vis, kind, stream
        ctx.save_for_backward(sh, nrm)
        return out

    @staticmethod
    def backward(ctx, gout):
        sh, nrm = ctx.saved_tensors
        return _backward(ctx, 2, lambda *need: sh_light_grad(ctx.fs, ctx.vis, sh, nrm, gout, ctx.kind, *need, ctx.stream))


def sh_light(fs, vis, sh, nrm, kind="irradiance", stream=None):
    """nine order-2 spherical-harmonic coefficients per channel evaluated at each pixel's normal under a visibility buffer `vis` of
    FrameSet `fs`: sh is [9, C] (every frame shares it) or [n_frames, 9, C] CUDA float32, C <= abi.SH_MAX_CH — cube_sh's output, a
    captured probe, or a learned parameter —, nrm [n_frames, 3, rows, W] of any length → [n_frames, C, rows, W] float32, unclamped:
    kind "irradiance", the cosine-convolved environment over pi, a drop-in for texture_cube(cube_irradiance(env, m), nrm) as ibl's
    `irr`; kind "radiance", the function itself.  Zeros where nobody owns the pixel or its normal has no finite positive length
    (FrameSet.sh; include/srz.h states the rule).  Differentiable with respect to sh (sums over the pixels in a fixed tree:
    bit-reproducible) and nrm (deterministic planes), not to kind.  Backward is one sh_light_grad call that asks only for the
    outputs some input needs.  stream: a raw stream handle, None = torch's current stream."""
    return _ShLight.apply(sh, nrm, fs, vis, kind, stream)


class _CubePrefilterPyramid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cube, c, roughness, cmin, stream):
        _prefilter_dims(cube, "cube_prefilter_pyramid")
        cube = cube.contiguous()
        L = len(roughness) + 1
        box = cube_mip_build(c, cube, L, stream)
        mip, dens = torch.empty_like(box), []
        for r, src, dst in zip(roughness, cube_mip_views(box, cube.shape, L), cube_mip_views(mip, cube.shape, L)):
            dens.append(torch.empty((6, src.shape[-2], src.shape[-2]), dtype=torch.float32, device=cube.device))
            _prefilter_call(c, src, src.shape[-2], abi.PREFILTER_GGX, r, cmin, dst, dens[-1], stream)
        ctx.c, ctx.roughness, ctx.cmin, ctx.stream, ctx.dens, ctx.shape = c, roughness, cmin, stream, dens, tuple(cube.shape)
        return mip

    @staticmethod
    def backward(ctx, gmip):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        from . import cube_mip_bytes
        gmip = gmip.contiguous()
        L = len(ctx.roughness) + 1
        gbox = torch.empty_like(gmip)  # the gradient of the box pyramid: every level written by its own prefilter_grad call
        for r, den, g, out in zip(ctx.roughness, ctx.dens, cube_mip_views(gmip, ctx.shape, L), cube_mip_views(gbox, ctx.shape, L)):
            cube_prefilter_grad(ctx.c, g, den, g.shape[-2], abi.PREFILTER_GGX, r, ctx.cmin, ctx.stream, out=out)
        gcube = torch.zeros(ctx.shape, dtype=torch.float32, device=gmip.device)
        tex_frames, n, n_ch, _ = _cube_mip_dims(ctx.shape, L)
        if L > 1:
            ctx.c.cube_mip_fold(gbox.data_ptr(), cube_mip_bytes(n, n_ch, tex_frames, L), n, n_ch, tex_frames, L, gcube.data_ptr(), _stream_ptr(ctx.stream))
        return gcube, None, None, None, None


def cube_prefilter_pyramid(ctx_or_fs, cube, roughness, cmin=0.0, stream=None):
    """the GGX-prefiltered levels 1 .. L - 1 of an environment cube [6, N, N, C] or [frames, 6, N, N, C] as ONE flat float32 tensor in
    cube_mip_build's layout, to pass as texture_cube_mip(..., mip=): roughness is a sequence, one value per level (L = len + 1 levels,
    at most srz.cube_mip_levels(N)); level l is cube_prefilter's GGX lobe at roughness[l - 1] of the BOX level l (cube_mip_build's),
    same size in and out.  Level 0 stays the cube itself.  One differentiable step with respect to cube: the backward runs
    cube_prefilter_grad per level into a gradient pyramid and folds it into cube.grad (cube_mip_fold); deterministic."""
    return _CubePrefilterPyramid.apply(cube, getattr(ctx_or_fs, "ctx", ctx_or_fs), tuple(float(r) for r in roughness), float(cmin), stream)


def _scene_draws(fs):
    """per frame of a sceneset the mesh slots of its draws, in draw order"""
    if not all(isinstance(f, abi.SceneFrame) for f in fs.frames):
        raise ValueError("the set is not a sceneset")
    return [[int(f._draws[i].mesh_id) for i in range(f.c.n_draws)] for f in fs.frames]


def _set_tris(fs, pos_tris):
    """pos_tris, or the largest triangle count of the set's frames (a sceneset: from the face counts of the slots it draws)"""
    if pos_tris is not None:
        return int(pos_tris)
    if all(hasattr(f, "n_tris") for f in fs.frames):
        return max(f.n_tris for f in fs.frames)
    return max(sum(fs.ctx.mesh_sizes[m][1] for m in draws) for draws in _scene_draws(fs))


def positions(fs, pos_tris=None, stream=None):
    """the screen positions of FrameSet `fs`'s triangles as the rasteriser reads them (FrameSet.positions; a sceneset runs its vertex
    stage) → [n_frames, T, 3, 3] float32 (triangle, corner, (x, y, z)), T = pos_tris (default: the largest triangle count of the
    set's frames), zeros behind a frame's last triangle.  stream: a raw stream handle, None = torch's current stream."""
    T = _set_tris(fs, pos_tris)
    pos = torch.empty((fs.n_frames, T, 3, 3), dtype=torch.float32, device="cuda")
    fs.positions(T, pos.data_ptr(), pos.numel() * 4, _stream_ptr(stream))
    return pos


def vertex_grad(fs, mesh_id, gpos, want_gverts=True, want_gdraw=True, stream=None, gdraw=None):
    """the backward of sceneset `fs`'s vertex stage for mesh slot mesh_id by one FrameSet.vertex_grad call: gpos [n_frames, T, 3, 3]
    (position_grad's, antialias_grad's, or their sum) → (gverts [n_frames, V, 3], gdraw [n_frames, D, 18]), each None when not wanted
    (not both), into zeros; D the largest draw count of the set's frames.  gverts is the gradient with respect to the slot's vertex
    positions, frame by frame — a gather, bit-reproducible; a row of gdraw is the gradient of a draw's ndc_mvp (16, its own
    column-major order), zscale and zoffset, zeros for draws of other slots — float atomics, not bit-reproducible.  gdraw: a
    [n_frames, D, 18] tensor to add into instead (several meshes into one buffer)."""
    if not want_gverts and not want_gdraw:
        raise ValueError("vertex_grad: neither gverts nor gdraw is asked for")
    if gpos is None or gpos.dtype != torch.float32 or not gpos.is_cuda or gpos.dim() != 4 or gpos.shape[0] != fs.n_frames or \
            tuple(gpos.shape[2:]) != (3, 3):
        raise ValueError("vertex_grad: gpos must be a CUDA float32 tensor [n_frames, T, 3, 3]" + _got(gpos, "plain"))
    gpos = gpos.contiguous()
    D = max(1, max(len(d) for d in _scene_draws(fs)))
    gverts = torch.zeros((fs.n_frames, fs.ctx.mesh_sizes[mesh_id][0], 3), dtype=torch.float32, device=gpos.device) if want_gverts else None
    if want_gdraw and gdraw is None:
        gdraw = torch.zeros((fs.n_frames, D, 18), dtype=torch.float32, device=gpos.device)
    if want_gdraw and (gdraw.dtype != torch.float32 or not gdraw.is_contiguous() or tuple(gdraw.shape) != (fs.n_frames, D, 18)):
        raise ValueError(f"vertex_grad: gdraw must be a contiguous float32 tensor {(fs.n_frames, D, 18)}")
    if want_gdraw:
        _on_device(gdraw, "vertex_grad: gdraw")
    fs.vertex_grad(mesh_id, gpos.data_ptr(), gpos.shape[1], _ptr(gverts), gdraw.data_ptr() if want_gdraw else None, D, _stream_ptr(stream))
    return gverts, (gdraw if want_gdraw else None)


def mesh_update(ctx, mesh_id, verts8, stream=None):
    """new vertices for mesh slot mesh_id of Context `ctx`, in place, from a CUDA float32 tensor [V, 8] (pos3 nrm3 uv2; V the slot's
    count): Context.mesh_update, one device-to-device copy.  Every sceneset that draws the slot stays valid and renders the new
    vertices from its next vertex stage on.  stream: a raw stream handle, None = torch's current stream."""
    if verts8 is None or verts8.dtype != torch.float32 or not verts8.is_cuda or verts8.dim() != 2 or verts8.shape[1] != 8:
        raise ValueError("mesh_update: verts8 must be a CUDA float32 tensor [V, 8]" + _got(verts8, "plain"))
    verts8 = verts8.detach().contiguous()
    ctx.mesh_update(mesh_id, verts8.data_ptr(), verts8.shape[0], _stream_ptr(stream))


class _ScenePositions(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fs, mesh_ids, pos_tris, stream, mvp, zmap, *verts):
        ctx.fs, ctx.mesh_ids, ctx.stream = fs, mesh_ids, stream
        ctx.shapes = [tuple(v.shape) for v in verts]
        return positions(fs, pos_tris, stream)

    @staticmethod
    def backward(ctx, gpos):
        fs = ctx.fs
        need_draw = ctx.needs_input_grad[4] or ctx.needs_input_grad[5]
        need_verts = {m: ctx.needs_input_grad[6 + i] for i, m in enumerate(ctx.mesh_ids)}
        # one call per mesh that needs a gradient (for the matrices: every mesh the set draws), sharing one gdraw buffer
        todo = sorted({m for draws in _scene_draws(fs) for m in draws} if need_draw else {m for m, need in need_verts.items() if need})
        gpos = gpos.contiguous()
        gdraw, gverts = None, {}
        for m in todo:
            gverts[m], gdraw = vertex_grad(fs, m, gpos, need_verts.get(m, False), need_draw, ctx.stream, gdraw)
        out = []
        for m, shape in zip(ctx.mesh_ids, ctx.shapes):
            g = gverts.get(m)
            out.append(None if g is None else (g.sum(0) if len(shape) == 2 else g))
        gmvp = gdraw[:, :, :16].contiguous() if ctx.needs_input_grad[4] else None
        gzmap = gdraw[:, :, 16:].contiguous() if ctx.needs_input_grad[5] else None
        return (None, None, None, None, gmvp, gzmap, *out)


def scene_positions(fs, meshes, mvp=None, zmap=None, pos_tris=None, stream=None):
    """the screen positions of sceneset `fs`'s triangles, positions(fs), as a differentiable function of what the set was made from —
    the `pos` that interpolate_geo, depth and antialias take, and where the chain begins.  meshes: a dict mesh slot → vertex positions,
    a CUDA float32 tensor [V, 3] (shared by the frames) or [n_frames, V, 3]; mvp: [n_frames, D, 16], every draw's ndc_mvp in its own
    column-major order (D the largest draw count of the frames); zmap: [n_frames, D, 2], (zscale, zoffset) of the draw's frame.  LIKE
    THE `pos` HANDLE THESE TENSORS ARE GRAPH HANDLES WHOSE VALUES ARE NEVER READ: the positions are the set's own (its vertex stage
    over what srz_mesh_upload / mesh_update and srz_sceneset_create / _update gave it), and the caller warrants that the tensors hold
    the same values.  The forward returns real values: positions(fs).  Backward: one vertex_grad call per mesh that needs a gradient
    (with mvp or zmap: per mesh the set draws), sharing one gdraw buffer; a [V, 3] tensor's gradient is the per-frame result summed
    over the frames (deterministic); mvp.grad and zmap.grad are the first 16 and the last 2 columns of gdraw (float atomics: not
    bit-reproducible), rows behind a frame's last draw zero.  A frame's zscale and zoffset are shared by its draws: sum zmap.grad
    over them.  antialias(fs, vis, interpolate_geo(fs, vis, attr, pos), pos) with pos = scene_positions(...) is the whole chain from a
    loss to the mesh and the pose."""
    ids = tuple(sorted(meshes))
    D = max(1, max(len(d) for d in _scene_draws(fs)))
    for m in ids:
        v = meshes[m]
        V = fs.ctx.mesh_sizes[m][0]
        if v.dtype != torch.float32 or tuple(v.shape) not in ((V, 3), (fs.n_frames, V, 3)):
            raise ValueError(f"scene_positions: mesh {m} must be float32 [{V}, 3] or [{fs.n_frames}, {V}, 3], got {tuple(v.shape)} {v.dtype}")
    if mvp is not None and (mvp.dtype != torch.float32 or tuple(mvp.shape) != (fs.n_frames, D, 16)):
        raise ValueError(f"scene_positions: mvp must be float32 {(fs.n_frames, D, 16)}, got {tuple(mvp.shape)} {mvp.dtype}")
    if zmap is not None and (zmap.dtype != torch.float32 or tuple(zmap.shape) != (fs.n_frames, D, 2)):
        raise ValueError(f"scene_positions: zmap must be float32 {(fs.n_frames, D, 2)}, got {tuple(zmap.shape)} {zmap.dtype}")
    return _ScenePositions.apply(fs, ids, pos_tris, stream, mvp, zmap, *[meshes[m] for m in ids])


# ------------------------------------------------------------------------------------------------ normals and per-vertex attributes
def _sets_arg(ctx, slot, t, name, who="mesh_normals", channels=3, batched=True):
    """a CUDA float32 per-vertex tensor for mesh slot `slot`, [V, C] or (batched) [B, V, C] with B <= 65535 -> (the tensor detached
    and contiguous, number of sets).  channels: the C asked for (3: positions, the default), None = a field of 1 .. abi.LAP_MAX_CH
    channels; batched False: [V, C] only (one set shared by the sets, as wpos is); who: the function the refusal names.  The ONE
    refusal of the mesh passes' tensors: its text says the form that was asked for"""
    V = ctx.mesh_sizes[slot][0]
    ok = t is not None and t.dtype == torch.float32 and t.is_cuda and t.dim() in ((2, 3) if batched else (2,))
    ok = ok and t.shape[-2] == V and (t.shape[-1] == channels if channels else 1 <= t.shape[-1] <= abi.LAP_MAX_CH)
    ok = ok and (t.dim() == 2 or 1 <= t.shape[0] <= 65535)
    if not ok:
        C_, cap = (channels, "") if channels else ("C", f"C 1 .. {abi.LAP_MAX_CH}, ")
        form = f"[{V}, {C_}] or [B, {V}, {C_}] ({cap}B <= 65535)" if batched else f"[{V}, {C_}]"
        raise ValueError(f"{who}: {name} must be a CUDA float32 tensor {form}" + _got(t, "plain"))
    return t.detach().contiguous(), (t.shape[0] if t.dim() == 3 else 1)


class _MeshNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, sctx, slot, stream):
        p, n_sets = _sets_arg(sctx, slot, pos, "pos")
        nrm = torch.empty_like(p)
        sctx.mesh_normals(slot, p.data_ptr(), 3, n_sets, nrm.data_ptr(), 3, _stream_ptr(stream))
        ctx.sctx, ctx.slot, ctx.stream, ctx.n_sets = sctx, slot, stream, n_sets
        ctx.save_for_backward(p)
        return nrm

    @staticmethod
    def backward(ctx, gnrm):
        (p,) = ctx.saved_tensors
        gnrm = gnrm.contiguous()
        work, gpos = torch.empty_like(p), torch.empty_like(p)
        ctx.sctx.mesh_normals_grad(ctx.slot, p.data_ptr(), 3, ctx.n_sets, gnrm.data_ptr(), 3, work.data_ptr(), gpos.data_ptr(),
                                   _stream_ptr(ctx.stream))
        return gpos, None, None, None


def mesh_normals(ctx, slot, pos, stream=None):
    """the area-weighted vertex normals of mesh slot `slot` of Context `ctx` at vertex positions pos, a CUDA float32 tensor [V, 3] or
    [B, V, 3] (B sets of positions over the slot's face list, one call) → the same shape: per vertex the sum of cross(p1 - p0, p2 - p0)
    over the faces that name it, normalised; zeros for a vertex no face names and for a sum that is zero or not finite
    (Context.mesh_normals, include/srz.h states the rule).  Differentiable with respect to pos (Context.mesh_normals_grad).  Both
    directions are gathers without atomics: the values and pos.grad are bit-reproducible.  The slot's own vertices are neither read
    nor written: refresh_normals is the in-place form.  stream: a raw stream handle, None = torch's current stream."""
    return _MeshNormals.apply(pos, ctx, slot, stream)


class _MeshTangents(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, sctx, slot, uv, stream):
        p, n_sets = _sets_arg(sctx, slot, pos, "pos")
        V = p.shape[-2]
        if uv is not None:
            if uv.dtype != torch.float32 or not uv.is_cuda or tuple(uv.shape) != (V, 2):
                raise ValueError(f"mesh_tangents: uv must be a CUDA float32 tensor [{V}, 2], got {tuple(uv.shape)} {uv.dtype}")
            uv = uv.detach().contiguous()
        tan = torch.empty(p.shape[:-1] + (4,), dtype=torch.float32, device=p.device)
        sctx.mesh_tangents(slot, p.data_ptr(), 3, n_sets, _ptr(uv), 2, tan.data_ptr(), 4, _stream_ptr(stream))
        ctx.sctx, ctx.slot, ctx.stream, ctx.n_sets, ctx.uv = sctx, slot, stream, n_sets, uv
        ctx.save_for_backward(p)
        return tan

    @staticmethod
    def backward(ctx, gtan):
        (p,) = ctx.saved_tensors
        gtan = gtan.contiguous()
        work, gpos = torch.empty_like(p), torch.empty_like(p)
        ctx.sctx.mesh_tangents_grad(ctx.slot, p.data_ptr(), 3, ctx.n_sets, _ptr(ctx.uv), 2, gtan.data_ptr(), 4, work.data_ptr(), gpos.data_ptr(),
                                    _stream_ptr(ctx.stream))
        return gpos, None, None, None, None


def mesh_tangents(ctx, slot, pos, uv=None, stream=None):
    """the uv-area-weighted vertex tangents and handedness of mesh slot `slot` of Context `ctx` at vertex positions pos, a CUDA float32
    tensor [V, 3] or [B, V, 3] → [V, 4] or [B, V, 4]: per vertex the unit tangent (along +u, mirrored uv or not) and w = +-1, so that
    w * cross(normal, tangent) points along +v; a zero tangent for a vertex no face names and for a sum that is zero or not finite
    (Context.mesh_tangents, include/srz.h states the rule).  uv: a CUDA float32 tensor [V, 2] shared by the B sets, None = the slot's
    own uv.  Differentiable with respect to pos only (Context.mesh_tangents_grad; uv and w are held).  Both directions are gathers
    without atomics: the values and pos.grad are bit-reproducible.  The 4-channel result is a corner_attr attribute:
    interpolate(fs, vis, corner_attr(fs, {slot: mesh_tangents(ctx, slot, verts)})) is normal_map's tan.  stream: a raw stream handle,
    None = torch's current stream."""
    return _MeshTangents.apply(pos, ctx, slot, uv, stream)


_LAP_KINDS = {"umbrella": abi.LAP_UMBRELLA, "graph": abi.LAP_GRAPH, "cotan": abi.LAP_COTAN}


def _lap_args(ctx, slot, x, name, kind, wpos, who):
    """the arguments of mesh_laplacian and mesh_solve, all through _sets_arg -> (the field detached and contiguous, number of sets,
    channels, SRZ_LAP_* of the kind's name — -1 for a name that is none: the library's to refuse —, wpos detached and contiguous or
    None)"""
    t, n_sets = _sets_arg(ctx, slot, x, name, who, None)
    if wpos is not None:
        wpos, _ = _sets_arg(ctx, slot, wpos, "wpos", who, 3, False)
    return t, n_sets, t.shape[-1], _LAP_KINDS.get(kind, -1) if isinstance(kind, str) else -1, wpos


def _lap_call(call, slot, t, n_sets, n_ch, kind, wpos, stream):
    """one plain call (Context.mesh_laplacian or its _grad) over the packed field t -> a new tensor of t's shape"""
    out = torch.empty_like(t)
    call(slot, t.data_ptr(), n_ch, n_ch, n_sets, kind, _ptr(wpos), 3, out.data_ptr(), n_ch, _stream_ptr(stream))
    return out


class _MeshLaplacian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sctx, slot, kind, wpos, stream):
        t, n_sets, n_ch, k, wpos = _lap_args(sctx, slot, x, "x", kind, wpos, "mesh_laplacian")
        ctx.sctx, ctx.slot, ctx.kind, ctx.wpos, ctx.stream, ctx.dims = sctx, slot, k, wpos, stream, (n_sets, n_ch)
        return _lap_call(sctx.mesh_laplacian, slot, t, n_sets, n_ch, k, wpos, stream)

    @staticmethod
    def backward(ctx, gout):
        gx = _lap_call(ctx.sctx.mesh_laplacian_grad, ctx.slot, gout.contiguous(), *ctx.dims, ctx.kind, ctx.wpos, ctx.stream)
        return gx, None, None, None, None, None


def mesh_laplacian(ctx, slot, x, kind="umbrella", wpos=None, stream=None):
    """the mesh Laplacian of mesh slot `slot` of Context `ctx` over the per-vertex field x, a CUDA float32 tensor [V, C] or [B, V, C]
    (C 1 .. 64 channels, B fields over the slot's connectivity in one call) → the same shape.  kind: "umbrella" (x[v] minus the mean
    of its neighbours, a neighbour counted once per face it shares with v), "graph" (n x[v] minus their sum: symmetric, positive
    semidefinite) or "cotan" (cotangent weights made from wpos, a CUDA float32 tensor [V, 3] shared by the B fields and HELD — None
    = the slot's own positions; a zero-area face is skipped).  Context.mesh_laplacian, include/srz.h states the rule.
    Differentiable with respect to x only (Context.mesh_laplacian_grad, the exact transpose; wpos is held as mesh_tangents holds
    uv).  Both directions are gathers without atomics: the values and x.grad are bit-reproducible.  The regulariser of the mesh
    side:
      reg   = (mesh_laplacian(ctx, slot, verts) ** 2).sum()                  # penalty
      verts = mesh_solve(ctx, slot, u, 10.0); ... loss(verts).backward()     # u.grad is the diffused gradient
    stream: a raw stream handle, None = torch's current stream."""
    return _MeshLaplacian.apply(x, ctx, slot, kind, wpos, stream)


def _cg(apply, b, iters, tol):
    """conjugate gradients in torch ops from a zero start: `apply` is a symmetric positive definite operator on tensors of b's
    shape (the whole tensor is ONE vector: the sums run over every element) -> u with apply(u) ~ b.  `apply` is called once per
    iteration and nowhere else.  tol None: exactly `iters` iterations and nothing read back — a zero p . Ap (or a zero r . r)
    gives a zero step through torch.where, never a division by zero.  tol: stops before an iteration once the recursive residual
    |r| is at most tol |b| (one scalar read back per iteration), after `iters` at the latest."""
    u, r = torch.zeros_like(b), b.clone()
    p, rr = r.clone(), (r * r).sum()
    zero, one = torch.zeros_like(rr), torch.ones_like(rr)
    stop = None if tol is None else rr * (float(tol) * float(tol))

    def ratio(num, den):
        ok = den != 0
        return torch.where(ok, num / torch.where(ok, den, one), zero)
    for _ in range(iters):
        if stop is not None and bool(rr <= stop):
            break
        Ap = apply(p)
        alpha = ratio(rr, (p * Ap).sum())
        u, r = u + alpha * p, r - alpha * Ap
        rr_new = (r * r).sum()
        p, rr = r + ratio(rr_new, rr) * p, rr_new
    return u


class _MeshSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, b, sctx, slot, lam, kind, wpos, iters, tol, stream):
        if kind not in ("graph", "cotan"):
            raise NotImplementedError(f"mesh_solve: conjugate gradients need a symmetric operator: kind must be 'graph' or 'cotan', got {kind!r}")
        t, n_sets, n_ch, k, wpos = _lap_args(sctx, slot, b, "b", kind, wpos, "mesh_solve")
        lam, iters = float(lam), int(iters)
        ctx.args = (sctx, slot, lam, kind, wpos, iters, tol, stream)
        # (sctx.mesh_laplacian is looked up per application: the plain call, once per iteration.  A raw handle is made torch's
        # current stream for the loop, so that its torch ops and the operator's launches are in ONE stream's order)
        with contextlib.nullcontext() if stream is None else torch.cuda.stream(torch.cuda.ExternalStream(stream)):
            return _cg(lambda p: p + lam * _lap_call(sctx.mesh_laplacian, slot, p.contiguous(), n_sets, n_ch, k, wpos, stream), t, iters, tol)

    @staticmethod
    def backward(ctx, gu):
        return (_MeshSolve.apply(gu.contiguous(), *ctx.args),) + (None,) * 8


def mesh_solve(ctx, slot, b, lam, kind="graph", wpos=None, iters=64, tol=None, stream=None):
    """u with (I + lam L) u = b, L = mesh_laplacian of mesh slot `slot` in one of its two SYMMETRIC kinds ("graph", "cotan";
    "umbrella" raises), lam >= 0; b: a CUDA float32 tensor [V, C] or [B, V, C] → the same shape.  The "large steps"
    reparameterisation of a mesh fit: optimise u, render verts = mesh_solve(ctx, slot, u, lam), and u.grad is the image gradient
    DIFFUSED over the surface instead of a penalty on the result:
      reg   = (mesh_laplacian(ctx, slot, verts) ** 2).sum()                  # penalty
      verts = mesh_solve(ctx, slot, u, 10.0); ... loss(verts).backward()     # u.grad is the diffused gradient
    Conjugate gradients in torch ops on the device over the plain Context.mesh_laplacian call, from a zero start, the whole of b one
    vector.  tol None: exactly `iters` iterations (as many applications of the operator) and no device-to-host read; a zero p . Ap
    gives a zero step, never a division by zero.  tol: stops once the recursive residual is at most tol |b| (one scalar read back
    per iteration), after `iters` at the latest.  The matrix is symmetric, so the backward is mesh_solve of the incoming gradient
    with the same arguments; wpos (cotan: a CUDA float32 [V, 3], None = the slot's own positions) is held.  stream: a raw stream
    handle, None = torch's current stream; the whole solve — the loop's torch ops and the operator's launches — runs on it (a handle
    is made torch's current stream for the duration), and ordering b before it and the result after it is the caller's, as for every
    pass."""
    return _MeshSolve.apply(b, ctx, slot, lam, kind, wpos, iters, tol, stream)


def _face_field(ctx, slot, sets):
    """an uninitialised CUDA float32 tensor sets + [F, 3] for mesh slot `slot` (never without an address: a slot with no faces is not
    an error, a null output is)"""
    F = ctx.mesh_sizes[slot][1]
    return torch.empty(tuple(sets) + (max(F, 1), 3), dtype=torch.float32, device="cuda")[..., :F, :]


def mesh_edge_counts(ctx, slot, stream=None):
    """the number of faces on every edge of mesh slot `slot` of Context `ctx` → a CUDA float32 tensor [F, 3], edge j of a face opposite
    its corner j: 1 a boundary edge, 2 a manifold edge, more a non-manifold one (Context.mesh_edges with abi.EDGE_COUNT; the
    adjacency is found from the slot's corner lists, include/srz.h states the rule).  It reads no positions and carries no gradient:
    the weight 1 / count that makes every undirected edge count once, and the boundary's mark.  stream: a raw stream handle, None =
    torch's current stream."""
    out = _face_field(ctx, slot, ())
    ctx.mesh_edges(slot, None, 8, 1, abi.EDGE_COUNT, out.data_ptr(), 3, _stream_ptr(stream))
    return out


class _MeshEdges(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, sctx, slot, kind, who, stream):
        p, n_sets = _sets_arg(sctx, slot, pos, "pos", who)
        out = _face_field(sctx, slot, p.shape[:-2])
        sctx.mesh_edges(slot, p.data_ptr(), 3, n_sets, kind, out.data_ptr(), 3, _stream_ptr(stream))
        ctx.sctx, ctx.slot, ctx.kind, ctx.stream, ctx.n_sets = sctx, slot, kind, stream, n_sets
        ctx.save_for_backward(p)
        return out

    @staticmethod
    def backward(ctx, gout):
        (p,) = ctx.saved_tensors
        gout = gout.contiguous()
        work = torch.empty_like(gout) if ctx.kind == abi.EDGE_DIHEDRAL else None
        gpos = torch.empty_like(p)
        ctx.sctx.mesh_edges_grad(ctx.slot, p.data_ptr(), 3, ctx.n_sets, ctx.kind, gout.data_ptr(), 3, _ptr(work), gpos.data_ptr(),
                                 _stream_ptr(ctx.stream))
        return gpos, None, None, None, None, None


def mesh_edge_lengths(ctx, slot, pos, stream=None):
    """the edge lengths of mesh slot `slot` of Context `ctx` at vertex positions pos, a CUDA float32 tensor [V, 3] or [B, V, 3] → [F, 3]
    or [B, F, 3]: edge j of a face (i0, i1, i2) lies opposite corner j and joins i[(j + 1) % 3] and i[(j + 2) % 3]
    (Context.mesh_edges with abi.EDGE_LENGTH, include/srz.h states the rule).  An interior edge appears once per face on it:
    weight by 1 / mesh_edge_counts to count every undirected edge once (mesh_edge_loss does).  Differentiable with respect to pos
    (Context.mesh_edges_grad; an edge of zero length passes no gradient on).  Both directions are gathers without atomics: the
    values and pos.grad are bit-reproducible.  stream: a raw stream handle, None = torch's current stream."""
    return _MeshEdges.apply(pos, ctx, slot, abi.EDGE_LENGTH, "mesh_edge_lengths", stream)


def mesh_normal_consistency(ctx, slot, pos, stream=None):
    """the normal consistency of mesh slot `slot` of Context `ctx` at vertex positions pos, a CUDA float32 tensor [V, 3] or [B, V, 3] →
    [F, 3] or [B, F, 3]: per face and edge the sum, over the faces across the edge, of 1 - cos of the two unit face normals — 0 flat, 2
    folded back or wound against each other, +0 on a boundary edge and on a face of zero area, which is skipped, never multiplied by
    zero (Context.mesh_edges with abi.EDGE_DIHEDRAL; the faces across an edge are found from the slot's corner lists, include/srz.h
    states the rule).  A pair of faces appears at both: the sum over the result counts it twice (mesh_normal_loss takes the mean).
    Differentiable with respect to pos (Context.mesh_edges_grad).  Both directions are gathers without atomics: the values and
    pos.grad are bit-reproducible.  stream: a raw stream handle, None = torch's current stream."""
    return _MeshEdges.apply(pos, ctx, slot, abi.EDGE_DIHEDRAL, "mesh_normal_consistency", stream)


def mesh_edge_loss(ctx, slot, pos, target=0.0, stream=None):
    """the mean over the UNDIRECTED edges of mesh slot `slot` of (length - target)^2, a scalar (per set of a [B, V, 3] pos: [B]): plain
    torch ops over mesh_edge_lengths weighted by 1 / mesh_edge_counts, so that an edge counts once however many faces share it.
    Keeps triangles from collapsing or stretching; differentiable with respect to pos."""
    w = 1.0 / mesh_edge_counts(ctx, slot, stream)
    d = mesh_edge_lengths(ctx, slot, pos, stream) - target
    return (w * d * d).sum((-2, -1)) / w.sum().clamp(min=1.0)


def mesh_normal_loss(ctx, slot, pos, stream=None):
    """the mean over the adjacent face pairs of mesh slot `slot` of 1 - cos of their normals, a scalar (per set of a [B, V, 3] pos:
    [B]): plain torch ops over mesh_normal_consistency — its sum counts every pair at both faces, and so does the divisor, the sum
    of mesh_edge_counts - 1.  Keeps a surface from creasing; differentiable with respect to pos."""
    pairs = (mesh_edge_counts(ctx, slot, stream) - 1.0).sum()
    return mesh_normal_consistency(ctx, slot, pos, stream).sum((-2, -1)) / pairs.clamp(min=1.0)


def refresh_normals(ctx, slot, stream=None):
    """the nrm fields of mesh slot `slot` recomputed IN PLACE from the positions the slot holds (Context.mesh_normals with both
    pointers null): the call that follows mesh_update on the same stream, so that shade_visibility, gbuffer(NORMAL) and the colour
    render of every sceneset that draws the slot see the normals of the moved mesh.  stream: a raw stream handle, None = torch's
    current stream."""
    ctx.mesh_normals(slot, None, 8, 1, None, 8, _stream_ptr(stream))


class _CornerAttr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fs, slots, pos_tris, stream, *attrs):
        T = _set_tris(fs, pos_tris)
        C_ = attrs[0].shape[-1]
        out = torch.zeros((fs.n_frames, T, 3, C_), dtype=torch.float32, device=attrs[0].device)
        for slot, a in zip(slots, attrs):
            a = a.detach().contiguous()
            fs.corner_attr(slot, a.data_ptr(), C_, a.shape[0] if a.dim() == 3 else 1, out.data_ptr(), T, _stream_ptr(stream))
        ctx.fs, ctx.slots, ctx.stream, ctx.T = fs, slots, stream, T
        ctx.shapes = [tuple(a.shape) for a in attrs]
        return out

    @staticmethod
    def backward(ctx, gout):
        fs = ctx.fs
        gout = gout.contiguous()
        grads = []
        for i, (slot, shape) in enumerate(zip(ctx.slots, ctx.shapes)):
            if not ctx.needs_input_grad[4 + i]:
                grads.append(None)
                continue
            g = torch.empty((fs.n_frames, shape[-2], shape[-1]), dtype=torch.float32, device=gout.device)
            fs.corner_attr_grad(slot, gout.data_ptr(), shape[-1], g.data_ptr(), ctx.T, _stream_ptr(ctx.stream))
            grads.append(g.sum(0) if len(shape) == 2 else g)
        return (None, None, None, None, *grads)


def corner_attr(fs, attrs, pos_tris=None, stream=None):
    """per-vertex attributes laid out as sceneset `fs`'s triangle stream — what interpolate takes.  attrs: a dict mesh slot → a CUDA
    float32 tensor [V, C] (shared by the frames) or [n_frames, V, C], V the slot's vertex count, one C <= abi.ATTR_MAX_CH for all →
    [n_frames, T, 3, C] float32, T = pos_tris (default: the largest triangle count of the set's frames): zeros first, then one
    FrameSet.corner_attr call per slot, so the triangles of slots the dict does not name stay zero.  Differentiable with respect to
    every tensor of the dict (FrameSet.corner_attr_grad, a gather: bit-reproducible); a [V, C] tensor's gradient is the per-frame
    result summed over the frames, as scene_positions has it.  interpolate(fs, vis, corner_attr(fs, {slot: mesh_normals(ctx, slot,
    verts)})) carries a shading loss to the vertices through the normals.  stream: a raw stream handle, None = torch's current stream."""
    slots = tuple(sorted(attrs))
    if not slots:
        raise ValueError("corner_attr: no attributes given")
    n_ch = attrs[slots[0]].shape[-1] if attrs[slots[0]].dim() else 0
    for m in slots:
        a = attrs[m]
        V = fs.ctx.mesh_sizes[m][0]
        if a.dtype != torch.float32 or not a.is_cuda or tuple(a.shape) not in ((V, n_ch), (fs.n_frames, V, n_ch)) or not 1 <= n_ch <= abi.ATTR_MAX_CH:
            raise ValueError(f"corner_attr: slot {m} must be a CUDA float32 tensor [{V}, C] or [{fs.n_frames}, {V}, C] with one C in "
                             f"1..{abi.ATTR_MAX_CH} for every slot, got {tuple(a.shape)} {a.dtype}")
    return _CornerAttr.apply(fs, slots, pos_tris, stream, *[attrs[m] for m in slots])


# ------------------------------------------------------------------------------------------------ perspective-correct interpolation
def _q_dims(fs, q, name):
    """→ (q detached and contiguous, its frame count, its triangle count)"""
    q_frames = _lead_frames(fs, q, (2, 3), f"{name}: q", "a CUDA float32 tensor [T, 3] or [n_frames, T, 3]", lambda t: t.shape[-1] == 3)
    return q.detach().contiguous(), q_frames, q.shape[-2]


def perspective(fs, vis, q, out=None, stream=None):
    """the visibility buffer `vis` of FrameSet `fs` with its screen-linear alpha, beta rewritten into the PERSPECTIVE-CORRECT ones
    (FrameSet.perspective; include/srz.h states the rule): q is a CUDA float32 tensor [T, 3] (one array for every frame) or
    [n_frames, T, 3], the reciprocal clip w of every triangle's corners (clip_q gives it for a sceneset), T at least every frame's
    triangle count → a buffer of vis's layout (`out`, or a new one), every word of it written: z, the ids and nobody's pixels
    copied.  The ATTRIBUTE-SIDE passes take the result — interpolate, interpolate_bary_grad, FrameSet.gbuffer and
    shade_visibility, and texture* through their planes — and are then perspective-correct; the GEOMETRIC ones keep taking the
    ORIGINAL `vis`: position_grad, FrameSet.motion, antialias, peel, interpolate_deriv.  Not differentiable by itself:
    interpolate_persp is the autograd form.  stream: a raw stream handle, None = torch's current stream."""
    _vis_arg(fs, vis, "perspective: vis")
    q, q_frames, q_tris = _q_dims(fs, q, "perspective")
    out = torch.empty(fs.out_shape, dtype=torch.float32, device=vis.device) if out is None else _vis_arg(fs, out, "perspective: out")
    fs.perspective(vis.data_ptr(), q.data_ptr(), q_frames, q_tris, out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, _stream_ptr(stream))
    return out


def perspective_grad(fs, vis, q, gbary_p, want_gbary=True, want_gq=True, stream=None):
    """the backward of perspective(fs, vis, q) by one FrameSet.perspective_grad call: gbary_p [n_frames, 2, rows, W], the gradient
    with respect to alpha', beta' (interpolate_bary_grad on the perspective buffer) → (gbary, gq), each None when not wanted (not
    both): gbary [n_frames, 2, rows, W] is the gradient with respect to the screen-linear alpha, beta — what position_grad takes
    together with the ORIGINAL vis; deterministic, zeros where nobody owns the pixel —, gq has q's shape: a sum of float atomics into
    zeros, not bit-reproducible between runs.  stream: a raw stream handle, None = torch's current stream."""
    if not want_gbary and not want_gq:
        raise ValueError("perspective_grad: neither gbary nor gq is asked for")
    _vis_arg(fs, vis, "perspective_grad: vis")
    q, q_frames, q_tris = _q_dims(fs, q, "perspective_grad")
    gbary_p = _plane(fs, gbary_p, 2, "perspective_grad: gbary_p")
    gbary = torch.empty_like(gbary_p) if want_gbary else None
    gq = torch.zeros_like(q) if want_gq else None
    fs.perspective_grad(vis.data_ptr(), q.data_ptr(), q_frames, q_tris, gbary_p.data_ptr(), _ptr(gbary), _ptr(gq), abi.FUSED_CLEAR,
                        _stream_ptr(stream))
    return gbary, gq


class _InterpolatePersp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, pos, q, fs, vis, stream):
        attr_frames, tris, n_ch = _attr_dims(fs, attr)
        attr, ctx.pos_shape = attr.contiguous(), _pos_handle(fs, pos, "interpolate_persp")
        pvis = perspective(fs, vis, q, stream=stream)
        out = torch.empty(fs.interpolate_shape(n_ch), dtype=torch.float32, device=attr.device)
        fs.interpolate(pvis.data_ptr(), attr.data_ptr(), n_ch, attr_frames, tris, out.data_ptr(), fs.interpolate_bytes(n_ch), abi.FUSED_CLEAR,
                       _stream_ptr(stream))
        ctx.fs, ctx.vis, ctx.pvis, ctx.stream = fs, vis, pvis, stream
        ctx.save_for_backward(attr, q.detach())
        return out

    @staticmethod
    def backward(ctx, gout):
        fs, vis, pvis, (attr, q) = ctx.fs, ctx.vis, ctx.pvis, ctx.saved_tensors
        need_attr, need_pos, need_q = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gout = gout.contiguous()
        attr_frames, tris, n_ch = _attr_dims(fs, attr)
        sp = _stream_ptr(ctx.stream)
        need_bary = need_pos or need_q
        # one interpolate_grad call on the perspective buffer for both of its outputs, one perspective_grad call, one position_grad
        # call on the ORIGINAL buffer
        gattr = torch.zeros_like(attr) if need_attr else None
        gbary_p = torch.empty(fs.interpolate_shape(2), dtype=torch.float32, device=gout.device) if need_bary else None
        if need_attr or need_bary:
            fs.interpolate_grad(pvis.data_ptr(), gout.data_ptr(), attr.data_ptr(), n_ch, attr_frames, tris, _ptr(gattr), _ptr(gbary_p), abi.FUSED_CLEAR, sp)
        gpos = gq = None
        if need_bary:
            gbary, gq = perspective_grad(fs, vis, q, gbary_p, need_pos, need_q, ctx.stream)
            if need_pos:
                gpos = torch.zeros(ctx.pos_shape, dtype=torch.float32, device=gout.device)
                fs.position_grad(vis.data_ptr(), gbary.data_ptr(), None, ctx.pos_shape[1], gpos.data_ptr(), None, abi.FUSED_CLEAR, sp)
        return gattr, gpos, gq, None, None, None


def interpolate_persp(fs, vis, attr, pos, q, stream=None):
    """interpolate_geo under the PERSPECTIVE-CORRECT interpolation: interpolate(fs, perspective(fs, vis, q), attr), differentiable
    with respect to attr, to the triangles' screen positions and to q.  attr and pos as interpolate_geo takes them — pos
    [n_frames, T, 3, 3] is the graph handle whose VALUES ARE NEVER READ (scene_positions gives it) —; q, [T, 3] or [n_frames, T, 3],
    is the reciprocal clip w of every corner and ITS VALUES ARE READ (clip_q gives it as a function of the vertices and matrices).
    Backward: interpolate_grad on the perspective buffer gives attr.grad and the alpha', beta' planes; perspective_grad turns those
    into q.grad and the screen-linear alpha, beta planes; position_grad on the ORIGINAL vis then gives pos.grad — each asked only for
    what some input needs.  The perspective buffer of the forward is SAVED for the backward (16 bytes per pixel held between the
    two), not recomputed.  Owners are held fixed; attr.grad, pos.grad and q.grad are sums of float atomics: not bit-reproducible
    between runs.  stream: a raw stream handle, None = torch's current stream."""
    return _InterpolatePersp.apply(attr, pos, q, fs, vis, stream)


def clip_q(fs, meshes, mvp, pos_tris=None, stream=None):
    """q for sceneset `fs` — the reciprocal of the clip w its vertex stage divides by, per corner of the triangle stream — as plain
    torch ops on the tensors scene_positions takes, so that autograd reaches the vertices and the matrices: meshes, a dict mesh slot
    → vertex positions [V, 3] or [n_frames, V, 3]; mvp [n_frames, D, 16], every draw's ndc_mvp in its own column-major order.  Per
    frame and draw r3 = (m[3] x + m[7] y) + (m[11] z + m[15]) over the slot's vertices, q = 1 / r3, laid out by corner_attr at one
    channel → [n_frames, T, 3] float32; the triangles of slots the dict does not name get q = 0 (their pixels keep the screen-linear
    weights).  UNLIKE scene_positions' handles THE VALUES ARE READ: the caller warrants they are what the set was made from.
    corner_attr gives every draw of a slot in a frame the same per-vertex array, so a set that draws one slot TWICE IN A FRAME
    raises ValueError: such a caller lays q out themselves, per draw."""
    draws = _scene_draws(fs)
    D = max(1, max(len(d) for d in draws))
    if mvp.dtype != torch.float32 or tuple(mvp.shape) != (fs.n_frames, D, 16):
        raise ValueError(f"clip_q: mvp must be float32 {(fs.n_frames, D, 16)}, got {tuple(mvp.shape)} {mvp.dtype}")
    per_vertex = {}
    for m in sorted(meshes):
        v = meshes[m]
        V = fs.ctx.mesh_sizes[m][0]
        if v.dtype != torch.float32 or tuple(v.shape) not in ((V, 3), (fs.n_frames, V, 3)):
            raise ValueError(f"clip_q: mesh {m} must be float32 [{V}, 3] or [{fs.n_frames}, {V}, 3], got {tuple(v.shape)} {v.dtype}")
        rows = []
        for f, d in enumerate(draws):
            if d.count(m) > 1:
                raise ValueError(f"clip_q: frame {f} draws mesh slot {m} {d.count(m)} times; lay q out per draw instead")
            vf = v if v.dim() == 2 else v[f]
            if m not in d:  # (corner_attr writes nothing for this frame: any finite values)
                rows.append(torch.ones((V, 1), dtype=torch.float32, device=v.device))
                continue
            w = mvp[f, d.index(m)]
            r3 = (w[3] * vf[:, 0] + w[7] * vf[:, 1]) + (w[11] * vf[:, 2] + w[15])
            rows.append((1.0 / r3)[:, None])
        per_vertex[m] = torch.stack(rows)
    return corner_attr(fs, per_vertex, pos_tris, stream)[..., 0]


def interpolate_deriv_persp(fs, vis, attr, q, stream=None):
    """interpolate_deriv under the PERSPECTIVE-CORRECT interpolation (FrameSet.interpolate_deriv_persp): the per-pixel screen-space
    derivatives of interpolate(fs, perspective(fs, vis, q), attr) → [n_frames, 2 C, rows, W] float32, the planes texture_mip takes
    for a [T, 3, 2] uv attribute.  vis is the ORIGINAL buffer, q as perspective takes it.  Not differentiable: the planes only select
    a mip level.  stream: a raw stream handle, None = torch's current stream."""
    _vis_arg(fs, vis, "interpolate_deriv_persp: vis")
    attr_frames, tris, n_ch = _attr_dims(fs, attr)
    attr, (q, q_frames, q_tris) = attr.detach().contiguous(), _q_dims(fs, q, "interpolate_deriv_persp")
    if n_ch > abi.ATTR_MAX_CH // 2:
        raise ValueError(f"interpolate_deriv_persp: {n_ch} channels; at most {abi.ATTR_MAX_CH // 2} are supported")
    out = torch.empty(fs.interpolate_shape(2 * n_ch), dtype=torch.float32, device=attr.device)
    fs.interpolate_deriv_persp(vis.data_ptr(), q.data_ptr(), q_frames, q_tris, attr.data_ptr(), n_ch, attr_frames, tris, out.data_ptr(),
                               fs.interpolate_bytes(2 * n_ch), abi.FUSED_CLEAR, _stream_ptr(stream))
    return out
