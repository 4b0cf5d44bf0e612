"""The texture-set lookup (srz.visibility.texture_set: srz_frameset_texture_set / _texture_set_grad) beside what a caller had to
write before it — one texture() per material over every pixel, a coverage mask per material through decode and batch_of, torch.where
— in one process, alternating.

    python tools/texset_probe.py [rounds] [--frames 256] [--out FILE]

The set is BASELINE config 2's in size (256 frames of 1024 x 1024) with the README scene's two batches, spot and the crate, each with
its own image as a float32 texture of three channels; uv is interpolate() of the frames' own uv.  The masks of the torch side are
made once outside the timed region (they cost an int64 round trip through decode and batch_of, timed on its own as `masks`).  After
10 warm-up rounds the calls alternate, each timed with device events on its own; the median of the rounds (default 20) is reported
with p10 and p90:
  1. the forward of both;  2. forward + backward of both, to both textures and to uv;
  3. torch.cuda.max_memory_allocated over one forward + backward of each, above what is allocated before it;
  4. a device copy of the output's size, its rate, and the time the fused forward's own bytes take at that rate — 4 B of id per
     pixel, 8 B of uv, 2 B of batch and 12 B written per owned pixel, from the owned-pixel count (the texels and the 1-byte map come
     from cache).
Prints one JSON line and writes it to --out.  Nothing is asserted."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import srz  # noqa: E402
from srz import scenes  # noqa: E402
from srz import visibility as V  # noqa: E402
from vis_probe import pct  # noqa: E402

C = 3
WARMUP = 10
WORKLOAD = "readme_spot_crate_1024"


def float_texture(img):
    """an uploaded 8-bit image [H, W, >= 3] → float32 [H, W, 3] in [0, 1]"""
    a = np.asarray(img)
    assert a.ndim == 3 and a.shape[2] >= 3, a.shape
    return np.ascontiguousarray(a[..., :3], np.float32) / np.float32(255)


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    n = int(args[args.index("--frames") + 1]) if "--frames" in args else 256
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    wl = scenes.WORKLOADS[WORKLOAD]()
    uniq = [wl.frame(i) for i in range(min(n, 36))]
    wl.upload_textures(ctx)
    frames = [uniq[i % len(uniq)] for i in range(n)]
    n_batches = len(frames[0].tris)
    assert n_batches == 2 and len(wl.texture_arrays) == 2
    fs = ctx.frameset(frames)
    vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, srz.abi.FUSED_CLEAR, s.cuda_stream)
    T = max(f.n_tris for f in uniq)
    attr = np.zeros((len(uniq), T, 3, 2), np.float32)
    for i, f in enumerate(uniq):
        attr[i, :f.n_tris] = np.concatenate([t["uv"] for t in f.tris])
    attr = torch.as_tensor(attr[[i % len(uniq) for i in range(n)]]).cuda()
    uv = V.interpolate(fs, vis, attr).detach()
    del attr
    texs = [torch.as_tensor(float_texture(wl.texture_arrays[frames[0]._batches[b].tex_id])).cuda() for b in range(n_batches)]
    batch_slot = torch.tensor([0, 1], dtype=torch.uint8, device="cuda")

    def make_masks():
        tri = V.decode(vis).tri
        b = torch.stack([V.batch_of(frames[i], tri[i]) for i in range(n)])
        return [(b == k)[:, None] for k in range(n_batches)]
    masks = make_masks()
    owned = [int(m.sum()) for m in masks]
    gen = torch.Generator(device="cuda").manual_seed(1)
    gout = torch.rand(fs.interpolate_shape(C), device="cuda", generator=gen)
    zero = torch.zeros((), device="cuda")
    pixels = n * fs.local_rows * fs.width
    src, dst = torch.rand(fs.interpolate_shape(C), device="cuda", generator=gen), torch.empty(fs.interpolate_shape(C), device="cuda")

    def leaves(ts):
        return [t.detach().requires_grad_(True) for t in ts]

    def composed(t, u):
        out = None
        for k in range(n_batches):
            term = torch.where(masks[k], V.texture(fs, vis, t[k], u), zero)
            out = term if out is None else out + term
        return out

    def set_fwd():
        with torch.no_grad():
            return V.texture_set(fs, vis, texs, uv, batch_slot)

    def torch_fwd():
        with torch.no_grad():
            return composed(texs, uv)

    def set_both():
        t, (u,) = leaves(texs), leaves([uv])
        (V.texture_set(fs, vis, t, u, batch_slot) * gout).sum().backward()

    def torch_both():
        t, (u,) = leaves(texs), leaves([uv])
        (composed(t, u) * gout).sum().backward()
    forward_equal = bool(torch.equal(set_fwd(), torch_fwd()))
    calls = {"set_forward": set_fwd, "torch_forward": torch_fwd, "set_forward_backward": set_both, "torch_forward_backward": torch_both,
             "copy": lambda: dst.copy_(src), "masks": make_masks}
    for _ in range(WARMUP):  # clock ramp, first launches, the allocator's pool
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            times[k].append((e0, e1))
    torch.cuda.synchronize()
    row = {"workload": WORKLOAD, "frames": n, "rounds": rounds, "channels": C, "slots": n_batches, "pixels": pixels, "owned_pixels_per_batch": owned,
           "texture_shapes": [list(t.shape) for t in texs], "forward_equal": forward_equal}
    for k, evs in times.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90)}
    for k in ("set_forward_backward", "torch_forward_backward"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        calls[k]()
        torch.cuda.synchronize()
        row[k]["peak_bytes_above_inputs"] = int(torch.cuda.max_memory_allocated() - base)
    copy_bytes = 2 * C * 4 * pixels
    rate = copy_bytes / (row["copy"]["ms_median"] * 1e-3)
    own_bytes = 4 * pixels + (8 + 2 + 4 * C) * sum(owned)
    row["copy_rate_TBps"] = rate / 1e12
    row["set_forward_bytes"] = own_bytes
    row["set_forward_ms_at_copy_rate"] = own_bytes / rate * 1e3
    fused_bytes = own_bytes + 4 * C * (pixels - sum(owned))  # (texture_set passes SRZ_FUSED_CLEAR: nobody's words are written too)
    row["set_forward_bytes_with_clear"] = fused_bytes
    row["set_forward_ms_at_copy_rate_with_clear"] = fused_bytes / rate * 1e3
    print(json.dumps(row), flush=True)
    fs.close()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
