"""Caller attributes over a visibility buffer (srz_frameset_interpolate / _interpolate_grad), BASELINE configs 1-5, in one process,
alternating.

    python tools/interp_probe.py [rounds] [--configs 1,2,3,4,5] [--out FILE]

Per config: one frameset of bench.py's batch size (tools/vis_probe.py's sets: poses of one mesh) and one visibility buffer of it.
For C in {2, 8}, after 10 warm-up rounds, five calls alternate, each timed with device events on its own; the median of the rounds
(default 20) is reported with p10 and p90: the forward pass, the backward with shared attributes ([T, 3, C]), the backward with
per-frame attributes ([n, T, 3, C]), gbuffer(UV) (the yardstick: at C = 2 the forward is the same work), and the formulation a user
writes in torch today (srz.visibility.decode, a gather of [n, H, W, 3, C], three multiplies per channel; backward: index_add_).
Counted in torch from the buffer: the owned pixels and the distinct (tile, owner) pairs, and the bytes of global float adds the
backward's design implies (pairs * 3 * C * 4) beside one add per (pixel, corner, channel).  Prints one JSON line per (config, C) and
writes them to --out.  Nothing is asserted."""
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
from srz import abi  # noqa: E402
from srz.visibility import decode  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

COPY_RATE, ADD_RATE = 6.29e12, 1.3e12  # bytes / s: device-to-device copies; global float adds, chip-wide
CHANNELS = (2, 8)
WARMUP = 10


def tile_owner_pairs(vis, n_tris):
    """distinct (frame, tile, owner) triples of a visibility buffer [n, 4, rows, W]"""
    ids = vis.view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
    n, rows, W = ids.shape
    ys, xs = torch.arange(rows, device=ids.device) // 32, torch.arange(W, device=ids.device) // 32
    tile = (torch.arange(n, device=ids.device)[:, None, None] * ((rows + 31) // 32) + ys[None, :, None]) * ((W + 31) // 32) + xs[None, None, :]
    owned = (ids > 0) & (ids <= n_tris)
    return int(torch.unique(tile[owned] * (n_tris + 1) + ids[owned]).numel())


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    pick = {1, 2, 3, 4, 5}
    out_path = None
    if "--configs" in args:
        pick = {int(c) for c in args[args.index("--configs") + 1].split(",")}
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    sp, F = s.cuda_stream, abi.FUSED_CLEAR
    rows = []
    for cfg, wl_name, n in CONFIGS:
        if cfg not in pick:
            continue
        frames = frames_of(cfg, wl_name, n, ctx)
        fs = ctx.frameset(frames)
        T = max(sum(len(t) for t in f.tris) for f in frames)
        vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
        fs.render_visibility(vis.data_ptr(), fs.out_bytes, F, sp)
        torch.cuda.synchronize()
        d = decode(vis)
        owned = d.tri >= 0
        pixels, n_owned, pairs = n * fs.local_rows * fs.width, int(owned.sum()), tile_owner_pairs(vis, T)
        gb = torch.empty(fs.gbuffer_shape(abi.GB_UV), dtype=torch.float32, device="cuda")
        for C in CHANNELS:
            shared = torch.randn((T, 3, C), device="cuda")
            per = torch.randn((n, T, 3, C), device="cuda")
            out = torch.empty(fs.interpolate_shape(C), dtype=torch.float32, device="cuda")
            gout = torch.randn(fs.interpolate_shape(C), device="cuda")
            g_sh, g_per = torch.zeros_like(shared), torch.zeros_like(per)
            nb = fs.interpolate_bytes(C)
            wts = torch.stack([d.alpha, d.beta, d.gamma], -1)  # [n, H, W, 3]
            idx = d.tri.clamp(min=0)

            def torch_forward():
                return (shared[idx] * wts[..., None]).sum(-2) * owned[..., None]  # the [n, H, W, 3, C] gather

            def torch_backward():
                contrib = (wts[..., None] * gout.permute(0, 2, 3, 1)[..., None, :])[owned]  # [owned, 3, C]
                return torch.zeros_like(shared).index_add_(0, d.tri[owned], contrib)
            calls = {"forward": lambda: fs.interpolate(vis.data_ptr(), shared.data_ptr(), C, 1, T, out.data_ptr(), nb, F, sp),
                     "backward_shared": lambda: fs.interpolate_grad(vis.data_ptr(), gout.data_ptr(), None, C, 1, T, g_sh.data_ptr(), None, F, sp),
                     "backward_per_frame": lambda: fs.interpolate_grad(vis.data_ptr(), gout.data_ptr(), None, C, n, T, g_per.data_ptr(), None, F, sp),
                     "gbuffer_uv": lambda: fs.gbuffer(vis.data_ptr(), gb.data_ptr(), fs.gbuffer_bytes(abi.GB_UV), abi.GB_UV, F, sp),
                     "torch_forward": torch_forward, "torch_backward": torch_backward}
            for k in ("torch_forward", "torch_backward"):  # the gather may not fit beside the set: the leg is then left out
                try:
                    calls[k]()
                except torch.cuda.OutOfMemoryError:
                    del calls[k]
                    torch.cuda.empty_cache()
            for _ in range(WARMUP):  # clock ramp, first launches, the caching allocator's blocks
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
            row = {"config": cfg, "workload": wl_name or "config1_256", "frames": n, "rounds": rounds, "channels": C, "pixels": pixels,
                   "owned_pixels": n_owned, "tile_owner_pairs": pairs, "atomic_bytes": pairs * 3 * C * 4,
                   "atomic_bytes_per_pixel_adds": n_owned * 3 * C * 4, "atomic_floor_ms": pairs * 3 * C * 4 / ADD_RATE * 1e3,
                   "forward_floor_ms": (4 * pixels + (8 + 12 * C) * n_owned + 4 * C * pixels) / COPY_RATE * 1e3,
                   "backward_floor_ms": (4 * pixels + 8 * n_owned + 4 * C * n_owned) / COPY_RATE * 1e3}
            for k, evs in times.items():
                ms = [a.elapsed_time(b) for a, b in evs]
                row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90), "ms_series": [round(x, 4) for x in ms]}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del shared, per, out, gout, g_sh, g_per, wts, idx
            torch.cuda.empty_cache()
        fs.close()
        del vis, gb, d, owned
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
