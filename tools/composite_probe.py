"""The fused depth-layer composite (srz.visibility.composite_layers: srz_frameset_composite / _composite_grad) beside the torch loop
(srz.visibility.composite), BASELINE config 2 by default, in one process, alternating.

    python tools/composite_probe.py [rounds] [--configs 2] [--out FILE]

layers(fs, 3) of the config's set, C = 3 random colours, an alpha plane per layer, a background.  The torch loop gets what a caller
has to build for it: alpha_k * (decode(layer_k).tri >= 0), made once outside the timed region.  After 10 warm-up rounds the calls
alternate, each timed with device events on its own; the median of the rounds (default 20) is reported with p10 and p90:
  1. the forward of both;  2. forward + backward of both (gradients to every colour, every alpha and the background);
  3. torch.cuda.max_memory_allocated over one forward + backward of each, above what is allocated before it;
  4. a device copy of the output's size, its rate, and the time the fused forward's own bytes take at that rate — 4 B of id per layer
     and pixel, (C + 1) * 4 B per covered layer pixel, C * 4 B of background read and C * 4 B written per pixel, from the layers'
     owned-pixel counts.
Prints one JSON line per config and writes them to --out.  Nothing is asserted."""
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
from srz import visibility as V  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

C, N_LAYERS = 3, 3
WARMUP = 10


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    pick = {2}
    out_path = None
    if "--configs" in args:
        pick = {int(c) for c in args[args.index("--configs") + 1].split(",")}
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    rows = []
    for cfg, wl_name, n in CONFIGS:
        if cfg not in pick:
            continue
        fs = ctx.frameset(frames_of(cfg, wl_name, n, ctx))
        lay = V.layers(fs, N_LAYERS, stream=s.cuda_stream)
        cov = [(V.decode(t).tri >= 0)[:, None] for t in lay]
        owned = [int(c.sum()) for c in cov]
        gen = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda k: torch.rand(fs.interpolate_shape(k), device="cuda", generator=gen)  # noqa: E731
        cols, alphas, bg, gout = [rnd(C) for _ in lay], [rnd(1) for _ in lay], rnd(C), rnd(C)
        eff = [a * c for a, c in zip(alphas, cov)]  # what the torch loop needs: the opacity times the coverage
        del cov
        H, W = fs.local_rows, fs.width
        pixels = n * H * W
        src, dst = rnd(C), torch.empty(fs.interpolate_shape(C), device="cuda")

        def leaves(ts):
            return [t.detach().requires_grad_(True) for t in ts]

        def fused_fwd():
            with torch.no_grad():
                return V.composite_layers(fs, lay, cols, alphas, bg)

        def torch_fwd():
            with torch.no_grad():
                return V.composite(cols, eff) + torch_through(eff) * bg

        def torch_through(es):
            T = 1 - es[0]
            for e in es[1:]:
                T = T * (1 - e)
            return T

        def fused_both():
            c, a, (b,) = leaves(cols), leaves(alphas), leaves([bg])
            (V.composite_layers(fs, lay, c, a, b) * gout).sum().backward()

        def torch_both():
            c, a, (b,) = leaves(cols), leaves(eff), leaves([bg])
            ((V.composite(c, a) + torch_through(a) * b) * gout).sum().backward()
        calls = {"fused_forward": fused_fwd, "torch_forward": torch_fwd, "fused_forward_backward": fused_both,
                 "torch_forward_backward": torch_both, "copy": lambda: dst.copy_(src)}
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
        row = {"config": cfg, "workload": wl_name or "config1_256", "frames": n, "rounds": rounds, "channels": C, "layers": N_LAYERS,
               "pixels": pixels, "owned_pixels_per_layer": owned}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90)}
        for k in ("fused_forward_backward", "torch_forward_backward"):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            calls[k]()
            torch.cuda.synchronize()
            row[k]["peak_bytes_above_inputs"] = int(torch.cuda.max_memory_allocated() - base)
        copy_bytes = 2 * C * 4 * pixels
        rate = copy_bytes / (row["copy"]["ms_median"] * 1e-3)
        own_bytes = 4 * N_LAYERS * pixels + (C + 1) * 4 * sum(owned) + 2 * C * 4 * pixels
        row["copy_rate_TBps"] = rate / 1e12
        row["fused_forward_bytes"] = own_bytes
        row["fused_forward_ms_at_copy_rate"] = own_bytes / rate * 1e3
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del lay, cols, alphas, eff, bg, gout, src, dst
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
