"""Gradients to vertex positions from a visibility buffer (srz_frameset_position_grad), BASELINE configs 1-5, in one process,
alternating.

    python tools/posgrad_probe.py [rounds] [--configs 1,2,3,4,5] [--out FILE]

Per config: one frameset of bench.py's batch size (tools/vis_probe.py's sets) and one visibility buffer of it.  After 10 warm-up
rounds the calls alternate, each timed with device events on its own; the median of the rounds (default 20) is reported with p10
and p90: position_grad from gbary (gpos; gpos and gpix), from gz, from both, gpix alone, and the formulation a user writes in torch
today (srz.visibility.decode, a gather of the owner's nine floats per owned pixel, the arithmetic of include/srz.h, index_add_ into
[n, T, 3, 3]).  Counted in torch from the buffer: the owned pixels and the distinct (tile, owner) pairs, and the bytes of global
float adds the design implies (pairs * 36) beside one add per (pixel, value).  Prints one JSON line per config and writes them to
--out.  Nothing is asserted."""
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
from interp_probe import tile_owner_pairs  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

COPY_RATE, ADD_RATE = 6.29e12, 1.3e12  # bytes / s: device-to-device copies; global float adds, chip-wide
WARMUP = 10


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
        T = max(f.n_tris for f in frames)
        vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
        fs.render_visibility(vis.data_ptr(), fs.out_bytes, F, sp)
        torch.cuda.synchronize()
        d = decode(vis)
        owned = d.tri >= 0
        pixels, n_owned, pairs = n * fs.local_rows * fs.width, int(owned.sum()), tile_owner_pairs(vis, T)
        host_pos = np.zeros((n, T, 3, 3), np.float32)
        for i, f in enumerate(frames):
            host_pos[i, :f.n_tris] = np.concatenate([t["pos"] for t in f.tris])
        pos = torch.as_tensor(host_pos).cuda()
        gbary, gz = torch.randn(fs.interpolate_shape(2), device="cuda"), torch.randn(fs.interpolate_shape(1), device="cuda")
        gpos = torch.zeros((n, T, 3, 3), dtype=torch.float32, device="cuda")
        gpix = torch.empty(fs.interpolate_shape(2), dtype=torch.float32, device="cuda")
        flat = (torch.arange(n, device="cuda")[:, None, None] * T + d.tri)[owned]  # [owned]: frame * T + triangle
        w = torch.stack([d.alpha, d.beta, d.gamma], -1)[owned]  # [owned, 3]

        def torch_formulation():
            P = pos.view(-1, 3, 3)[flat]  # the gather: nine floats per owned pixel
            a, b, c = P[:, 0], P[:, 1], P[:, 2]
            r = 1.0 / ((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]))
            g = gz[:, 0][owned]
            da = gbary[:, 0][owned] + g * (a[:, 2] - c[:, 2])
            db = gbary[:, 1][owned] + g * (b[:, 2] - c[:, 2])
            gx = (da * (b[:, 1] - c[:, 1]) + db * (c[:, 1] - a[:, 1])) * r
            gy = (da * (c[:, 0] - b[:, 0]) + db * (a[:, 0] - c[:, 0])) * r
            terms = torch.stack([-w * gx[:, None], -w * gy[:, None], w * g[:, None]], -1)  # [owned, corner, (x, y, z)]
            return torch.zeros((n * T, 3, 3), device="cuda").index_add_(0, flat, terms)

        def pg(b, z, p, x):
            return lambda: fs.position_grad(vis.data_ptr(), gbary.data_ptr() if b else None, gz.data_ptr() if z else None, T,
                                            gpos.data_ptr() if p else None, gpix.data_ptr() if x else None, F, sp)
        calls = {"gbary_gpos": pg(1, 0, 1, 0), "gbary_gpos_gpix": pg(1, 0, 1, 1), "gz_gpos": pg(0, 1, 1, 0), "both_gpos": pg(1, 1, 1, 0),
                 "both_gpix": pg(1, 1, 0, 1), "torch": torch_formulation}
        try:  # the gather may not fit beside the set: the leg is then left out
            calls["torch"]()
        except torch.cuda.OutOfMemoryError:
            del calls["torch"]
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
        row = {"config": cfg, "workload": wl_name or "config1_256", "frames": n, "rounds": rounds, "pixels": pixels, "owned_pixels": n_owned,
               "tile_owner_pairs": pairs, "atomic_bytes": pairs * 36, "atomic_bytes_per_pixel_adds": n_owned * 36,
               "atomic_floor_ms": pairs * 36 / ADD_RATE * 1e3,
               "floor_ms_gbary_gpos": (4 * pixels + (8 + 36 + 8) * n_owned) / COPY_RATE * 1e3,
               "floor_ms_both_gpos": (4 * pixels + (8 + 36 + 12) * n_owned) / COPY_RATE * 1e3}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90), "ms_series": [round(x, 4) for x in ms]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del vis, d, owned, pos, gbary, gz, gpos, gpix, flat, w
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
