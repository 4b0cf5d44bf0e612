"""Silhouette antialiasing of a visibility buffer (srz_frameset_antialias / _antialias_grad), BASELINE configs 1-5 at n_ch = 3, in
one process, alternating.

    python tools/antialias_probe.py [rounds] [--configs 1,2,3,4,5] [--out FILE]

Per config: one frameset of bench.py's batch size (tools/vis_probe.py's sets), one visibility buffer of it and seeded planes.  After
10 warm-up rounds the calls alternate, each timed with device events on its own; the median of the rounds (default 20) is reported
with p10 and p90: the forward, the backward with gin only, with gpos only and with both, and interpolate at C = 3, which reads the
same ids and writes the same planes.  Counted: the differing pairs of the whole set (in torch, from the ids), and on frame 0 — by
the tests' CPU reference (tests/antialiasref.py) on that frame's buffer — the blended and the interior-skipped pairs.  The floor is
4 bytes of id per pixel plus 8 n_ch bytes per pixel at the device-to-device copy rate.  Prints one JSON line per config and writes
them to --out.  Nothing is asserted."""
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import antialiasref  # noqa: E402
import srz  # noqa: E402
from srz import abi  # noqa: E402
from srz.visibility import decode  # noqa: E402
from support import frame_positions  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s: device-to-device copies
WARMUP, N_CH = 10, 3


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
    tmp = tempfile.mkdtemp()
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
        tri = decode(vis).tri
        pixels = n * fs.local_rows * fs.width
        differ = int((tri[:, :, 1:] != tri[:, :, :-1]).sum()) + int((tri[:, 1:] != tri[:, :-1]).sum())
        k0 = antialiasref.counters(tmp, frame_positions(frames[0]), frames[0].n_tris, vis[0].cpu().numpy().view(np.uint32))
        nb = fs.interpolate_bytes(N_CH)
        cin, gout = torch.randn(fs.interpolate_shape(N_CH), device="cuda"), torch.randn(fs.interpolate_shape(N_CH), device="cuda")
        out = torch.empty_like(cin)
        gpos = torch.zeros((n, T, 3, 3), dtype=torch.float32, device="cuda")
        attr = torch.randn((T, 3, N_CH), device="cuda")

        def bw(i, p):
            return lambda: fs.antialias_grad(vis.data_ptr(), cin.data_ptr(), gout.data_ptr(), N_CH, out.data_ptr() if i else None, T,
                                             gpos.data_ptr() if p else None, F, sp)
        calls = {"forward": lambda: fs.antialias(vis.data_ptr(), cin.data_ptr(), N_CH, out.data_ptr(), nb, F, sp),
                 "grad_gin": bw(1, 0), "grad_gpos": bw(0, 1), "grad_both": bw(1, 1),
                 "interpolate": lambda: fs.interpolate(vis.data_ptr(), attr.data_ptr(), N_CH, 1, T, out.data_ptr(), nb, F, sp)}
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
        row = {"config": cfg, "workload": wl_name or "config1_256", "frames": n, "rounds": rounds, "n_ch": N_CH, "pixels": pixels,
               "differing_pairs": differ, "frame0": k0, "floor_ms": (4 + 8 * N_CH) * pixels / COPY_RATE * 1e3}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90), "ms_series": [round(x, 4) for x in ms]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del vis, tri, cin, gout, out, gpos, attr
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
