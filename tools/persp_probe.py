"""The perspective-correct passes over a visibility buffer (srz_frameset_perspective / _perspective_grad /
_interpolate_deriv_persp), BASELINE configs 1-5, in one process, alternating.

    python tools/persp_probe.py [rounds] [--configs 1,2,3,4,5] [--out FILE]

Per config: one frameset of bench.py's batch size (tools/vis_probe.py's sets: poses of one mesh), one visibility buffer of it, q drawn
from [0.25, 4] per corner ([T, 3], shared by the frames), the frames' own normals ([n, T, 3, 3]) and uv ([n, T, 3, 2]) as attributes.
After 10 warm-up rounds the calls alternate, each timed with device events on its own; the median of the rounds (default 10) is
reported with p10 and p90: perspective forward; perspective_grad with gbary only, with gq only and with both;
interpolate_deriv_persp at n_ch = 2; and the yardsticks, interpolate forward at C = 3 and interpolate_deriv at n_ch = 2.  The
forward's floor is 32 bytes per pixel plus 12 per owned pixel at the copy rate DESIGN.md §5 records.  Prints one JSON line per config
and writes them to --out.  Nothing is asserted."""
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
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s: device-to-device copies
WARMUP = 10


def attrs_of(frames, field, k):
    """[n, T, 3, k] float32 on the device: a per-vertex field of every frame's triangle stream (a set's frames repeat: each distinct
    frame is laid out once)"""
    T = max(sum(len(t) for t in f.tris) for f in frames)
    a = torch.zeros((len(frames), T, 3, k), dtype=torch.float32, device="cuda")
    seen = {}
    for i, f in enumerate(frames):
        if id(f) not in seen:
            v = np.concatenate([t[field] for t in f.tris]) if T else np.zeros((0, 3, k), np.float32)
            seen[id(f)] = torch.as_tensor(np.ascontiguousarray(v, np.float32)).cuda()
        a[i, :seen[id(f)].shape[0]] = seen[id(f)]
    return a, T


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 10
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
        nrm, T = attrs_of(frames, "nrm", 3)
        uv, _ = attrs_of(frames, "uv", 2)
        q = torch.as_tensor(np.random.default_rng(cfg).uniform(0.25, 4.0, (max(T, 1), 3)).astype(np.float32)).cuda()
        vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
        fs.render_visibility(vis.data_ptr(), fs.out_bytes, F, sp)
        torch.cuda.synchronize()
        pixels = n * fs.local_rows * fs.width
        ids = vis.view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
        n_own = int(((ids > 0) & (ids <= T)).sum())
        del ids
        pvis = torch.empty_like(vis)
        out3 = torch.empty(fs.interpolate_shape(3), dtype=torch.float32, device="cuda")
        out4 = torch.empty(fs.interpolate_shape(4), dtype=torch.float32, device="cuda")
        gbp = torch.randn(fs.interpolate_shape(2), device="cuda")
        gbary, gq = torch.empty_like(gbp), torch.zeros_like(q)
        Tq = q.shape[0]

        def bwd(want_bary, want_q):
            return lambda: fs.perspective_grad(vis.data_ptr(), q.data_ptr(), 1, Tq, gbp.data_ptr(), gbary.data_ptr() if want_bary else None,
                                               gq.data_ptr() if want_q else None, F, sp)
        calls = {"forward": lambda: fs.perspective(vis.data_ptr(), q.data_ptr(), 1, Tq, pvis.data_ptr(), fs.out_bytes, F, sp),
                 "backward_gbary": bwd(True, False), "backward_gq": bwd(False, True), "backward_both": bwd(True, True),
                 "deriv_persp_c2": lambda: fs.interpolate_deriv_persp(vis.data_ptr(), q.data_ptr(), 1, Tq, uv.data_ptr(), 2, n, T, out4.data_ptr(),
                                                                      fs.interpolate_bytes(4), F, sp),
                 "interpolate_c3": lambda: fs.interpolate(vis.data_ptr(), nrm.data_ptr(), 3, n, T, out3.data_ptr(), fs.interpolate_bytes(3), F, sp),
                 "interpolate_deriv_c2": lambda: fs.interpolate_deriv(vis.data_ptr(), uv.data_ptr(), 2, n, T, out4.data_ptr(), fs.interpolate_bytes(4),
                                                                      F, sp)}
        for _ in range(WARMUP):  # clock ramp, first launches
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
        row = {"config": cfg, "workload": wl_name or "config1_256", "frames": n, "rounds": rounds, "pixels": pixels, "owned_pixels": n_own,
               "forward_floor_ms": (32 * pixels + 12 * n_own) / COPY_RATE * 1e3}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90), "ms_series": [round(x, 4) for x in ms]}
        row["forward_over_floor"] = row["forward"]["ms_median"] / row["forward_floor_ms"] if row["forward_floor_ms"] else None
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del vis, pvis, out3, out4, gbp, gbary, gq, nrm, uv, q
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
