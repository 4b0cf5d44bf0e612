"""Tangent-space normal mapping (srz_frameset_normal_map / _normal_map_grad) beside the lighting pass it feeds (srz_frameset_light /
_light_grad, one light, planes only) on BASELINE config 2's set (256 frames of 1024^2), and the mesh tangents (srz_mesh_tangents /
_tangents_grad) beside the mesh normals (srz_mesh_normals / _normals_grad) on the spot mesh, in one process, alternating.

    python tools/normal_map_probe.py [rounds] [--frames N] [--sets 1,16] [--out FILE]

One frameset of tools/vis_probe.py's config 2, one visibility buffer of it, the normal planes interpolate writes for the frames' own
per-vertex normals, tangent planes of noise roughly along x with w = +-1, m planes of noise around (0, 0, 1), position planes from a
linear ramp.  After 10 warm-up rounds the calls alternate, each timed with device events on its own; the median of the rounds (default
20) is reported with p10 and p90.  Per pass: the bytes it must move (forward: the id word of every pixel, ten input words per owned
pixel, three output words per pixel under the fused clear; backward: the id word, thirteen input words per owned pixel, ten output
words per pixel), that over the median as a fraction of the measured 6.29 TB/s copy rate, and the ratio to light's forward /
backward from the same run.  The mesh legs: per number of position sets, the tangents' medians over the normals'.  Prints one JSON
line and writes it to --out.  Nothing is asserted: no threshold exists to hold these to."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lightref  # noqa: E402
import srz  # noqa: E402
from cube_probe import normals_of  # noqa: E402
from srz import abi, scenes  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s: device-to-device copies
P, WARMUP = 5, 10


def timed(s, calls, rounds):
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
    out = {}
    for k, evs in times.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        out[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90), "ms_series": [round(x, 4) for x in ms]}
    return out


def passes(ctx, s, n_frames, rounds):
    sp, F = s.cuda_stream, abi.FUSED_CLEAR
    cfg, wl_name, _ = next(c for c in CONFIGS if c[0] == 2)
    frames = frames_of(cfg, wl_name, n_frames, ctx)
    fs = ctx.frameset(frames)
    attr, T = normals_of(frames)
    vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
    nrm = torch.empty(fs.interpolate_shape(3), dtype=torch.float32, device="cuda")
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, F, sp)
    fs.interpolate(vis.data_ptr(), attr.data_ptr(), 3, n_frames, T, nrm.data_ptr(), fs.interpolate_bytes(3), F, sp)
    del attr
    H, W = fs.local_rows, fs.width
    tan = torch.randn(fs.interpolate_shape(4), device="cuda") * 0.3
    tan[:, 0] = tan[:, 0].abs() + 0.6
    tan[:, 3] = torch.where(tan[:, 3] < 0, -1.0, 1.0)
    m = torch.randn(fs.interpolate_shape(3), device="cuda") * 0.4
    m[:, 2] = m[:, 2].abs() + 0.4
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda") * (2.0 / H) - 1, torch.arange(W, device="cuda") * (2.0 / W) - 1, indexing="ij")
    pos = torch.stack([xs, ys, 0.1 * xs - 0.2 * ys]).expand(n_frames, 3, H, W).contiguous()
    gout = torch.randn(fs.interpolate_shape(3), device="cuda")
    out, gn, gm, gp = (torch.empty_like(nrm) for _ in range(4))
    gt = torch.empty_like(tan)
    par = torch.as_tensor(lightref.make_params(7, 1)).cuda().reshape(1, -1).contiguous()
    ids = vis.view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
    n_own = int(((ids > 0) & (ids <= T)).sum())
    del ids
    torch.cuda.synchronize()
    pixels, nb = n_frames * H * W, fs.interpolate_bytes(3)
    v, n_, t_, m_, g_ = vis.data_ptr(), nrm.data_ptr(), tan.data_ptr(), m.data_ptr(), gout.data_ptr()
    calls = {"normal_map": lambda: fs.normal_map(v, n_, t_, m_, out.data_ptr(), nb, F, sp),
             "normal_map_grad": lambda: fs.normal_map_grad(v, n_, t_, m_, g_, gn.data_ptr(), gt.data_ptr(), gm.data_ptr(), F, sp),
             "normal_map_grad_gm": lambda: fs.normal_map_grad(v, n_, t_, m_, g_, None, None, gm.data_ptr(), F, sp),
             "light": lambda: fs.light(v, n_, pos.data_ptr(), None, par.data_ptr(), 1, 1, P, out.data_ptr(), nb, F, sp),
             "light_grad": lambda: fs.light_grad(v, n_, pos.data_ptr(), None, par.data_ptr(), 1, 1, P, g_, gn.data_ptr(), gp.data_ptr(), None, None,
                                                 None, 0, F, sp)}
    row = {"config": cfg, "frames": n_frames, "rounds": rounds, "pixels": pixels, "owned_pixels": n_own}
    row.update(timed(s, calls, rounds))
    moved = {"normal_map": 4 * pixels + 40 * n_own + 12 * pixels, "normal_map_grad": 4 * pixels + 52 * n_own + 40 * pixels,
             "normal_map_grad_gm": 4 * pixels + 52 * n_own + 12 * pixels}
    for k, b in moved.items():
        row[k]["bytes"] = b
        row[k]["of_copy_rate"] = b / (row[k]["ms_median"] * 1e-3) / COPY_RATE
    row["normal_map"]["over_light"] = row["normal_map"]["ms_median"] / row["light"]["ms_median"]
    for k in ("normal_map_grad", "normal_map_grad_gm"):
        row[k]["over_light_grad"] = row[k]["ms_median"] / row["light_grad"]["ms_median"]
    fs.close()
    return row


def mesh(ctx, s, sets, rounds):
    sp = s.cuda_stream
    wl = scenes.WORKLOADS["spot_bunny_phong_1080p"]()
    wl.upload_meshes(ctx)
    slot = next(i for i, mm in enumerate(wl.meshes) if "spot" in mm[0])
    v, f = wl.scene.mesh(wl.meshes[slot][0])
    v = np.asarray(v, np.float32).reshape(-1, 8)
    rows = []
    for B in sets:
        pos = (torch.as_tensor(v[:, :3]).cuda()[None] * (1.0 + 0.01 * torch.rand((B, 1, 1), device="cuda"))).contiguous()
        nrm, work, gpos, gn = (torch.empty_like(pos) for _ in range(4))
        tan, gt = torch.empty((B, len(v), 4), device="cuda"), torch.randn((B, len(v), 4), device="cuda")
        gn.normal_()
        calls = {"normals": lambda: ctx.mesh_normals(slot, pos.data_ptr(), 3, B, nrm.data_ptr(), 3, sp),
                 "tangents": lambda: ctx.mesh_tangents(slot, pos.data_ptr(), 3, B, None, 0, tan.data_ptr(), 4, sp),
                 "normals_grad": lambda: ctx.mesh_normals_grad(slot, pos.data_ptr(), 3, B, gn.data_ptr(), 3, work.data_ptr(), gpos.data_ptr(), sp),
                 "tangents_grad": lambda: ctx.mesh_tangents_grad(slot, pos.data_ptr(), 3, B, None, 0, gt.data_ptr(), 4, work.data_ptr(),
                                                                 gpos.data_ptr(), sp)}
        row = {"mesh": wl.meshes[slot][0], "sets": B, "vertices": len(v), "faces": len(np.asarray(f).reshape(-1, 3))}
        row.update(timed(s, calls, rounds))
        row["tangents"]["over_normals"] = row["tangents"]["ms_median"] / row["normals"]["ms_median"]
        row["tangents_grad"]["over_normals_grad"] = row["tangents_grad"]["ms_median"] / row["normals_grad"]["ms_median"]
        rows.append(row)
    return rows


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    n_frames, sets, out_path = 256, [1, 16], None
    if "--frames" in args:
        n_frames = int(args[args.index("--frames") + 1])
    if "--sets" in args:
        sets = [int(c) for c in args[args.index("--sets") + 1].split(",")]
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    row = {"passes": passes(ctx, s, n_frames, rounds)}
    torch.cuda.empty_cache()
    row["mesh"] = mesh(ctx, s, sets, rounds)
    print(json.dumps(row), flush=True)
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
