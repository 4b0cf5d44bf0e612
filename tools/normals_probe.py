"""Vertex normals and per-vertex attributes on the device (srz_mesh_normals, srz_mesh_normals_grad, srz_sceneset_corner_attr,
srz_sceneset_corner_attr_grad) beside the torch formulation of the same results, on the spot mesh and the bunny, in one process,
alternating.

    python tools/normals_probe.py [rounds] [--sets 1,16] [--out FILE]

Per mesh and B (position sets = frames of the sceneset, BASELINE config 3's two meshes): after 10 warm-up rounds the calls alternate,
each timed with device events on its own; the median of the rounds (default 20) is reported with p10 and p90.  The torch legs are what
a user writes today: the normals as a gather through the faces, a cross product, three index_add_ and a guarded normalise; their
backward as torch.autograd.grad over that graph (built once, retained); the corner layout as a fancy-indexed copy into the stream per
draw; its backward as an index_add_ of the corners onto the vertices.  Three channels (a normal) for the attribute legs.  Prints one
JSON line per (mesh, B) and writes them to --out.  Nothing is asserted."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import srz  # noqa: E402
from srz import scenes  # noqa: E402

WARMUP, N_CH = 10, 3


def pct(xs, q):
    return float(np.percentile(np.asarray(xs), q))


def torch_normals(p, f):
    """p [B, V, 3], f [F, 3] int64 -> [B, V, 3]"""
    a, b, c = p[:, f[:, 0]], p[:, f[:, 1]], p[:, f[:, 2]]
    N = torch.cross(b - a, c - a, dim=2)
    S = torch.zeros_like(p)
    for k in range(3):
        S = S.index_add(1, f[:, k], N)
    len2 = (S * S).sum(2, keepdim=True)
    ok = (len2 > 0) & torch.isfinite(len2)
    return torch.where(ok, S * torch.rsqrt(torch.where(ok, len2, torch.ones_like(len2))), torch.zeros_like(S))


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    sets = [1, 16]
    out_path = None
    if "--sets" in args:
        sets = [int(c) for c in args[args.index("--sets") + 1].split(",")]
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    wl = scenes.WORKLOADS["spot_bunny_phong_1080p"]()
    wl.upload_meshes(ctx)
    rows = []
    for B in sets:
        sframes = [wl.scene_frame(i) for i in range(B)]
        fs = ctx.frameset(sframes)
        order = [int(sframes[0]._draws[j].mesh_id) for j in range(sframes[0].c.n_draws)]
        T = sum(ctx.mesh_sizes[m][1] for m in order)
        for slot, (mname, _, _, _, _) in enumerate(wl.meshes):
            v, f = wl.scene.mesh(mname)
            v = np.asarray(v, np.float32).reshape(-1, 8)
            V, F = len(v), len(np.asarray(f).reshape(-1, 3))
            first = sum(ctx.mesh_sizes[m][1] for m in order[:order.index(slot)])
            faces = torch.as_tensor(np.asarray(f, np.int64).reshape(-1, 3)).cuda()
            flat = faces.reshape(-1)
            pos = (torch.as_tensor(v[:, :3]).cuda()[None] * (1.0 + 0.01 * torch.rand((B, 1, 1), device="cuda"))).contiguous()
            nrm, work, gpos, gn = (torch.empty_like(pos) for _ in range(4))
            gn.normal_()
            attr, gattr = torch.randn((B, V, N_CH), device="cuda"), torch.empty((B, V, N_CH), device="cuda")
            out, gout = torch.zeros((B, T, 3, N_CH), device="cuda"), torch.randn((B, T, 3, N_CH), device="cuda")
            leaf = pos.clone().requires_grad_(True)
            graph = torch_normals(leaf, faces)

            def t_corner():
                out[:, first:first + F] = attr[:, faces]

            def t_corner_grad():
                return torch.zeros((B, V, N_CH), device="cuda").index_add_(1, flat, gout[:, first:first + F].reshape(B, 3 * F, N_CH))
            calls = {"normals": lambda: ctx.mesh_normals(slot, pos.data_ptr(), 3, B, nrm.data_ptr(), 3, sp),
                     "normals_torch": lambda: torch_normals(pos, faces),
                     "normals_grad": lambda: ctx.mesh_normals_grad(slot, pos.data_ptr(), 3, B, gn.data_ptr(), 3, work.data_ptr(), gpos.data_ptr(), sp),
                     "normals_grad_torch": lambda: torch.autograd.grad(graph, leaf, gn, retain_graph=True),
                     "corner_attr": lambda: fs.corner_attr(slot, attr.data_ptr(), N_CH, B, out.data_ptr(), T, sp),
                     "corner_attr_torch": t_corner,
                     "corner_attr_grad": lambda: fs.corner_attr_grad(slot, gout.data_ptr(), N_CH, gattr.data_ptr(), T, sp),
                     "corner_attr_grad_torch": t_corner_grad}
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
            row = {"mesh": mname, "sets": B, "vertices": V, "faces": F, "rounds": rounds, "channels": N_CH}
            for k, evs in times.items():
                ms = [a.elapsed_time(b) for a, b in evs]
                row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90)}
            for k in ("normals", "normals_grad", "corner_attr", "corner_attr_grad"):
                row[k + "_torch_over_device"] = row[k + "_torch"]["ms_median"] / row[k]["ms_median"]
            print(json.dumps(row), flush=True)
            rows.append(row)
        fs.close()
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
