"""The mesh Laplacian on the device (srz_mesh_laplacian, srz_mesh_laplacian_grad) beside the same operator in plain torch on the same
device, on the spot mesh and a generated grid of about a million vertices, in one process, alternating.

    python tools/lap_probe.py [rounds] [--grid 1024] [--out FILE]

Per mesh and kind, a field of C = 3 channels, one set: after 5 warm-up rounds the legs alternate, each timed with device events on its
own; the median of the rounds (default 20) is reported with p10 and p90.  Legs: the forward call; the forward and the backward call;
and the torch formulation of both — what a user writes today with the weights precomputed: per corner the gathers x[a], x[b], one
index_add_ onto the corner's vertex forward, two index_add_ (float atomics) onto a and b backward.  The byte floor of a call is the
corner lists, the faces and the field read once plus the output written (COTAN: and the weight positions); `floor_fraction` is that
floor at `--peak` GB/s (default 8000: HBM's nominal rate) over the measured time.  Prints one JSON line per (mesh, kind) and writes
them to --out.  Nothing is asserted."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import srz  # noqa: E402
from srz import abi, scenes  # noqa: E402

WARMUP, N_CH, SLOT = 5, 3, 11
KINDS = {"umbrella": abi.LAP_UMBRELLA, "graph": abi.LAP_GRAPH, "cotan": abi.LAP_COTAN}


def pct(xs, q):
    return float(np.percentile(np.asarray(xs), q))


def grid_mesh(n):
    """n x n vertices over the unit square with a wave in z, 2 (n - 1)^2 faces"""
    ys, xs = np.mgrid[0:n, 0:n].astype(np.float32) / np.float32(n - 1)
    pos = np.stack([xs.ravel(), ys.ravel(), 0.1 * np.sin(9.0 * xs.ravel()) * np.cos(7.0 * ys.ravel())], 1).astype(np.float32)
    j, i = np.mgrid[0:n - 1, 0:n - 1]
    a = (j * n + i).ravel()
    faces = np.concatenate([np.stack([a, a + 1, a + n + 1], 1), np.stack([a, a + n + 1, a + n], 1)]).astype(np.uint32)
    return pos, faces


def torch_operator(pos, faces, kind):
    """the weights precomputed -> (forward(x), backward(g)) over [V, C] tensors"""
    V = pos.shape[0]
    f = faces.long()
    v = torch.cat([f[:, k] for k in range(3)])
    a = torch.cat([f[:, (k + 1) % 3] for k in range(3)])
    b = torch.cat([f[:, (k + 2) % 3] for k in range(3)])
    n = torch.zeros(V, device=pos.device).index_add_(0, v, torch.full((len(v),), 2.0, device=pos.device))
    if kind == "cotan":
        p = pos[f]
        N = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
        d2 = (N * N).sum(1)
        ia = torch.where(d2 > 0, torch.rsqrt(torch.where(d2 > 0, d2, torch.ones_like(d2))), torch.zeros_like(d2))
        cot = [((p[:, (m + 1) % 3] - p[:, m]) * (p[:, (m + 2) % 3] - p[:, m])).sum(1) * ia for m in range(3)]
        wa = 0.5 * torch.cat([cot[(k + 2) % 3] for k in range(3)])
        wb = 0.5 * torch.cat([cot[(k + 1) % 3] for k in range(3)])
        d = torch.zeros(V, device=pos.device).index_add_(0, v, wa + wb)
    elif kind == "graph":
        wa = wb = torch.ones(len(v), device=pos.device)
        d = n
    else:
        wa = wb = (1.0 / n.clamp(min=1.0))[v]
        d = (n > 0).float()
    wa, wb, d = wa[:, None], wb[:, None], d[:, None]

    def forward(x):
        return (d * x).index_add_(0, v, -(wa * x[a] + wb * x[b]))

    def backward(g):
        gv = g[v]
        return (d * g).index_add_(0, a, -(wa * gv)).index_add_(0, b, -(wb * gv))
    return forward, backward


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    n_grid = int(args[args.index("--grid") + 1]) if "--grid" in args else 1024
    peak = float(args[args.index("--peak") + 1]) if "--peak" in args else 8000.0
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    wl = scenes.WORKLOADS["spot_bunny_phong_1080p"]()
    spot = next(m[0] for m in wl.meshes if "spot" in m[0])
    sv, sf = wl.scene.mesh(spot)
    meshes = {"spot": (np.asarray(sv, np.float32).reshape(-1, 8)[:, :3].copy(), np.asarray(sf, np.uint32).reshape(-1, 3)),
              f"grid{n_grid}": grid_mesh(n_grid)}
    rows = []
    for mname, (pos, faces) in meshes.items():
        v8 = np.zeros((len(pos), 8), np.float32)
        v8[:, :3] = pos
        ctx.mesh_upload(SLOT, v8, faces)
        V, F = len(pos), len(faces)
        d_pos, d_faces = torch.as_tensor(pos).cuda(), torch.as_tensor(faces.astype(np.int64)).cuda()
        x, g = torch.randn((V, N_CH), device="cuda"), torch.randn((V, N_CH), device="cuda")
        out, gx = torch.empty_like(x), torch.empty_like(x)
        for kname, kind in KINDS.items():
            t_fwd, t_bwd = torch_operator(d_pos, d_faces, kname)

            def fwd():
                ctx.mesh_laplacian(SLOT, x.data_ptr(), N_CH, N_CH, 1, kind, d_pos.data_ptr(), 3, out.data_ptr(), N_CH, sp)

            def both():
                fwd()
                ctx.mesh_laplacian_grad(SLOT, g.data_ptr(), N_CH, N_CH, 1, kind, d_pos.data_ptr(), 3, gx.data_ptr(), N_CH, sp)
            calls = {"forward": fwd, "forward_torch": lambda: t_fwd(x), "both": both, "both_torch": lambda: (t_fwd(x), t_bwd(g))}
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
            floor = 4 * ((V + 1) + 3 * F + 3 * F + 2 * V * N_CH + (3 * V if kname == "cotan" else 0))
            row = {"mesh": mname, "kind": kname, "vertices": V, "faces": F, "rounds": rounds, "channels": N_CH, "floor_bytes": floor,
                   "peak_gbs": peak}
            for k, evs in times.items():
                ms = [a.elapsed_time(b) for a, b in evs]
                row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90)}
            for k, calls_n in (("forward", 1), ("both", 2)):
                row[k + "_torch_over_device"] = row[k + "_torch"]["ms_median"] / row[k]["ms_median"]
                row[k + "_floor_fraction"] = calls_n * floor / (peak * 1e6) / row[k]["ms_median"]
            print(json.dumps(row), flush=True)
            rows.append(row)
        del x, g, out, gx, d_pos, d_faces
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
