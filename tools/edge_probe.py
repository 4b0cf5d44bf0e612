"""The mesh edge terms on the device (srz_mesh_edges, srz_mesh_edges_grad) beside the same two terms in plain torch on the same device,
on the spot mesh and a generated grid of about a million vertices, in one process, alternating.

    python tools/edge_probe.py [rounds] [--grid 1024] [--peak GB/s] [--out FILE]

Per mesh and term (length, dihedral), one position set: after 5 warm-up rounds the legs alternate, each timed with device events on
its own; the median of the rounds (default 20) is reported with p10 and p90.  Legs: the forward call; the forward and the backward
call; and the torch formulation of both — what a user writes today: an edge table built on the host from the faces (not timed),
gathers through it, and autograd's backward, which ends in index_add_ (float atomics) onto the vertices.  The torch legs work per
UNDIRECTED edge and per adjacent face pair — half the elements of the device's per-(face, edge) field on a closed mesh, the cheaper
way round for torch.  The byte floor of a forward call is the corner lists, the faces and the positions read once plus the output
written; `forward_floor_fraction` is that floor at `--peak` GB/s (default 8000: HBM's nominal rate) over the measured time.  Prints one
JSON line per (mesh, term) and writes them to --out.  Nothing is asserted."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import srz  # noqa: E402
from srz import abi, scenes  # noqa: E402

WARMUP, SLOT = 5, 11
KINDS = {"length": abi.EDGE_LENGTH, "dihedral": abi.EDGE_DIHEDRAL}


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


def edge_table(faces, n_verts):
    """the host-built table: (edges [E, 2] the undirected edges, pairs [P, 2] the two faces of every edge that has exactly two)"""
    f = faces.astype(np.int64)
    a, b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]]), np.concatenate([f[:, 2], f[:, 0], f[:, 1]])  # edge j joins i[j + 1], i[j + 2]
    face = np.tile(np.arange(len(f)), 3)
    key = np.minimum(a, b) * n_verts + np.maximum(a, b)
    order = np.argsort(key, kind="stable")
    key, face = key[order], face[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    size = np.diff(np.concatenate([first, [len(key)]]))
    two = first[size == 2]
    return np.stack([key[first] // n_verts, key[first] % n_verts], 1), np.stack([face[two], face[two + 1]], 1)


def torch_terms(pos, faces, edges, pairs):
    """-> {term: function of the positions} in torch ops, differentiable by autograd"""
    def length(p):
        d = p[edges[:, 1]] - p[edges[:, 0]]
        return torch.sqrt((d * d).sum(1))

    def dihedral(p):
        q = p[faces]
        n = torch.nn.functional.normalize(torch.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0], dim=1), dim=1)
        return 1.0 - (n[pairs[:, 0]] * n[pairs[:, 1]]).sum(1)
    return {"length": length, "dihedral": dihedral}


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
        edges, pairs = (torch.as_tensor(t).cuda() for t in edge_table(faces, V))
        d_pos, d_faces = torch.as_tensor(pos).cuda(), torch.as_tensor(faces.astype(np.int64)).cuda()
        out, gout = torch.empty((F, 3), device="cuda"), torch.randn((F, 3), device="cuda")
        work, gpos = torch.empty((F, 3), device="cuda"), torch.empty((V, 3), device="cuda")
        terms = torch_terms(d_pos, d_faces, edges, pairs)
        for kname, kind in KINDS.items():
            term = terms[kname]
            with torch.no_grad():
                g_t = torch.randn_like(term(d_pos))
            leaf = d_pos.clone().requires_grad_(True)

            def fwd():
                ctx.mesh_edges(SLOT, d_pos.data_ptr(), 3, 1, kind, out.data_ptr(), 3, sp)

            def both():
                fwd()
                ctx.mesh_edges_grad(SLOT, d_pos.data_ptr(), 3, 1, kind, gout.data_ptr(), 3, work.data_ptr(), gpos.data_ptr(), sp)

            def fwd_torch():
                with torch.no_grad():
                    return term(d_pos)

            def both_torch():
                return torch.autograd.grad(term(leaf), leaf, g_t)
            calls = {"forward": fwd, "forward_torch": fwd_torch, "both": both, "both_torch": both_torch}
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
            floor = 4 * ((V + 1) + 3 * F + 3 * F + 3 * V + 3 * F)
            row = {"mesh": mname, "term": kname, "vertices": V, "faces": F, "edges": int(len(edges)), "pairs": int(len(pairs)), "rounds": rounds,
                   "floor_bytes": floor, "peak_gbs": peak}
            for k, evs in times.items():
                ms = [a.elapsed_time(b) for a, b in evs]
                row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90)}
            for k in ("forward", "both"):
                row[k + "_torch_over_device"] = row[k + "_torch"]["ms_median"] / row[k]["ms_median"]
            row["forward_floor_fraction"] = floor / (peak * 1e6) / row["forward"]["ms_median"]
            print(json.dumps(row), flush=True)
            rows.append(row)
        del out, gout, work, gpos, d_pos, d_faces, edges, pairs, terms
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
