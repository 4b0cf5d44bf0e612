"""The vertex stage's backward (srz_sceneset_vertex_grad) and the set's positions (srz_frameset_positions), BASELINE configs 2-5 as
scenesets (bench.py's: meshes resident, the vertex stage on the device), in one process, alternating.

    python tools/vertexgrad_probe.py [rounds] [--configs 2,3,4,5] [--out FILE]

Per config: one sceneset of bench.py's batch size and a dense random gpos [n, T, 3, 3].  After 10 warm-up rounds the calls alternate,
each timed with device events on its own; the median of the rounds (default 20) is reported with p10 and p90: vertex_grad over every
mesh of the workload (one call per mesh) for gverts only, gdraw only and both; positions; and the formulation a user writes in torch
today — per mesh an index_add_ of the corners' gpos onto the vertices, the transform and its derivative in batched torch arithmetic,
a sum over the vertices for the matrices.  Beside them the byte floor of the gverts pass: 36 B of gpos per referenced triangle and
frame, 12 B of vertex and 12 B of output per vertex and frame, at the device-to-device copy rate.  Prints one JSON line per config
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
from srz import scenes  # noqa: E402
from vis_probe import CONFIGS, pct  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s: device-to-device copies
WARMUP = 10


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    pick = {2, 3, 4, 5}
    out_path = None
    if "--configs" in args:
        pick = {int(c) for c in args[args.index("--configs") + 1].split(",")}
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    rows = []
    for cfg, wl_name, n in CONFIGS:
        if cfg not in pick or wl_name is None:
            continue
        wl = scenes.WORKLOADS[wl_name]()
        wl.upload_meshes(ctx)
        uniq = [wl.scene_frame(i) for i in range(min(n, 36))]
        wl.upload_textures(ctx)
        sframes = [uniq[i % len(uniq)] for i in range(n)]
        fs = ctx.frameset(sframes)
        draws = [[int(f._draws[j].mesh_id) for j in range(f.c.n_draws)] for f in sframes]
        assert all(d == draws[0] for d in draws)  # (the workloads draw the same meshes in every frame)
        slots = sorted(set(draws[0]))
        n_verts, n_faces = {m: ctx.mesh_sizes[m][0] for m in slots}, {m: ctx.mesh_sizes[m][1] for m in slots}
        T, D = sum(n_faces[m] for m in draws[0]), len(draws[0])
        gpos = torch.randn((n, T, 3, 3), device="cuda")
        pos = torch.empty((n, T, 3, 3), dtype=torch.float32, device="cuda")
        gverts = {m: torch.zeros((n, n_verts[m], 3), device="cuda") for m in slots}
        gdraw = torch.zeros((n, D, 18), device="cuda")
        # what the torch formulation reads: the meshes and matrices as tensors
        verts, faces = {}, {}
        for i, (mname, _, _, _, _) in enumerate(wl.meshes):
            v, f = wl.scene.mesh(mname)
            verts[i] = torch.as_tensor(np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1, 8)[:, :3])).cuda()
            faces[i] = torch.as_tensor(np.asarray(f, np.int64).reshape(-1)).cuda()
        mvp = torch.as_tensor(np.array([[list(f._draws[j].ndc_mvp) for j in range(D)] for f in sframes], np.float32)).cuda()  # [n, D, 16]
        zs = torch.as_tensor(np.array([f.c.zscale for f in sframes], np.float32)).cuda()

        def torch_formulation():
            out_v = {m: torch.zeros((n, n_verts[m], 3), device="cuda") for m in slots}
            out_d = torch.zeros((n, D, 18), device="cuda")
            first = 0
            for j, m in enumerate(draws[0]):
                F = n_faces[m]
                G = torch.zeros((n, n_verts[m], 3), device="cuda").index_add_(1, faces[m], gpos[:, first:first + F].reshape(n, 3 * F, 3))
                M = mvp[:, j].view(n, 4, 4).transpose(1, 2)  # rows
                P = verts[m]
                r = torch.einsum("nic,vc->nvi", M[:, :, :3], P) + M[:, None, :, 3]
                inv = 1.0 / r[..., 3]
                X, Y, Q = r[..., 0] * inv, r[..., 1] * inv, r[..., 2] * inv
                gq = G[..., 2] * zs[:, None]
                g3 = -(G[..., 0] * X + G[..., 1] * Y + gq * Q) * inv
                g = torch.stack([G[..., 0] * inv, G[..., 1] * inv, gq * inv, g3], -1)  # [n, V, 4]
                out_v[m] += torch.einsum("nic,nvi->nvc", M[:, :, :3], g)
                out_d[:, j, :12] = torch.einsum("nvi,vc->nci", g, P).reshape(n, 12)
                out_d[:, j, 12:16] = g.sum(1)
                out_d[:, j, 16] = (G[..., 2] * Q).sum(1)
                out_d[:, j, 17] = G[..., 2].sum(1)
                first += F
            return out_v, out_d

        def vg(want_v, want_d):
            def f():
                for m in slots:
                    fs.vertex_grad(m, gpos.data_ptr(), T, gverts[m].data_ptr() if want_v else None, gdraw.data_ptr() if want_d else None, D, sp)
            return f
        calls = {"gverts": vg(1, 0), "gdraw": vg(0, 1), "both": vg(1, 1), "positions": lambda: fs.positions(T, pos.data_ptr(), pos.numel() * 4, sp),
                 "torch": torch_formulation}
        try:  # the batched intermediates may not fit beside the set: the leg is then left out
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
        n_v = sum(n_verts[m] for m in slots)
        row = {"config": cfg, "workload": wl_name, "frames": n, "rounds": rounds, "triangles_per_frame": T, "draws_per_frame": D,
               "vertices": n_v, "floor_ms_gverts": n * (36 * T + 24 * n_v) / COPY_RATE * 1e3, "floor_ms_positions": n * 72 * T / COPY_RATE * 1e3}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90), "ms_series": [round(x, 4) for x in ms]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del gpos, pos, gverts, gdraw, verts, faces, mvp
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
