"""The lighting pass over a visibility buffer (srz_frameset_light / _light_grad) beside the same rule written in torch ops, on
BASELINE config 2's set (256 frames of 1024^2), at 1 and 3 lights, in one process, alternating.

    python tools/light_probe.py [rounds] [--frames N] [--lights 1,3] [--out FILE]

One frameset of bench.py's batch size (tools/vis_probe.py's set: poses of one mesh), one visibility buffer of it, the normal planes
interpolate writes for the frames' own per-vertex normals, position planes from a linear ramp over the frame, albedo planes of
uniform noise, one parameter frame shared by every frame, p = 5.  After 5 warm-up rounds the calls alternate, each timed with device
events on its own; the median of the rounds (default 10) is reported with p10 and p90: light, light_grad with the three planes only,
light_grad with the planes and gpar, and — the only comparison there is, nothing of this pass existed before — the rule in torch
float32 ops (lightref.torch_rule's formulation: about 40 elementwise launches per light over [n, 3, H, W] planes), forward alone and
forward + autograd backward to the planes and the parameters.  The torch leg holds many [n, 3, H, W] temporaries: --frames
(default 256) lowers the set where memory does not allow it, and the torch leg is skipped (null) if it runs out of memory.
Prints one JSON line per light count and writes them to --out.  Nothing is asserted: there is no timing gate, because nothing
exists to regress against."""
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
from srz import abi  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s: device-to-device copies
P, WARMUP = 5, 5


def timed(s, calls, rounds):
    for _ in range(WARMUP):
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


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 10
    n_frames, lights, out_path = 256, (1, 3), None
    if "--frames" in args:
        n_frames = int(args[args.index("--frames") + 1])
    if "--lights" in args:
        lights = tuple(int(c) for c in args[args.index("--lights") + 1].split(","))
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
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
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda") * (2.0 / H) - 1, torch.arange(W, device="cuda") * (2.0 / W) - 1, indexing="ij")
    pos = torch.stack([xs, ys, 0.1 * xs - 0.2 * ys]).expand(n_frames, 3, H, W).contiguous()
    kd = torch.rand(fs.interpolate_shape(3), device="cuda") * 0.9 + 0.1
    gout = torch.randn(fs.interpolate_shape(3), device="cuda")
    out, gn, gp, gk = (torch.empty_like(nrm) for _ in range(4))
    ids = vis.view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
    n_own = int(((ids > 0) & (ids <= T)).sum())
    del ids
    torch.cuda.synchronize()
    pixels, nb, rows = n_frames * H * W, fs.interpolate_bytes(3), []
    for L in lights:
        par = torch.as_tensor(lightref.make_params(7, L)).cuda().reshape(1, -1).contiguous()
        gpar = torch.empty_like(par)
        wb = fs.light_work_bytes(L)
        work = torch.empty(wb // 4, dtype=torch.float32, device="cuda")

        def bwd(with_par):
            return lambda: fs.light_grad(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), kd.data_ptr(), par.data_ptr(), L, 1, P, gout.data_ptr(),
                                         gn.data_ptr(), gp.data_ptr(), gk.data_ptr(), gpar.data_ptr() if with_par else None,
                                         work.data_ptr() if with_par else None, wb if with_par else 0, F, sp)
        calls = {"light": lambda: fs.light(vis.data_ptr(), nrm.data_ptr(), pos.data_ptr(), kd.data_ptr(), par.data_ptr(), L, 1, P,
                                           out.data_ptr(), nb, F, sp),
                 "light_grad_planes": bwd(False), "light_grad_planes_gpar": bwd(True)}
        row = {"config": cfg, "frames": n_frames, "rounds": rounds, "lights": L, "p": P, "pixels": pixels, "owned_pixels": n_own,
               # the id plane, nine words read and three written per owned pixel; backward: twelve read, nine written
               "forward_floor_ms": (4 * pixels + (36 + 12) * n_own) / COPY_RATE * 1e3,
               "backward_floor_ms": (4 * pixels + (48 + 36) * n_own) / COPY_RATE * 1e3}
        row.update(timed(s, calls, rounds))
        pieces = [par[0, 9:].reshape(L, 6).clone().requires_grad_(True)] + [par[0, i:i + 3].clone().requires_grad_(True) for i in (0, 3, 6)]

        def torch_fwd():
            with torch.no_grad():
                return lightref.torch_rule(nrm, pos, kd, *[t.detach() for t in pieces], P)

        def torch_both():
            planes = [t.detach().requires_grad_(True) for t in (nrm, pos, kd)]
            for t in pieces:
                t.grad = None
            lightref.torch_rule(*planes, *pieces, P).backward(gout)
        for name, fn in (("torch_forward", torch_fwd), ("torch_forward_backward", torch_both)):  # (each on its own: the second may not fit)
            try:
                row.update(timed(s, {name: fn}, max(2, rounds // 3)))
            except torch.OutOfMemoryError:
                row[name] = None
            torch.cuda.empty_cache()
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    fs.close()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
