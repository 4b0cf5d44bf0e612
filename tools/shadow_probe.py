"""The shadow-map lookup over a visibility buffer (srz_frameset_shadow / _shadow_grad) beside the same rule written in torch ops, on
BASELINE config 2's set (256 frames of 1024^2), hard and soft, in one process, alternating.

    python tools/shadow_probe.py [rounds] [--frames N] [--out FILE]

One frameset of bench.py's batch size (tools/vis_probe.py's set: poses of one mesh), one visibility buffer of it.  The map of frame
i is plane 0 of that buffer itself (a light looking along the camera: a 1024^2 map per frame, +inf where nobody is), the
coordinates are each pixel's own place moved by (0.37, 0.61) texels — so the four taps are four different texels and both fractions
are in play — and its own depth: neighbouring depths differ by little, so with the soft width (a twentieth of the depth range) most
corners are on the ramp and add to gmap, which is the expensive case.  After 5 warm-up rounds the calls alternate, each timed with
device events on its own; the median of the rounds (default 10) is reported with p10 and p90: shadow, shadow_grad with gsc only, with
gmap only, and with both — and the only comparison there is, nothing of this pass existed before: the rule in torch float32 ops
(shadowref.torch_rule: four gathers and about thirty elementwise launches over [n, H, W] planes), forward alone and forward +
autograd backward to the map and the coordinates.  --frames (default 256) lowers the set where memory does not allow it, and a torch
leg is skipped (null) if it runs out of memory.  Prints one JSON line per width and writes them to --out.  Nothing is asserted:
there is no timing gate, because nothing exists to regress against."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

import shadowref  # noqa: E402
import srz  # noqa: E402
from light_probe import COPY_RATE, timed  # noqa: E402
from srz import abi  # noqa: E402
from vis_probe import CONFIGS, frames_of  # noqa: E402


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 10
    n_frames, out_path = 256, None
    if "--frames" in args:
        n_frames = int(args[args.index("--frames") + 1])
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    sp, F = s.cuda_stream, abi.FUSED_CLEAR
    cfg, wl_name, _ = next(c for c in CONFIGS if c[0] == 2)
    frames = frames_of(cfg, wl_name, n_frames, ctx)
    fs = ctx.frameset(frames)
    T = max(f.n_tris for f in frames)
    vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render_visibility(vis.data_ptr(), fs.out_bytes, F, sp)
    H, W = fs.local_rows, fs.width
    ids = vis.view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
    own = (ids > 0) & (ids <= T)
    n_own = int(own.sum())
    del ids
    zmap = vis[:, 0].contiguous()
    z = torch.where(own, zmap, torch.zeros_like(zmap))
    z_lo, z_hi = float(zmap[own].min()), float(zmap[own].max())
    del own
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    sc = torch.stack([(xs + 0.37).expand(n_frames, H, W), (ys + 0.61).expand(n_frames, H, W), z], 1).contiguous()
    del z
    gout = torch.randn(fs.interpolate_shape(1), device="cuda")
    out, gsc, gmap = torch.empty_like(gout), torch.empty_like(sc), torch.zeros_like(zmap)
    torch.cuda.synchronize()
    pixels, nb, rows = n_frames * H * W, fs.interpolate_bytes(1), []
    bias = 0.0
    for width in (0.0, 0.05 * (z_hi - z_lo)):
        def bwd(want_map, want_sc):
            return lambda: fs.shadow_grad(vis.data_ptr(), sc.data_ptr(), gout.data_ptr(), zmap.data_ptr(), W, H, n_frames, bias, width,
                                          gmap.data_ptr() if want_map else None, gsc.data_ptr() if want_sc else None, F, sp)
        calls = {"shadow": lambda: fs.shadow(vis.data_ptr(), sc.data_ptr(), zmap.data_ptr(), W, H, n_frames, bias, width, out.data_ptr(), nb, F, sp),
                 "shadow_grad_gsc": bwd(False, True), "shadow_grad_gmap": bwd(True, False), "shadow_grad_both": bwd(True, True)}
        row = {"config": cfg, "frames": n_frames, "rounds": rounds, "width": width, "depth_range": [z_lo, z_hi], "pixels": pixels,
               "owned_pixels": n_own,
               # the id plane, then per owned pixel three words read, four gathered and one written; backward: one more read (gout),
               # three written (gsc) and / or up to four texels added to (gmap: the table combines a tile's adds first)
               "forward_floor_ms": (4 * pixels + (12 + 16 + 4) * n_own) / COPY_RATE * 1e3,
               "backward_gsc_floor_ms": (4 * pixels + (12 + 16 + 4 + 12) * n_own) / COPY_RATE * 1e3}
        row.update(timed(s, calls, rounds))
        lit = out[:, 0]
        row["lit_mean"] = float(lit.sum() / max(n_own, 1))
        row["gmap_nonzero"] = int((gmap != 0).sum())
        gmap.zero_()

        def torch_fwd():
            with torch.no_grad():
                return shadowref.torch_rule(zmap, sc[:, 0], sc[:, 1], sc[:, 2], bias, width)

        def torch_both():
            m = zmap.detach().requires_grad_(True)
            c = sc.detach().requires_grad_(True)
            shadowref.torch_rule(m, c[:, 0], c[:, 1], c[:, 2], bias, width).backward(gout[:, 0])
        for name, fn in (("torch_forward", torch_fwd), ("torch_forward_backward", torch_both)):  # (each on its own: the second may not fit)
            try:
                row.update(timed(s, {name: fn}, max(2, rounds // 3)))
            except torch.OutOfMemoryError:
                row[name] = None
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
