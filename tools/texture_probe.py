"""Caller textures over a visibility buffer (srz_frameset_texture / _texture_grad), BASELINE configs 1-5, in one process, alternating.

    python tools/texture_probe.py [rounds] [--configs 1,2,3,4,5] [--out FILE]

Per config: one frameset of bench.py's batch size (tools/vis_probe.py's sets: poses of one mesh), one visibility buffer of it and
its uv planes (gbuffer(UV)).  The texture is the spot texture as float32 [H, W, 3], shared by every frame, CLAMP mode.  After 10
warm-up rounds the calls alternate, each timed with device events on its own; the median of the rounds (default 20) is reported
with p10 and p90: the forward pass, the backward with gtex only, with guv only and with both, interpolate at C = 3 (the yardstick:
the same planes written, 9 floats gathered per owned pixel where the texture pass gathers 12), and the formulation a user writes in
torch today (torch.nn.functional.grid_sample, bilinear, border padding, and its autograd to the texture and to the grid).
Counted from the buffers, by the rule of include/srz.h restated in torch: the sampled pixels, the distinct (tile, texel) pairs —
the global float adds k_tex_grad's design implies are pairs * C, beside 4 * C per sampled pixel — and, by emulating the tile's
table (2048 slots, 8 probes, the multiplicative hash of csrc/srz_kernels.hip; one insertion order: the device's is unspecified)
on every EMULATE_EVERY-th tile that samples anything, the share of adds whose texel found no slot.  Prints one JSON line per
config and writes them to --out.  Nothing is asserted."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import scenes as test_scenes  # noqa: E402
import srz  # noqa: E402
from srz import abi  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

COPY_RATE, ADD_RATE = 6.29e12, 1.3e12  # bytes / s: device-to-device copies; global float adds, chip-wide
C = 3
WARMUP = 10
TG_SLOT_BITS, TG_PROBES = 11, 8
EMULATE_EVERY = 16


def taps(uv, own, tw, th):
    """CLAMP taps of the rule in float32 → (sampled [n, rows, W] bool, the four texel indices [4, n, rows, W] int64)"""
    def axis(c, n):
        f = torch.clamp(c * float(n) - 0.5, 0.0, float(n - 1))
        i0 = torch.floor(f).to(torch.int64)
        return i0, torch.clamp(i0 + 1, max=n - 1)
    u, v = uv[:, 0], uv[:, 1]
    sampled = own & torch.isfinite(u) & torch.isfinite(v)
    u, v = torch.where(sampled, u, torch.zeros_like(u)), torch.where(sampled, v, torch.zeros_like(v))
    x0, x1 = axis(u, tw)
    y0, y1 = axis(v, th)
    return sampled, torch.stack([y0 * tw + x0, y0 * tw + x1, y1 * tw + x0, y1 * tw + x1])


def table_overflow(keys):
    """keys: the texel indices + 1 of one tile's adds (int64, with repeats) → the adds whose texel finds no slot, inserting the
    distinct texels in ascending order of the probe round"""
    uniq, counts = np.unique(keys, return_counts=True)
    slots = 1 << TG_SLOT_BITS
    h = ((uniq.astype(np.uint64) * np.uint64(0x9e3779b1)) & np.uint64(0xffffffff)) >> np.uint64(32 - TG_SLOT_BITS)
    taken = np.zeros(slots, bool)
    left = np.arange(len(uniq))
    for p in range(TG_PROBES):
        if not len(left):
            break
        s = ((h[left] + np.uint64(p)) & np.uint64(slots - 1)).astype(np.int64)
        free = ~taken[s]
        _, first = np.unique(s[free], return_index=True)  # one texel per free slot
        placed = np.flatnonzero(free)[first]
        taken[s[placed]] = True
        keep = np.ones(len(left), bool)
        keep[placed] = False
        left = left[keep]
    return int(counts[left].sum())


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
    tex = torch.as_tensor(np.ascontiguousarray(test_scenes.spot_texture(), np.float32)).cuda()
    th, tw = tex.shape[0], tex.shape[1]
    rows = []
    for cfg, wl_name, n in CONFIGS:
        if cfg not in pick:
            continue
        frames = frames_of(cfg, wl_name, n, ctx)
        fs = ctx.frameset(frames)
        T = max(sum(len(t) for t in f.tris) for f in frames)
        vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
        uv = torch.empty(fs.gbuffer_shape(abi.GB_UV), dtype=torch.float32, device="cuda")
        fs.render_visibility(vis.data_ptr(), fs.out_bytes, F, sp)
        fs.gbuffer(vis.data_ptr(), uv.data_ptr(), fs.gbuffer_bytes(abi.GB_UV), abi.GB_UV, F, sp)
        torch.cuda.synchronize()
        H, W = fs.local_rows, fs.width
        ids = vis.view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
        own = (ids > 0) & (ids <= T)
        pixels = n * H * W
        # ---- counted: sampled pixels, (tile, texel) pairs, the emulated overflow
        sampled, idx = taps(uv, own, tw, th)
        n_sampled = int(sampled.sum())
        ty, tx = (H + 31) // 32, (W + 31) // 32
        tile = ((torch.arange(n, device="cuda")[:, None, None] * ty + (torch.arange(H, device="cuda") // 32)[None, :, None]) * tx
                + (torch.arange(W, device="cuda") // 32)[None, None, :])
        pairs, emu_adds, emu_over, busiest = 0, 0, 0, 0
        for f0 in range(0, n, 8):  # (eight frames at a time: the keys of a 4096^2 batch do not fit at once)
            m = sampled[f0:f0 + 8]
            key = (tile[f0:f0 + 8][None].expand(4, -1, -1, -1)[:, m] * (tw * th) + idx[:, f0:f0 + 8][:, m]).reshape(-1)
            uniq = torch.unique(key)
            pairs += int(uniq.numel())
            per_tile = torch.unique(uniq // (tw * th), return_counts=True)
            busiest = max(busiest, int(per_tile[1].max()) if per_tile[1].numel() else 0)
            pick_tiles = per_tile[0][::EMULATE_EVERY]
            sel = torch.isin(key // (tw * th), pick_tiles)
            k_np, t_np = (key[sel] % (tw * th) + 1).cpu().numpy(), (key[sel] // (tw * th)).cpu().numpy()
            order = np.argsort(t_np, kind="stable")
            k_np, t_np = k_np[order], t_np[order]
            for chunk in np.split(k_np, np.flatnonzero(np.diff(t_np)) + 1):
                if len(chunk):
                    emu_adds += len(chunk)
                    emu_over += table_overflow(chunk)
            del key, uniq, sel
        del idx, tile
        torch.cuda.empty_cache()
        # ---- timed
        out = torch.empty(fs.interpolate_shape(C), dtype=torch.float32, device="cuda")
        gout = torch.randn(fs.interpolate_shape(C), device="cuda")
        gtex, guv = torch.zeros_like(tex), torch.empty_like(uv)
        attr = torch.randn((T, 3, C), device="cuda")
        nb = fs.interpolate_bytes(C)
        tex_t = tex.permute(2, 0, 1)[None].contiguous()  # [1, C, H, W] for grid_sample

        def bwd(want_tex, want_uv):
            return lambda: fs.texture_grad(vis.data_ptr(), uv.data_ptr(), gout.data_ptr(), tex.data_ptr(), tw, th, C, 1, abi.TEX_CLAMP,
                                           gtex.data_ptr() if want_tex else None, guv.data_ptr() if want_uv else None, F, sp)

        def torch_forward():
            grid = (uv.permute(0, 2, 3, 1) * 2.0 - 1.0).nan_to_num(0.0, 0.0, 0.0)
            return torch.nn.functional.grid_sample(tex_t.expand(n, -1, -1, -1), grid, mode="bilinear", padding_mode="border",
                                                   align_corners=False) * own[:, None]

        def torch_backward():
            t, g = tex_t.clone().requires_grad_(True), (uv.permute(0, 2, 3, 1) * 2.0 - 1.0).nan_to_num(0.0, 0.0, 0.0).requires_grad_(True)
            o = torch.nn.functional.grid_sample(t.expand(n, -1, -1, -1), g, mode="bilinear", padding_mode="border", align_corners=False)
            o.backward(gout * own[:, None])
            return t.grad, g.grad
        calls = {"forward": lambda: fs.texture(vis.data_ptr(), uv.data_ptr(), tex.data_ptr(), tw, th, C, 1, abi.TEX_CLAMP, out.data_ptr(), nb, F, sp),
                 "backward_gtex": bwd(True, False), "backward_guv": bwd(False, True), "backward_both": bwd(True, True),
                 "interpolate_c3": lambda: fs.interpolate(vis.data_ptr(), attr.data_ptr(), C, 1, T, out.data_ptr(), nb, F, sp),
                 "torch_forward": torch_forward, "torch_backward": torch_backward}
        for k in ("torch_forward", "torch_backward"):  # the planes of grid_sample may not fit beside the set: the leg is then left out
            try:
                calls[k]()
            except torch.cuda.OutOfMemoryError:
                del calls[k]
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
        row = {"config": cfg, "workload": wl_name or "config1_256", "frames": n, "rounds": rounds, "channels": C, "texture": [tw, th],
               "pixels": pixels, "owned_pixels": int(own.sum()), "sampled_pixels": n_sampled, "tile_texel_pairs": pairs,
               "busiest_tile_texels": busiest, "atomic_bytes": pairs * C * 4, "atomic_bytes_per_corner_adds": n_sampled * 4 * C * 4,
               "emulated_adds": emu_adds, "emulated_overflow_share": (emu_over / emu_adds) if emu_adds else 0.0,
               "atomic_floor_ms": pairs * C * 4 / ADD_RATE * 1e3,
               "forward_floor_ms": (4 * pixels + (8 + 16 * C) * n_sampled + 4 * C * pixels) / COPY_RATE * 1e3,
               "backward_floor_ms": (4 * pixels + 8 * n_sampled + 4 * C * n_sampled) / COPY_RATE * 1e3}
        for k, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90), "ms_series": [round(x, 4) for x in ms]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        fs.close()
        del vis, uv, out, gout, guv, attr, own, ids, sampled
        torch.cuda.empty_cache()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
