"""Mipmapped texture sampling over a visibility buffer (srz_frameset_texture_mip / _texture_mip_grad, srz_texture_mip_build / _fold,
srz_frameset_interpolate_deriv) beside the bilinear pass, BASELINE configs 1-5, in one process, alternating.

    python tools/texture_mip_probe.py [rounds] [--configs 1,2,3,4,5] [--out FILE]

Per config: one frameset of bench.py's batch size (tools/vis_probe.py's sets), one visibility buffer of it, uv = interpolate and
uvd = interpolate_deriv of the frames' own uv.  The texture is the spot texture as float32 [H, W, 3], shared by every frame, CLAMP
mode, every level of its pyramid.  After 10 warm-up rounds the calls alternate, each timed with device events on its own; the median
of the rounds (default 20) is reported with p10 and p90.  The legs of one row are meant to be compared with each other: the mip
pass's forward, backward with the texel gradients only (gtex + gmip), with guv only and with both, against the same four legs of the
bilinear pass; and what only the mip pass has: interpolate_deriv, the build of the pyramid, the fold of the gradient pyramid.
Counted from the buffers, by the rule of include/srz.h restated in torch (float32, unfused: a pixel on a level boundary may fall on
the other side): the sampled pixels per level, and — by emulating the tile's table (tools/texture_probe.py's emulation: 2048 slots,
8 probes) once per (tile, level) as k_tex_mip_grad runs it, and once per tile as k_tex_grad does, on every EMULATE_EVERY-th tile
that samples anything — the share of adds whose texel finds no slot, for both passes.  Prints one JSON line per config and writes
them to --out.  Nothing is asserted."""
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
from texture_probe import EMULATE_EVERY, table_overflow, taps  # noqa: E402
from vis_probe import CONFIGS, frames_of, pct  # noqa: E402

C = 3
WARMUP = 10


def lod(uvd, tw, th, L):
    """the level rule in torch float32 → (l0 int64, f float32) [n, rows, W]"""
    ux, uy, vx, vy = uvd[:, 0], uvd[:, 1], uvd[:, 2], uvd[:, 3]
    fin = torch.isfinite(uvd).all(1)
    ax, ay, bx, by = ux * float(tw), vx * float(th), uy * float(tw), vy * float(th)
    r2 = torch.maximum(ax * ax + ay * ay, bx * bx + by * by)
    ok = fin & (r2 < float("inf"))
    rho = torch.sqrt(torch.where(ok, r2, torch.ones_like(r2)))
    m, e = torch.frexp(rho)
    l = e.to(torch.int64) - 1
    f = 2.0 * m - 1.0
    mag = ~(rho > 1.0)
    top = ~ok | (~mag & (l >= L - 1))
    l0 = torch.where(top, torch.full_like(l, L - 1), torch.where(mag, torch.zeros_like(l), l))
    return l0, torch.where(top | mag, torch.zeros_like(f), f)


def emulate(key, span):
    """key: tile * span + texel of every add of some tiles → (adds, adds whose texel finds no slot), each tile's table on its own"""
    k_np, t_np = (key % span + 1).cpu().numpy(), (key // span).cpu().numpy()
    order = np.argsort(t_np, kind="stable")
    k_np, t_np = k_np[order], t_np[order]
    adds = over = 0
    for chunk in np.split(k_np, np.flatnonzero(np.diff(t_np)) + 1):
        if len(chunk):
            adds += len(chunk)
            over += table_overflow(chunk)
    return adds, over


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
    L = srz.mip_levels(tw, th)
    mip_bytes = srz.mip_bytes(tw, th, C, 1, L)
    mip = torch.empty((mip_bytes // 4,), dtype=torch.float32, device="cuda")
    ctx.mip_build(tex.data_ptr(), tw, th, C, 1, L, mip.data_ptr(), mip_bytes, sp)
    rows = []
    for cfg, wl_name, n in CONFIGS:
        if cfg not in pick:
            continue
        frames = frames_of(cfg, wl_name, n, ctx)
        fs = ctx.frameset(frames)
        T = max(sum(len(t) for t in f.tris) for f in frames)
        uniq = {}
        a = np.zeros((n, T, 3, 2), np.float32)
        for i, f in enumerate(frames):  # (poses repeat: one concatenation per distinct frame)
            if id(f) not in uniq:
                uniq[id(f)] = np.concatenate([t["uv"] for t in f.tris]).astype(np.float32)
            a[i, :len(uniq[id(f)])] = uniq[id(f)]
        attr = torch.as_tensor(a).cuda()
        vis = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
        uv = torch.empty(fs.interpolate_shape(2), dtype=torch.float32, device="cuda")
        uvd = torch.empty(fs.interpolate_shape(4), dtype=torch.float32, device="cuda")
        fs.render_visibility(vis.data_ptr(), fs.out_bytes, F, sp)
        fs.interpolate(vis.data_ptr(), attr.data_ptr(), 2, n, T, uv.data_ptr(), fs.interpolate_bytes(2), F, sp)

        def deriv():
            fs.interpolate_deriv(vis.data_ptr(), attr.data_ptr(), 2, n, T, uvd.data_ptr(), fs.interpolate_bytes(4), F, sp)
        deriv()
        torch.cuda.synchronize()
        H, W = fs.local_rows, fs.width
        pixels = n * H * W
        ty, tx = (H + 31) // 32, (W + 31) // 32
        # ---- counted, eight frames at a time: pixels per level, the emulated overflow of both passes
        per_level, n_sampled, n_two = [0] * L, 0, 0
        emu = {"bilinear": [0, 0], "mip": [0, 0]}
        for f0 in range(0, n, 8):
            k = min(8, n - f0)
            ids = vis[f0:f0 + k].view(torch.int32)[:, 1].to(torch.int64) & 0x7fffffff
            own = (ids > 0) & (ids <= T)
            tile = ((torch.arange(k, device="cuda")[:, None, None] * ty + (torch.arange(H, device="cuda") // 32)[None, :, None]) * tx
                    + (torch.arange(W, device="cuda") // 32)[None, None, :])
            sampled, idx = taps(uv[f0:f0 + k], own, tw, th)
            l0, fr = lod(uvd[f0:f0 + k], tw, th, L)
            n_sampled += int(sampled.sum())
            n_two += int((sampled & (fr != 0)).sum())
            tiles = torch.unique(tile[sampled])[::EMULATE_EVERY]
            sel = sampled & torch.isin(tile, tiles)
            span = tw * th
            adds, over = emulate((tile[None].expand(4, -1, -1, -1)[:, sel] * span + idx[:, sel]).reshape(-1), span)
            emu["bilinear"][0] += adds
            emu["bilinear"][1] += over
            for l in range(L):
                per_level[l] += int((sampled & (l0 == l)).sum())
                part = sel & ((l0 == l) | ((l0 + 1 == l) & (fr != 0)))
                if not bool(part.any()):
                    continue
                wl, hl = max(1, tw >> l), max(1, th >> l)
                _, idx_l = taps(uv[f0:f0 + k], part, wl, hl)
                adds, over = emulate((tile[None].expand(4, -1, -1, -1)[:, part] * span + idx_l[:, part]).reshape(-1), span)
                emu["mip"][0] += adds
                emu["mip"][1] += over
            del ids, own, tile, sampled, idx, l0, fr, sel
        torch.cuda.empty_cache()
        # ---- timed
        out = torch.empty(fs.interpolate_shape(C), dtype=torch.float32, device="cuda")
        gout = torch.randn(fs.interpolate_shape(C), device="cuda")
        gtex, gmip, guv = torch.zeros_like(tex), torch.zeros_like(mip), torch.empty_like(uv)
        nb = fs.interpolate_bytes(C)
        v, u, d, x, m, g = vis.data_ptr(), uv.data_ptr(), uvd.data_ptr(), tex.data_ptr(), mip.data_ptr(), gout.data_ptr()

        def bwd(want_tex, want_uv):
            return lambda: fs.texture_grad(v, u, g, x, tw, th, C, 1, abi.TEX_CLAMP, gtex.data_ptr() if want_tex else None,
                                           guv.data_ptr() if want_uv else None, F, sp)

        def mip_bwd(want_tex, want_uv):
            return lambda: fs.texture_mip_grad(v, u, d, g, x, m, tw, th, C, 1, abi.TEX_CLAMP, L, gtex.data_ptr() if want_tex else None,
                                               gmip.data_ptr() if want_tex else None, guv.data_ptr() if want_uv else None, F, sp)
        calls = {"forward": lambda: fs.texture(v, u, x, tw, th, C, 1, abi.TEX_CLAMP, out.data_ptr(), nb, F, sp),
                 "mip_forward": lambda: fs.texture_mip(v, u, d, x, tw, th, C, 1, abi.TEX_CLAMP, m, L, out.data_ptr(), nb, F, sp),
                 "backward_gtex": bwd(True, False), "mip_backward_gtex": mip_bwd(True, False),
                 "backward_guv": bwd(False, True), "mip_backward_guv": mip_bwd(False, True),
                 "backward_both": bwd(True, True), "mip_backward_both": mip_bwd(True, True),
                 "interpolate_deriv": deriv,
                 "mip_build": lambda: ctx.mip_build(x, tw, th, C, 1, L, m, mip_bytes, sp),
                 "mip_fold": lambda: ctx.mip_fold(gmip.data_ptr(), mip_bytes, tw, th, C, 1, L, gtex.data_ptr(), sp)}
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
        row = {"config": cfg, "workload": wl_name or "config1_256", "frames": n, "rounds": rounds, "channels": C, "texture": [tw, th], "levels": L,
               "pixels": pixels, "sampled_pixels": n_sampled, "sampled_per_level": per_level, "two_level_pixels": n_two,
               "emulated_adds": emu["bilinear"][0], "emulated_overflow_share": emu["bilinear"][1] / max(1, emu["bilinear"][0]),
               "mip_emulated_adds": emu["mip"][0], "mip_emulated_overflow_share": emu["mip"][1] / max(1, emu["mip"][0])}
        for k, evs in times.items():
            ms = [a_.elapsed_time(b_) for a_, b_ in evs]
            row[k] = {"ms_median": float(np.median(ms)), "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90), "ms_series": [round(t_, 4) for t_ in ms]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        if out_path:  # (after every config: a long run leaves what it has)
            with open(out_path, "w") as fh:
                json.dump(rows, fh, indent=1)
        fs.close()
        del vis, uv, uvd, out, gout, guv, attr
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
