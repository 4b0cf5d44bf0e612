"""Dev probe of the tile-sparse exchange (srz_frameset_sparse_pack / _unpack): one GPU plays every rank r of N in {2, 4, 8} for
configs 2, 4 and 5.  Not a test and not bench.py.

Per (config, N) it renders every rank's bands of the same frames (FUSED_CLEAR, one frameset per rank), packs each rank's message
and times it with device events, then unpacks every peer's message into rank 0's gathered buffer and times that.  It prints

  * the message bytes / the dense shard bytes (mean and max over the ranks),
  * pack and unpack ms (median of 5) and their HBM fraction (bytes moved / ms against the 8 TB/s peak),
  * the predicted step of an N-GPU job at F frames per GPU (config 2: 256), scaled from the measured frames:
    link = the largest message / 153 GB/s per peer link (xGMI: every rank sends its message once to each peer over that peer's own
    link — the figure DESIGN.md §6 uses, not measured on hardware here), local = render + pack + unpack on this GPU's HBM;
    step = max(link, local), frames/s = F·N / step — beside the dense in-place exchange's shard / 153 GB/s.

Its own time limit (--limit seconds, SIGALRM): no retries.  Usage:  python tools/sparse_exchange_probe.py [--configs 2,4,5] [--out FILE]
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "software-rasterizer_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

LINK_GBS, PEAK_TBS = 153.0, 8.0
# frames of the whole job rendered per (config, N) and frames per GPU the prediction is scaled to
SETS = {2: (64, 1024, 256), 4: (16, 2048, 32), 5: (4, 4096, 8)}


def frames_of(cfg, n, size):
    import scenes
    build = {2: lambda i: scenes.config2(i, size=size), 4: lambda i: scenes.config4(i, size=size), 5: lambda i: scenes.config5(i, size=size)}[cfg]
    return [build(i) for i in range(n)]


def timed(torch, fn, reps=5):
    s = torch.cuda.current_stream()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def run(cfg, world, frames, what, torch, srz, abi, parallel, tex):
    s = torch.cuda.current_stream().cuda_stream
    msgs, stats, keep = [], [], None
    h = frames[0].height
    for r in range(world):
        ctx = srz.Context(0, r, world)
        ctx.texture_upload(0, tex)
        fs = ctx.frameset(frames)
        planes = torch.empty((world,) + fs.out_shape, dtype=torch.float32, device="cuda")
        fs.render(planes[r].data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s)           # (warm: pool sizing, clear grid)
        render_ms = timed(torch, lambda: fs.render(planes[r].data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, s))
        if what == abi.EXCHANGE_PLANES:
            g = planes
        else:
            g = torch.empty((world, len(frames), 1, fs.local_rows, frames[0].width * 3), dtype=torch.uint8, device="cuda")
            fs.resolve8(planes[r].data_ptr(), g[r].data_ptr(), g[r].numel(), s)
        cap = fs.sparse_capacity(what)
        msg = torch.empty(cap, dtype=torch.uint8, device="cuda")
        pack_ms = timed(torch, lambda: fs.sparse_pack(g[r].data_ptr(), msg.data_ptr(), cap, what, s))
        torch.cuda.synchronize()
        n_t, n_tab, nbytes = parallel.sparse_header(msg)
        shard = fs.exchange_bytes(what)
        lay = parallel.sparse_layout(len(frames), fs.local_rows // 32, frames[0].width, 4 if what == abi.EXCHANGE_PLANES else 1)
        pack_bytes = 2 * n_t * lay["tile_bytes"] + 8 * n_tab + 4 * n_tab    # tiles read + written, tile_info read, table written
        stats.append({"rank": r, "render_ms": render_ms, "pack_ms": pack_ms, "msg_bytes": nbytes, "shard_bytes": shard,
                      "touched": n_t, "tiles": n_tab, "pack_hbm_frac": pack_bytes / (pack_ms * 1e-3) / (PEAK_TBS * 1e12)})
        msgs.append(msg)
        if r == 0:
            keep = (ctx, fs, g)
        else:
            del planes, g
            fs.close(), ctx.close()
    ctx, fs, g = keep
    recv = torch.stack(msgs).contiguous()
    cap = msgs[0].numel()
    del msgs
    row_bytes = frames[0].width * (16 if what == abi.EXCHANGE_PLANES else 3)
    mine = sum(r1 - r0 for (_, _, r0, r1) in parallel.band_rows(h, 0, world))
    written = len(frames) * (h - mine) * row_bytes   # (the peers' real rows)
    read = sum(st["touched"] for st in stats[1:]) * lay["tile_bytes"]
    ms = timed(torch, lambda: fs.sparse_unpack(recv.data_ptr(), cap, g.data_ptr(), what, s))
    unpack = {"ms": ms, "hbm_frac": (written + read) / (ms * 1e-3) / (PEAK_TBS * 1e12), "write_tbs": written / (ms * 1e-3) / 1e12}
    fs.close(), ctx.close()
    del g, recv
    torch.cuda.empty_cache()
    return stats, unpack, written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,4,5")
    ap.add_argument("--worlds", default="2,4,8")
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: (print("sparse_exchange_probe: time limit", flush=True), os._exit(3)))
    signal.alarm(a.limit)
    import torch
    import scenes
    import srz
    from srz import abi, parallel
    tex = scenes.spot_texture()
    res = []
    t0 = time.time()
    for cfg in (int(c) for c in a.configs.split(",")):
        n_frames, size, f_gpu = SETS[cfg]
        frames = frames_of(cfg, n_frames, size)
        for world in (int(w) for w in a.worlds.split(",")):
            for what, name in ((abi.EXCHANGE_PLANES, "planes"), (abi.EXCHANGE_BGR8, "bgr8")):
                stats, unpack, written = run(cfg, world, frames, what, torch, srz, abi, parallel, tex)
                frac = [st["msg_bytes"] / st["shard_bytes"] for st in stats]
                scale = f_gpu * world / n_frames       # measured frames → F frames per GPU
                link = max(st["msg_bytes"] for st in stats) * scale / (LINK_GBS * 1e9) * 1e3
                dense_link = stats[0]["shard_bytes"] * scale / (LINK_GBS * 1e9) * 1e3
                render = max(st["render_ms"] for st in stats) * scale
                pack = max(st["pack_ms"] for st in stats) * scale
                un = unpack["ms"] * scale
                step = max(link, render + pack + un)
                row = {"config": cfg, "N": world, "exchange": name, "frames_measured": n_frames, "size": size, "F_per_gpu": f_gpu,
                       "msg_frac_mean": statistics.mean(frac), "msg_frac_max": max(frac),
                       "touched_frac": sum(st["touched"] for st in stats) / sum(st["tiles"] for st in stats),
                       "pack_ms": statistics.mean(st["pack_ms"] for st in stats), "pack_hbm_frac": statistics.mean(st["pack_hbm_frac"] for st in stats),
                       "unpack_ms": unpack["ms"], "unpack_hbm_frac": unpack["hbm_frac"], "unpack_write_tbs": unpack["write_tbs"],
                       "render_ms_max": max(st["render_ms"] for st in stats),
                       "predicted": {"link_ms": link, "render_ms": render, "pack_ms": pack, "unpack_ms": un, "step_ms": step,
                                     "frames_per_s": f_gpu * world / step * 1e3, "dense_link_ms": dense_link,
                                     "dense_frames_per_s": f_gpu * world / max(dense_link, render) * 1e3}}
                res.append(row)
                print(json.dumps(row), flush=True)
    print(f"sparse_exchange_probe: {len(res)} rows in {time.time() - t0:.0f} s", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
