#!/usr/bin/env python3
"""bench.py — frames/s (+ Mfragments/s) of the MI355X raster + fragment-shade stage on BASELINE.json's configs[1]
(spot_triangulated_good.obj, 1024x1024, TEXTURE shader + 2 point lights).

A "step" = one pass of the hot path (setup → tile binning → visibility raster → shading, the fused clear beside them) over
one batch of F synthetic frames per GPU (frame i is the spot mesh rotated by 10*i degrees, the reference's own per-frame
variation), inputs (post-MVP triangle streams, lights, texture) already resident in HBM, output = the reference's
framebuffer layout (z + 3 planar float colour planes per frame) in HBM.

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python bench.py --gpus N ...          (N > 1 without a launcher: bench.py starts the N ranks itself — launch_ranks below)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run measures the headline only: set-up, priming + W warm-up steps, K timed steps (`value`, `ms_per_step`), the line.
--dump-outputs DIR writes a seeded sample of the last timed step's framebuffer (dump_outputs).  --full measures the rest too:
the unprimed region, the counting pass, the one-stream per-kernel split and, at N = 1 after the headline config and outside
its timed region, the other GPU configs of BASELINE.json (configs[2..4], whole frames on one GPU), configs[1] at scope "draw"
(vertex stage timed too), the README loop, the emulated N-GPU shards and the CPU baseline: `configs` in the JSON.

N > 1: one process per GPU; every frame's 32-row bands are dealt round-robin to the ranks (srz_set_shard), each rank
renders its bands of F*N frames (per-GPU pixel work fixed → weak scaling), and the exchange north_star names — ONE in-place
RCCL all-gather over xGMI behind the C ABI (srz_frameset_allgather_inplace) — reassembles every full framebuffer on every
rank.  The exchange of step k runs on its own stream while step k+1 renders (double-buffered).
WHAT is exchanged at N > 1: the headline (`value`) exchanges the four float planes (16 B/px: z + the three
m_channels — what draw() leaves, and what north_star's parity is stated on: z bit-exact) at every N, so rounds compare; the same
run then times the exchange of display()'s 8-bit image (src/Render.cpp:61-62: every rank resolves its bands on the device,
k_resolve8, and all-gathers 3 B/px) and reports it beside the headline in `multi_gpu.bgr8`, never as `value`.

Prints ONE compact JSON line (rank 0) of < 6 KB as the LAST line of stdout; every note and the full per-workload records go to
bench_details.json next to this script and to stderr (emit()).  PyTorch is only plumbing here (device buffers, streams, the rendezvous).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)
N_SIMD, SCLK_HZ = 1024, 2.4e9  # 256 CUs x 4 SIMD-32, max shader clock (same guide)
HBM_MEASURED_COPY_GBS = 6290.0
XGMI_LINK_GBS = 153.0  # per link, per direction (7 links per GPU)
# the other GPU configs of BASELINE.json, whole frames on one GPU: (workload, frames per step, steps)
EXTRA_CASES = [("spot_bunny_phong_1080p", 128, 20), ("spot_x16_texture_2048", 128, 20), ("spot_x8_overdraw_4096", 64, 20),
               ("readme_spot_crate_1024", 256, 20),  # (+ the scene of the reference's one published raster figure)
               # configs[1] away from the benchmark's own shading parameters: 3 lights, p = 32 (FAST builds of k_shade for other
               # counts / exponents), p = 7.5 (the generic build), the BUMP shader
               ("spot_texture_1024_3lights", 256, 10), ("spot_texture_1024_p32", 256, 10), ("spot_texture_1024_p7.5", 256, 10),
               ("spot_bump_1024", 256, 10)]


# workloads whose summary goes into roofline.per_config (the part of the line the driver's parser keeps): BASELINE configs 3 / 4 / 5,
# the scene of the reference's one published figure, configs[1] at scope draw, the exponent variant the generic build used to serve
# (workload, frames per step, steps) rendered once more in the tolerance mode (SRZ_OPT_APPROX_SHADE): `<workload>:approx` rows
APPROX_CASES = [("spot_texture_1024", 256, 10), ("spot_bunny_phong_1080p", 128, 10), ("spot_x16_texture_2048", 128, 10),
                ("spot_x8_overdraw_4096", 64, 10)]
PER_CONFIG = ("spot_bunny_phong_1080p", "spot_x16_texture_2048", "spot_x8_overdraw_4096", "readme_spot_crate_1024", "spot_texture_1024_p7.5")
HBM_BYTES = 288e9  # per MI355X
PRIME_TO = 26      # untimed renders in front of every timed region, the --warmup steps included (time_single_gpu): the clock ramp
                   # after idle, and the 24 renders over which a frameset measures the grid of its clear (srz_api.hip, ClearTune)


def kernel_source_hash():
    """sha256 of the DEVICE CODE of the library that runs (the .hip_fatbin section of software-rasterizer_amd/libsrz.so: every
    kernel as compiled for gfx950), first 16 hex digits: bench.py writes it into its line, profiles/summarize.py stores the one
    of the profiled run in profiles/pmc_counters.json next to the counters, and a bench line of a build with OTHER kernels reports
    traffic: null + traffic_stale instead of another code version's counters.  (The compiled kernels, not the source text and
    not the host code around them: a comment or a host-side edit does not invalidate a profile; a kernel, flag or compiler
    change does.)"""
    import hashlib
    import struct
    lib = os.environ.get("SRZ_LIB_PATH", os.path.join(REPO, "software-rasterizer_amd", "libsrz.so"))
    try:
        b = open(lib, "rb").read()
    except OSError:
        return "no-library"
    try:  # ELF64 little-endian section walk
        shoff, = struct.unpack_from("<Q", b, 0x28)
        shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
        sec = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize) for i in range(shnum)]
        str_off = sec[shstrndx][4]
        for name, _t, _f, _a, off, size, *_ in sec:
            end = b.index(b"\0", str_off + name)
            if b[str_off + name:end] == b".hip_fatbin":
                return "fb-" + hashlib.sha256(b[off:off + size]).hexdigest()[:16]
    except (struct.error, ValueError, IndexError):
        pass
    return hashlib.sha256(b).hexdigest()[:16]  # (no such section: the whole file)


def launch_ranks(n_ranks, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as FRESH child processes (the same command the driver
    uses: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <argv>), relay rank 0's JSON line as this
    process's own last line of stdout and return the children's exit status.  Called BEFORE this process imports torch or
    touches HIP (a process that has initialised the GPU must not start others by exec, and must not hold the GPU while the
    ranks need it); the children are a process group of their own, killed as a group if they outlive the time limit."""
    import signal
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, SRZ_BENCH_LAUNCHED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (dmabuf IPC: RCCL between processes needs it on this host driver)
    limit = float(os.environ.get("SRZ_BENCH_LAUNCH_TIMEOUT", "1500"))
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=None, text=True, env=env, start_new_session=True)
    line = None

    def on_alarm(signum, frame):
        raise TimeoutError
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(int(limit))
    try:
        for out in p.stdout:
            if out.startswith('{"metric"'):
                line = out.strip()
            else:
                sys.stderr.write(out)
        rc = p.wait()
    except TimeoutError:
        os.killpg(p.pid, signal.SIGKILL)  # (exactly the group started above)
        p.wait()
        sys.stderr.write(f"bench.py: the {n_ranks} ranks did not finish within {limit:.0f} s; killed\n")
        return 124
    finally:
        signal.alarm(0)
    if line is not None:
        print(line, flush=True)
    if rc == 0 and line is None:
        sys.stderr.write("bench.py: the ranks exited without a JSON line\n")
        return 1
    return rc


def readme_loop():
    """The reference's own published protocol (README.md:619-642: 1024x1024, spot + crate scene, 100 warm-up + 1000 frames, clear()
    per frame, the angle rotated every frame, std::chrono around draw(); ONE frame in flight — latency, not throughput) through
    the C++ API: software-rasterizer_amd/build/loop_bench (tools/cpp/loop_bench.cpp, built by __graft_entry__.build()), run as a
    child process BEFORE this process touches the GPU.  → its JSON record, or {"error": ...}"""
    import subprocess
    exe = os.path.join(REPO, "software-rasterizer_amd", "build", "loop_bench")
    if not os.path.exists(exe):  # (normally built by __graft_entry__.build(); the GPU box has the same toolchain)
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "software-rasterizer_amd"), "build/loop_bench"], capture_output=True)
    if not os.path.exists(exe):
        return {"scope": "readme_loop", "error": f"{exe} not built (run __graft_entry__.build())"}
    try:
        r = subprocess.run([exe, REPO, "1000", "readme"], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            return {"scope": "readme_loop", "error": f"loop_bench exited {r.returncode}: {r.stderr[-300:]}"}
        rec = json.loads(r.stdout.strip().splitlines()[-1])
    except Exception as e:  # noqa: BLE001  (an extra must never cost the headline line)
        return {"scope": "readme_loop", "error": repr(e)}
    rec.update({"workload": "readme_spot_crate_1024", "scope": "readme_loop", "width": 1024, "height": 1024, "warmup_frames": 100,
                "protocol": "README.md:619-642 of the reference: one frame in flight, clear() + matrices + draw() per frame"})
    return rec


def host_cpu_info():
    """→ (logical CPUs this process may run on, where that number comes from, CPU model string)"""
    n, src = os.cpu_count() or 1, "os.cpu_count"
    try:
        aff = len(os.sched_getaffinity(0))
        if aff < n:
            n, src = aff, "sched_getaffinity"
    except (AttributeError, OSError):
        pass
    try:  # cgroup v2 CPU quota ("max 100000" = none)
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max" and int(q) // int(per) >= 1 and int(q) // int(per) < n:
            n, src = int(q) // int(per), "cgroup cpu.max"
    except (OSError, ValueError):
        pass
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return n, src, model


def cpu_baseline(workload_name, budget_s=12.0, max_frames=100000):
    """The CPU oracle's OpenMP entry points (oracle/srz_oracle.c: the same per-pixel code as the checker) timed on this host's
    cores on a bounded sample of the same workload, in the two shapes a CPU can run it and in two builds:
      rows   — one frame at a time, its rows dealt in bands to the threads (the reference's own structure: it parallelises
               inside a frame, `src/Rasterizer.cpp:217`),
      frames — whole frames dealt to the threads, each with private planes (the throughput shape, = what the GPU batch does);
      -O2 (the checker's build) and -O3 -mavx2 -mfma with the vectoriser on (the reference's own target, README.md:608).
    Team sizes are tried up to every CPU this process may use (cgroup quota / affinity / count: `host_cpus_source`).  The best
    of the four is `value`; all are in `sample`.  kind = "port": the reference itself cannot be built in this image (DESIGN.md,
    Oracle).  This is the ONLY place bench.py touches oracle/."""
    sys.path.insert(0, REPO)
    from oracle import oracle  # noqa: E402
    from srz import scenes
    wl = scenes.WORKLOADS[workload_name]()
    frames = [wl.frame(i) for i in range(36)]
    oracle.lib(True)  # (load the -O3 build before the textures are registered with every loaded build)
    for slot, tex in enumerate(wl.texture_arrays):
        oracle.texture_set(slot, tex)
    planes = oracle.new_planes(wl.width, wl.height)
    ncpu, ncpu_src, model = host_cpu_info()
    cands = sorted({t for t in (4, 8, 16, 32, 64, 96, 128, 192, 256, ncpu) if 1 <= t <= ncpu})
    share = budget_s / 4.0
    results = {}
    for fast in (False, True):
        tag = "O3" if fast else "O2"
        # ---- rows: pick the team size that serves one frame best (short trials), then a bounded run ----------------------
        best_t, best_rate = cands[0], 0.0
        for t in cands:
            rc, _ = oracle.draw_omp(frames[0], planes, band=8, threads=t, fast=fast)  # warm-up at this team size
            assert rc == 0
            k, t0 = 0, time.perf_counter()
            while k < 200 and time.perf_counter() - t0 < share / (3.0 * len(cands)):
                oracle.draw_omp(frames[k % len(frames)], planes, band=8, threads=t, fast=fast)
                k += 1
            rate = k / (time.perf_counter() - t0)
            if rate > best_rate:
                best_t, best_rate = t, rate
        n, t0, used = 0, time.perf_counter(), best_t
        while n < max_frames and (time.perf_counter() - t0) < share * 2.0 / 3.0:
            rc, used = oracle.draw_omp(frames[n % len(frames)], planes, band=8, threads=best_t, fast=fast)  # FUSED_CLEAR: clear + draw
            n += 1
        dt = time.perf_counter() - t0
        results[f"rows_{tag}"] = {"rate": n / dt, "threads": used, "frames": n, "seconds": dt}
        # ---- frames: whole frames per thread; calibrate the team size on ~2 frames per thread, then a bounded run ---------
        fbest_t, fbest_rate = cands[0], 0.0
        for t in cands:
            k = 2 * t
            t0 = time.perf_counter()
            rc, _ = oracle.draw_frames_omp(frames, k, threads=t, fast=fast)
            assert rc == 0
            rate = k / (time.perf_counter() - t0)
            if rate > fbest_rate:
                fbest_t, fbest_rate = t, rate
        fn = int(min(max_frames, max(fbest_t, fbest_rate * share * 0.6)))
        t0 = time.perf_counter()
        rc, used = oracle.draw_frames_omp(frames, fn, threads=fbest_t, fast=fast)
        dt = time.perf_counter() - t0
        results[f"frames_{tag}"] = {"rate": fn / dt, "threads": used, "frames": fn, "seconds": dt}
    t1 = time.perf_counter()
    oracle.draw(frames[0], planes, want_stats=False)
    single = time.perf_counter() - t1
    best = max(results, key=lambda k: results[k]["rate"])
    return {"value": results[best]["rate"], "unit": "frames/s", "cores": int(results[best]["threads"]), "kind": "port",
            "shape": best, "cpu_model": model, "host_cpus": ncpu, "host_cpus_source": ncpu_src, "thread_candidates": cands,
            "sample": f"{workload_name}, clear+draw per frame, rotation 10 deg/frame; " +
                      "; ".join(f"{k}: {v['frames']} frames in {v['seconds']:.1f} s on {v['threads']} threads = {v['rate']:.0f} frames/s"
                                for k, v in results.items()) +
                      f"; single-thread -O2 oracle: {1.0 / single:.1f} frames/s (rows = bands of 8 rows of one frame per thread, "
                      "frames = whole frames per thread; O2 = the checker's build, O3 = -O3 -mavx2 -mfma -ftree-vectorize)",
            "sample_short": f"{workload_name}: clear+draw per frame, {results[best]['frames']} frames in {results[best]['seconds']:.1f} s on "
                            f"{results[best]['threads']} threads ({best}: best of rows/frames x O2/O3, ~{budget_s:.0f} s in all); 1 thread: {1.0 / single:.1f} frames/s",
            "variants": {k: {"frames_per_sec": v["rate"], "threads": v["threads"]} for k, v in results.items()}}


def pct(xs, q):
    xs = sorted(xs)
    if not xs:
        return None
    i = q * (len(xs) - 1)
    lo, hi = int(i), min(int(i) + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (i - lo)


class Case:
    """One workload resident on this rank's GPU: frameset, counters, output buffers."""

    def __init__(self, ctx, torch, workload, frames_per_gpu, scope, world, n_out=1, stats=True):
        import srz
        from srz import scenes
        self.torch, self.ctx, self.name, self.scope, self.world = torch, ctx, workload, scope, world
        wl = scenes.WORKLOADS[workload]()
        n_frames = frames_per_gpu * world
        uniq = [wl.frame(i) for i in range(min(n_frames, 36))]  # 36 distinct rotations (10 deg steps)
        frames = [uniq[i % len(uniq)] for i in range(n_frames)]
        wl.upload_textures(ctx)
        self.tris_per_frame = frames[0].n_tris
        if scope == "draw":  # same frames, given as meshes + matrices: the device runs the vertex stage every step
            wl.upload_meshes(ctx)
            suniq = [wl.scene_frame(i) for i in range(min(n_frames, 36))]
            frames = [suniq[i % len(suniq)] for i in range(n_frames)]
        self.frames, self._lanes = frames, {}
        self.fs = ctx.frameset(frames)
        # counting variant of the kernels, run once, outside every timed region (stats=False: not run, self.stats is None); the
        # algorithmic bytes need its count of textured pixels, so they are None without it too
        self.stats = self.fs.stats() if stats else None
        self.algo_bytes = self.fs.algorithmic_bytes() if stats else None
        self.n_frames, self.frames_per_gpu = n_frames, frames_per_gpu
        self.out = [torch.empty(self.fs.out_shape, dtype=torch.float32, device="cuda") for _ in range(n_out)]

    _streams = []  # the lanes' streams, made ONCE per process and shared by every case: HIP deals new streams round-robin onto a
                   # few hardware queues, and a later case's fresh pair can land on one queue (its lanes then take turns instead of
                   # overlapping: seen as 1.32 instead of 1.08 ms per step on one of the configs[] entries)

    def lanes(self, n):
        """the same frames as n lane framesets on n streams (srz.parallel.LaneRenderer), built once per n"""
        from srz import parallel
        while len(Case._streams) < n:
            Case._streams.append(self.torch.cuda.Stream())
        if n not in self._lanes:
            self._lanes[n] = parallel.LaneRenderer(self.ctx, self.frames, n, streams=Case._streams[:n])
        return self._lanes[n]

    def close(self):
        self.out = None
        self.fs.close()
        for lr in self._lanes.values():
            lr.close()
        self.torch.cuda.empty_cache()


DUMP_SEED = 0
DUMP_PIXELS = 1 << 20  # 1 M pixels x 4 planes: values 16 MB + their non-finite codes 16 MB + indices as float64 8 MB, below 64 MB


def dump_outputs(out_dir, out):
    """--dump-outputs DIR: what the timed path handed its caller after its last step, as .npy files, so that two builds can be
    compared output for output.  out: that output on the device, [..., P, rows, cols] (frames, or ranks x frames, of P planes),
    seen as [A, P, B]: A frames or frame shards of P planes of B pixels.  Every file holds finite numbers only, yet loses nothing:
      framebuffer_sample.npy           float32 [S, P]  every plane of S pixels, a non-finite value (z of an uncovered pixel: +inf) as 0
      framebuffer_sample_nonfinite.npy float32 [S, P]  what stood there instead: 0 finite, 1 +inf, -1 -inf, 2 NaN
      framebuffer_sample_index.npy     float64 [S]     the pixels' flat indices a * B + b, ascending
    S pixels = every pixel when there are at most DUMP_PIXELS, else DUMP_PIXELS of them drawn without replacement by numpy's
    generator seeded with DUMP_SEED — the same pixels for the same arguments."""
    import numpy as np
    import torch
    planes = out.flatten(0, -4).flatten(-2)
    n_a, _, n_b = planes.shape
    n = n_a * n_b
    if n <= DUMP_PIXELS:
        idx = np.arange(n, dtype=np.int64)
    else:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n, DUMP_PIXELS, replace=False))
    i = torch.from_numpy(idx).to(planes.device)
    sample = planes[i // n_b, :, i % n_b].float()
    code = torch.zeros_like(sample)
    code[torch.isposinf(sample)], code[torch.isneginf(sample)], code[torch.isnan(sample)] = 1.0, -1.0, 2.0
    sample = torch.where(code == 0, sample, torch.zeros_like(sample))
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "framebuffer_sample.npy"), sample.cpu().numpy())
    np.save(os.path.join(out_dir, "framebuffer_sample_nonfinite.npy"), code.cpu().numpy())
    np.save(os.path.join(out_dir, "framebuffer_sample_index.npy"), idx.astype(np.float64))


def time_single_gpu(case, steps, warmup, fence, lanes=2, unprimed=False, split=True):
    """W warm-up steps, then EXACTLY K steps bracketed by fences.

    A step renders the whole batch: `lanes` runs of whole frames, each on a stream of its own (srz.parallel.LaneRenderer —
    the lanes are not synchronised with each other, so consecutive steps overlap at their edges; every step is complete
    before the closing fence).  Inside the timed region every render carries two HIP events on its stream (start / end of
    its launch set); the device time of the region is the span from the first start to the last end.  The per-kernel split
    comes from a short pass AFTER the timed region (split=True: one_stream_split) — the batch in one piece on one stream, with
    two more events per render: each event is a barrier in the stream, so the split is kept out of the throughput measurement.
    On return case.out[0] holds what the last timed step computed unless the split ran (it renders into the same buffer)."""
    torch, ctx, fs = case.torch, case.ctx, case.fs
    from srz import abi
    out = case.out[0]
    if lanes <= 0:  # auto: two lanes when each still holds a batch (measured: +4..8 % at >= 64 frames per step, -2 % at 32)
        lanes = 2 if case.n_frames >= 64 else 1
    lr = case.lanes(lanes)
    # priming (not counted as warm-up; reported as `priming_steps`): the first ~13 renders after idle run up to 10 % slower
    # (clock ramp, first touch of the list pool: tools/step_series_probe.py prints the series), and renders 6..23 of a frameset are the
    # ones that try the candidate grids of its clear (srz_api.hip, srz_frameset::ClearTune) — a short --warmup ends inside both.
    # With --full the headline case therefore times TWO regions: first exactly what the arguments say from idle (W untimed steps,
    # K timed: `value_unprimed` / `ms_per_step_unprimed`), then W more untimed steps and K timed ones in the steady state (`value`);
    # a plain run and the other workloads make sure of PRIME_TO untimed renders in all and time one region.
    unprimed_dt = None
    if unprimed:  # the driver's arguments taken literally: W untimed steps from idle, then K timed ones (`value_unprimed`); they
        for _ in range(warmup):  # also serve as the priming of the region that follows
            lr.render(out.data_ptr(), abi.FUSED_CLEAR)
        fence()
        tu = time.perf_counter()
        for _ in range(steps):
            lr.render(out.data_ptr(), abi.FUSED_CLEAR)
        fence()
        unprimed_dt = time.perf_counter() - tu
        done = warmup + steps
    else:
        done = 0
    extra = max(0, PRIME_TO - warmup - done)
    for _ in range(extra):
        lr.render(out.data_ptr(), abi.FUSED_CLEAR)
    priming = done + extra  # renders in front of the timed region beyond its own --warmup
    for _ in range(warmup):
        lr.render(out.data_ptr(), abi.FUSED_CLEAR)
    fence()
    ctx.set_kernel_timing(1)
    ctx.kernel_time_ms(reset=True)
    t0 = time.perf_counter()
    for k in range(steps):
        lr.render(out.data_ptr(), abi.FUSED_CLEAR)
    fence()
    dt = time.perf_counter() - t0
    samples, span_ms = ctx.kernel_time_samples()
    kt = ctx.kernel_time_ms(reset=True)
    n_l = len(lr.sets)
    per_step = [max(samples[i:i + n_l]) for i in range(0, len(samples) - n_l + 1, n_l)]  # a step ends with its slowest lane
    kt["lane_launch_ms"], kt["total_ms"], kt["lanes"] = kt["total_ms"], span_ms / max(steps, 1), n_l
    # grid of each lane's side-stream clear as its frameset measured it during the priming renders (srz_api.hip, ClearTune) and whether
    # the measurement was complete before the timed region
    dc = [s_.debug_counters() for s_ in lr.sets]
    kt["clear_wgs"], kt["clear_tuned"] = [d_["clear_wgs"] for d_ in dc], all(d_["clear_tuned"] for d_ in dc)
    kt["unprimed_dt"], kt["priming_steps"] = unprimed_dt, priming
    if split:
        one_stream_split(case, steps, fence, kt)
    ctx.set_kernel_timing(0)
    return dt, kt, per_step


def one_stream_split(case, steps, fence, kt):
    """Not part of the measurement: the batch of time_single_gpu in ONE piece on ONE stream (whole-launch time, then the
    per-kernel split), run after its timed region; adds one_stream_ms_per_step, bin_ms / raster_ms / shade_ms and
    split_total_ms to kt.  Renders into case.out[0]."""
    torch, ctx, fs = case.torch, case.ctx, case.fs
    from srz import abi
    out = case.out[0]
    ctx.set_kernel_timing(1)  # (as in the timed region: a render carries its two events)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for _ in range(PRIME_TO):  # (this frameset measures the grid of its clear too)
            fs.render(out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream.cuda_stream)
        fence()
        n1 = min(steps, 20)
        t1 = time.perf_counter()
        for k in range(n1):
            fs.render(out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream.cuda_stream)
        fence()
        kt["one_stream_ms_per_step"] = (time.perf_counter() - t1) / n1 * 1e3
        ctx.set_kernel_timing(2)
        ctx.kernel_time_ms(reset=True)
        for k in range(min(steps, 5)):
            fs.render(out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream.cuda_stream)
        fence()
        split = ctx.kernel_time_ms(reset=True)
    ctx.set_kernel_timing(0)
    for k in ("bin_ms", "raster_ms", "shade_ms"):
        kt[k] = split[k]
    kt["split_total_ms"] = split["total_ms"]


def make_comm(ctx, dist, torch, rank, world):
    """The exchange's RCCL communicator behind the C ABI (srz_comm_create), decided COLLECTIVELY: ncclCommInitRank is a
    collective, so a rank must not enter it unless every rank will, and all ranks must end up on the same exchange path.
      1. rank-local: can this rank load librccl and make an id at all?  (srz_comm_unique_id — no communication)
      2. all-reduce(MIN) of that flag over torch.distributed: one failure → nobody calls srz_comm_create
      3. rank 0's id is broadcast, every rank calls srz_comm_create
      4. all-reduce(MIN) of the results: one failure → every rank drops its communicator and all exchange through
         torch.distributed's RCCL instead (+ the HIP de-interleave)
    → (comm or None, note or None)"""
    import srz
    err = None
    try:
        my_id = srz.Comm.unique_id()
    except Exception as e:  # noqa: BLE001
        my_id, err = None, f"librccl not usable on rank {rank}: {e}"
    ok = torch.tensor([1 if my_id is not None else 0], dtype=torch.int32, device="cuda")
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok[0]) == 0:
        return None, (err or "librccl not usable on some rank") + "; exchange through torch.distributed instead"
    ids = [my_id if rank == 0 else None]
    dist.broadcast_object_list(ids, src=0)
    comm = None
    try:
        comm = srz.Comm(ctx, ids[0], rank, world)
    except Exception as e:  # noqa: BLE001
        err = f"srz_comm_create failed on rank {rank}: {e}"
    ok = torch.tensor([1 if comm is not None else 0], dtype=torch.int32, device="cuda")
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok[0]) == 0:
        if comm is not None:
            comm.close()
        return None, (err or "srz_comm_create failed on some rank") + "; exchange through torch.distributed instead"
    return comm, None


def time_multi_gpu(case, comm, dist, steps, warmup, fence, exchange="planes", no_overlap=False, layout="shards", rank=0,
                   exchange_alone=True):
    """N > 1 (also runs at world 1 with a one-rank communicator — tests/test_gpu_exchange.py drives it there, so the scaling
    run is not this code's first execution): render on one stream, exchange on another, double-buffered: the exchange of step
    k runs while step k+1 renders.  layout "shards": the rank renders (or resolves) straight into its slot of the gathered
    buffer and the exchange is ONE in-place all-gather, no second pass (result in rank-major shard order,
    srz_frameset_allgather_inplace); "rows": all-gather into a staging buffer + one HIP de-interleave pass (row-major frames).
    exchange_alone=False skips the pass that times the exchange without a render beside it (its figures are then None).
    → (dt, kernel times, per-step list, multi dict)"""
    from srz import abi, parallel
    torch, ctx, fs, world = case.torch, case.ctx, case.fs, case.world
    what = abi.EXCHANGE_PLANES if exchange == "planes" else abi.EXCHANGE_BGR8
    bpr = fs.local_rows // 32 if world > 1 else None
    rows_full = bpr * world * 32 if world > 1 else fs.local_rows
    shard_shape, dtype = ((case.n_frames, 4, fs.local_rows, fs.width), torch.float32) if exchange == "planes" else \
                         ((case.n_frames, 1, fs.local_rows, fs.width * 3), torch.uint8)  # (display()'s image: one "plane" of W*3 bytes per row)
    gathered = [torch.empty((world,) + shard_shape, dtype=dtype, device="cuda") for _ in range(2)]
    if layout == "shards":  # this rank's shard IS its slot of the gathered buffer
        shard = [g[rank] for g in gathered]
        full = gathered
        planes = shard if exchange == "planes" else case.out
    else:
        shard = case.out if exchange == "planes" else [torch.empty(shard_shape, dtype=dtype, device="cuda") for _ in range(2)]
        full = [torch.empty((case.n_frames, shard_shape[1], rows_full, shard_shape[3]), dtype=dtype, device="cuda") for _ in range(2)]
        planes = case.out
    rq = parallel.TorchQueue()
    xq = rq if no_overlap else parallel.TorchQueue()

    def render(b):
        fs.render(planes[b].data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, rq.handle)
        if exchange == "bgr8":
            fs.resolve8(planes[b].data_ptr(), shard[b].data_ptr(), shard[b].numel(), rq.handle)

    def do_exchange(b):
        if layout == "shards":
            if comm is not None:
                fs.allgather_inplace(comm, gathered[b].data_ptr(), what, xq.handle)
            elif world > 1:  # (torch.distributed's RCCL on the current = exchange stream, in place)
                dist.all_gather_into_tensor(gathered[b].view(-1), shard[b].reshape(-1))
        elif comm is not None:
            fs.allgather(comm, shard[b].data_ptr(), gathered[b].data_ptr(), full[b].data_ptr(), what, xq.handle)
        else:  # (torch.distributed's RCCL on the current = exchange stream, then the HIP de-interleave)
            dist.all_gather_into_tensor(gathered[b].view(-1), shard[b].reshape(-1))
            fs.deinterleave(gathered[b].data_ptr(), full[b].data_ptr(), what, xq.handle)

    pipe = parallel.ExchangePipeline(render, do_exchange, rq, xq)
    for _ in range(max(0, PRIME_TO - warmup) + warmup):  # (priming + warm-up: see time_single_gpu)
        pipe.step()
    pipe.drain()
    fence()
    ctx.set_kernel_timing(2)  # (per-kernel split: the exchange dominates an N > 1 step, two more events do not matter)
    ctx.kernel_time_ms(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        pipe.step()
    pipe.drain()
    fence()
    dt = time.perf_counter() - t0
    kt = ctx.kernel_time_ms(reset=True)
    ctx.set_kernel_timing(False)
    # the exchange alone (no render beside it), same buffers: what the overlap has to hide
    x_alone = None
    if exchange_alone:
        fence()
        t1 = time.perf_counter()
        for k in range(steps):
            xq.submit(lambda b=k % 2: do_exchange(b))
        xq.drain()
        fence()
        x_alone = (time.perf_counter() - t1) / steps * 1e3
    if dist is not None:
        tt = torch.tensor([dt, (x_alone or 0.0) * 1e-3], dtype=torch.float64, device="cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt[0])
        if x_alone is not None:
            x_alone = float(tt[1]) * 1e3
    step_ms = dt / steps * 1e3
    shard_bytes = shard[0].numel() * shard[0].element_size()
    multi = {"exchange": exchange, "layout": layout, "second_pass": layout != "shards", "behind_c_abi": comm is not None, "overlapped": not no_overlap,
             "step_ms": step_ms, "render_ms_per_step": kt["total_ms"], "exchange_alone_ms_per_step": x_alone,
             "hidden_ms_per_step": max(0.0, kt["total_ms"] + x_alone - step_ms) if x_alone is not None else None,
             "bytes_sent_per_rank_per_step": shard_bytes, "bytes_received_per_rank_per_step": (world - 1) * shard_bytes,
             "predicted_exchange_ms_at_xgmi_peak": shard_bytes / (XGMI_LINK_GBS * 1e9) * 1e3,
             "note": "exchange = ncclAllGather of every rank's band shard (each rank sends its shard once to each of the N-1 peers, one "
                     "xGMI link per peer: time >= shard bytes / 153 GB/s); layout shards: in place, nothing else "
                     "(srz_frameset_allgather_inplace; frames stay in rank-major shard order), layout rows: + one HIP "
                     "de-interleave pass into row-major frames (srz_frameset_allgather); step k's exchange runs while step k+1 renders",
             "last_full": full[(steps - 1) % 2]}
    return dt, kt, [], multi


_PMC = None


def pmc_counters(workload, frames_per_step, scope):
    """HBM bytes and VALU wave-instructions per step of this workload from profiles/pmc_counters.json — the rocprofv3 --pmc passes
    of the same bench.py command with --lanes 1 (profiles/collect.sh; the counters are per dispatch, i.e. per step of a
    one-stream run: the bytes and instructions of a step do not depend on how its launches are spread over streams).  NOT
    measured in this run: a profile of another code version describes that version — the file carries the hash of the kernel
    sources it profiled (kernel_source_hash), and counters of other sources are not reported (→ None; pmc_stale() says why)."""
    global _PMC
    if _PMC is None:
        try:
            _PMC = json.load(open(os.path.join(REPO, "profiles", "pmc_counters.json")))
        except Exception:  # noqa: BLE001
            _PMC = {}
    if pmc_stale():
        return None
    t = _PMC.get(workload)
    if not isinstance(t, dict) or t.get("frames_per_step") != frames_per_step or scope != "raster":
        return None
    return t


def pmc_stale():
    """True when profiles/pmc_counters.json was collected from other kernel sources than the ones in this tree"""
    if _PMC is None:
        pmc_counters("", 0, "")
    return bool(_PMC) and _PMC.get("_kernel_source_hash") != kernel_source_hash()


def case_record(case, steps, dt, kt, per_step, frag_total, vis_total):
    fs = case.fs
    fps = case.n_frames * steps / dt
    pipeline_s = kt["total_ms"] * 1e-3
    achieved = (case.algo_bytes / pipeline_s / 1e9 if pipeline_s > 0 else 0.0) if case.algo_bytes is not None else None
    pm = pmc_counters(case.name, case.n_frames, case.scope) if case.world == 1 else None
    # VALU issue beside the HBM fraction (a kernel can sit far below the HBM roofline because it is bound by instruction issue):
    # wave-instructions per step x 2 cycles / the SIMD-cycles of the step's device time.  A CDNA4 SIMD is 32 lanes wide: with two
    # or more resident waves it retires one plain wave64 VALU instruction per 2 cycles (measured, tools/cpp/valu_rate_probe.hip:
    # v_fma_f32 2.5 cycles at the nominal 2.4 GHz, i.e. 2 at the clock the chip sustains under that load; one wave alone 5.6;
    # v_mul_f64 and v_pk_fma_f32 4.2-4.5, v_rcp_f32 8.2) — so this is a LOWER bound of the pipe's occupancy;
    # valu_pipe_frac_est prices binary64 arithmetic at 4 and transcendentals at 8 cycles from the instruction-class counters
    # (packed f32 instructions, 4 cycles, are not counted apart: still a lower bound)
    valu = None
    if pm and pipeline_s > 0 and vis_total is not None:
        simd_cycles = N_SIMD * SCLK_HZ * pipeline_s
        valu = {"valu_wave_insts_per_step": pm["valu_wave_insts_per_step"],
                "valu_frac": pm["valu_wave_insts_per_step"] * 2.0 / simd_cycles,
                "valu_pipe_frac_est": (pm["valu_pipe_cycles_per_step"] / simd_cycles) if pm.get("valu_pipe_cycles_per_step") else None,
                "valu_per_64_visible_px": pm["valu_wave_insts_per_step"] / max(1.0, vis_total / 64.0),
                "definition": "SQ_INSTS_VALU per step x 2 cycles / (1024 SIMDs x 2.4 GHz x launch_ms)",
                "source": f"profiles/{pm['from']} (rocprofv3 --pmc pass of this workload, --lanes 1; not measured in this run)"}
    return {
        "workload": case.name, "scope": case.scope, "lanes": kt.get("lanes", 1), "width": fs.width, "height": fs.height,
        "frames_per_step": case.n_frames, "triangles_per_frame": case.tris_per_frame, "steps": steps,
        "frames_per_sec": fps, "ms_per_step": dt / steps * 1e3,
        "ms_per_step_p10_median_p90": [pct(per_step, 0.1), pct(per_step, 0.5), pct(per_step, 0.9)] if per_step else None,
        "us_per_frame_median": (pct(per_step, 0.5) * 1e3 / case.n_frames) if per_step else None,
        # (frag_total / vis_total None: the counting pass did not run, a plain run without --full)
        "mfragments_per_sec": frag_total / fs.n_frames * fps / 1e6 if frag_total is not None else None,
        "fragments_per_frame": frag_total / fs.n_frames if frag_total is not None else None,
        "visible_pixels_per_frame": vis_total / fs.n_frames if vis_total is not None else None,
        "valu": valu,
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS if achieved is not None else None,
                     "traffic": pm["hbm_bytes_per_step"] if pm else None, "traffic_stale": (pmc_stale() and case.world == 1) or None,
                     "traffic_over_algorithmic": pm["hbm_bytes_per_step"] / case.algo_bytes if pm and case.algo_bytes else None,
                     "algorithmic_bytes_per_launch": case.algo_bytes, "launch_ms": kt["total_ms"],
                     "lanes": kt.get("lanes", 1), "lane_launch_ms": kt.get("lane_launch_ms"),
                     "clear_wgs": kt.get("clear_wgs"), "clear_tuned": kt.get("clear_tuned"),
                     "one_stream": {"ms_per_step": kt.get("one_stream_ms_per_step"), "launch_ms": kt.get("split_total_ms"),
                                    "k_setup_bin_ms": kt.get("bin_ms"), "k_raster_ms": kt.get("raster_ms"), "k_shade_ms": kt.get("shade_ms")}},
    }


def per_config_summary(rec):
    """the compact per-workload record of roofline.per_config"""
    if "error" in rec:
        return {"error": rec["error"]}
    if rec.get("scope") == "readme_loop":
        return {"scope": "readme_loop", "draw_complete_ms_p10_median_p90": [rec["draw_complete_ms"][k] for k in ("p10", "median", "p90")],
                "draw_submit_ms_median": rec["draw_submit_ms"]["median"], "display_ms_median": rec["display_ms"]["median"],
                "frames": rec["frames"], "reference_published_draw_ms_median": 17.06}
    r, v = rec["roofline"], rec.get("valu") or {}
    return {"scope": rec["scope"], "frames_per_step": rec["frames_per_step"], "lanes": rec["lanes"], "frames_per_sec": rec["frames_per_sec"],
            "ms_per_step": rec["ms_per_step"], "frac": r["frac"], "traffic_over_algorithmic": r["traffic_over_algorithmic"], "clear_wgs": r.get("clear_wgs"),
            "valu_pipe_frac_est": v.get("valu_pipe_frac_est"),
            "one_stream_us": {"setup_bin": r["one_stream"]["k_setup_bin_ms"] * 1e3, "raster": r["one_stream"]["k_raster_ms"] * 1e3,
                              "shade": r["one_stream"]["k_shade_ms"] * 1e3}}


def emulate_shards(srz, torch, device, fence, args):
    """The render-side term of the N-GPU job, measured on ONE GPU: for N in {2, 4, 8} this GPU plays every rank r
    of N in turn (srz.Context(device, r, N): its 32-row bands of all F*N frames, one frameset on one stream as an N > 1 rank
    renders them) and reports the per-rank render time, its imbalance, and the step an N-GPU job cannot beat:
    max(slowest rank's render, shard bytes / 153 GB/s per xGMI link) for both exchanges.  F (frames per GPU) is smaller than
    the headline's so that the fourteen + sixteen framesets stay cheap: every term scales with F, their ratios do not.
    No multi-GPU run — nothing here claims one."""
    from srz import abi, scenes
    plan = [(args.workload, 32, (2, 4, 8)), ("spot_x16_texture_2048", 8, (8,)), ("spot_x8_overdraw_4096", 4, (8,))]
    out = {}
    stream = torch.cuda.Stream()
    for (w, f_gpu, worlds) in plan:
        wl = scenes.WORKLOADS[w]()
        rec = {"frames_per_gpu": f_gpu}
        for n in worlds:
            n_frames = f_gpu * n
            uniq = [wl.frame(i) for i in range(min(n_frames, 36))]
            frames = [uniq[i % len(uniq)] for i in range(n_frames)]
            ms = []
            shard_bytes = 0
            for r in range(n):
                c = srz.Context(device, r, n)
                wl.upload_textures(c)
                fs = c.frameset(frames)
                buf = torch.empty(fs.out_shape, dtype=torch.float32, device="cuda")
                shard_bytes = fs.out_bytes
                with torch.cuda.stream(stream):
                    for _ in range(4):
                        fs.render(buf.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream.cuda_stream)
                    fence()
                    c.set_kernel_timing(1)
                    c.kernel_time_ms(reset=True)
                    for _ in range(6):
                        fs.render(buf.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream.cuda_stream)
                    fence()
                    kt = c.kernel_time_ms(reset=True)
                ms.append(kt["total_ms"])
                fs.close()
                c.close()
                del buf
            torch.cuda.empty_cache()
            x_planes = shard_bytes / (XGMI_LINK_GBS * 1e9) * 1e3
            x_bgr8 = x_planes * 3.0 / 16.0
            rec[f"N{n}"] = {"shard_render_ms": ms, "max_over_mean": max(ms) / (sum(ms) / len(ms)),
                            "predicted_step_ms": {"planes": max(max(ms), x_planes), "bgr8": max(max(ms), x_bgr8)},
                            "predicted_fps": {"planes": n_frames / max(max(ms), x_planes) * 1e3, "bgr8": n_frames / max(max(ms), x_bgr8) * 1e3}}
        out[w] = rec
    return out


def sig(x, n=4):
    """floats to n significant digits (the line is for reading and for the driver's parser; the full precision is in the details file)"""
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    if x != x or x in (float("inf"), float("-inf")):
        return None
    return float(f"{x:.{n}g}")


def compact(o, n=4):
    if isinstance(o, dict):
        return {k: compact(v, n) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [compact(v, n) for v in o]
    return sig(o, n)


LINE_LIMIT = 6000  # bytes: the driver keeps 8 KB of stdout and parses the LAST line of it (round 4's 21 KB line came back parsed: null)
DETAILS = os.path.join(REPO, "bench_details.json")
SHORT = {"spot_bunny_phong_1080p": "c3", "spot_x16_texture_2048": "c4", "spot_x8_overdraw_4096": "c5", "readme_spot_crate_1024": "readme",
         "spot_texture_1024_p7.5": "c2_p7.5", "spot_texture_1024": "c2"}


def emit(res, extras):
    """The full record (every note, every configs[] entry at full precision) goes to bench_details.json next to this script
    (and, as one line, to stderr); stdout gets ONE compact JSON line of < LINE_LIMIT bytes as its LAST line: the contract's
    keys, `roofline` (flat per-config scalars the driver's parser keeps + the nested per_config), `valu`, `cpu_baseline`."""
    full = dict(res, configs=extras)
    try:
        with open(DETAILS, "w") as f:
            json.dump(full, f, indent=1)
    except OSError:
        pass
    sys.stderr.write("bench.py details: " + json.dumps(full) + "\n")
    sys.stderr.flush()
    roof = res["roofline"]
    one = roof.get("one_stream") or {}
    r = {k: roof.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_stale", "traffic_over_algorithmic",
                                  "algorithmic_bytes_per_launch", "launch_ms", "lanes", "clear_wgs", "launches_timed", "kernel_source_hash")}
    r["kernel"] = "k_setup+k_bin+k_raster+k_shade in line, k_clear beside them (second stream); HIP events on the launch streams"
    # both peaks, as BASELINE.md §4 asks: 8.0 TB/s spec (`peak`, `frac`) and the 6.29 TB/s measured float4 copy of the guide
    r["peak_measured"] = HBM_MEASURED_COPY_GBS
    r["frac_measured"] = roof["achieved"] / HBM_MEASURED_COPY_GBS if roof.get("achieved") is not None else None
    r["frac_unprimed"] = (roof["algorithmic_bytes_per_launch"] / (res["ms_per_step_unprimed"] * 1e-3) / 1e9 / HBM_PEAK_GBS) if res.get("ms_per_step_unprimed") else None
    r["one_stream_us"] = [x * 1e3 if x is not None else None for x in (one.get("k_setup_bin_ms"), one.get("k_raster_ms"), one.get("k_shade_ms"))]
    pc = {}
    for name, v in (roof.get("per_config") or {}).items():
        base, _, tag = name.partition(":")
        key = SHORT.get(base, base) + (":" + tag if tag else "")
        if "error" in v:
            pc[key] = {"error": v["error"][:80]}
        elif v.get("scope") == "readme_loop":
            pc[key] = {"draw_ms_p10_med_p90": v["draw_complete_ms_p10_median_p90"], "display_ms": v["display_ms_median"], "frames": v["frames"],
                       "ref_published_draw_ms": v["reference_published_draw_ms_median"]}
        else:
            pc[key] = {"F": v["frames_per_step"], "fps": v["frames_per_sec"], "ms": v["ms_per_step"], "frac": v["frac"],
                       "t_over_a": v["traffic_over_algorithmic"], "us": [v["one_stream_us"][k] for k in ("setup_bin", "raster", "shade")],
                       "wgs": v.get("clear_wgs")}
            if not tag:  # flat scalars: the driver's parser keeps a nested object's scalars only
                r["frac_" + key], r["fps_" + key] = v["frac"], v["frames_per_sec"]
                r["frac_measured_" + key] = v["frac"] * HBM_PEAK_GBS / HBM_MEASURED_COPY_GBS
    r["per_config"] = pc
    r["per_config_keys"] = "F frames/step, fps, ms/step (2 lanes), frac of 8 TB/s (frac_measured*: of the 6.29 TB/s measured copy), traffic/algorithmic, us = one-stream [setup+bin, raster, shade], wgs = measured grid of each lane's clear"
    mg = roof.get("multi_gpu_emulated")
    if mg is not None:
        r["multi_gpu_emulated"] = mg if "error" in mg else {
            SHORT.get(w, w): {k: (v if not isinstance(v, dict) else
                                  {"ms": v["shard_render_ms"], "max_over_mean": v["max_over_mean"], "pred_ms": v["predicted_step_ms"], "pred_fps": v["predicted_fps"]})
                              for k, v in rec.items()} for w, rec in mg.items()}
    line = {k: res.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                    "vs_baseline", "dtype", "data")}
    line["config"] = res["config"]
    line.update({k: res.get(k) for k in ("priming_steps", "value_unprimed", "ms_per_step_unprimed", "mfragments_per_sec", "fragments_per_frame",
                                         "visible_pixels_per_frame", "ms_per_step_p10_median_p90")})
    line["roofline"] = r
    v = res.get("valu")
    line["valu"] = {k: v.get(k) for k in ("valu_frac", "valu_pipe_frac_est", "valu_per_64_visible_px")} if v else None
    cb = res.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {k: cb.get(k) for k in ("value", "unit", "cores", "kind", "shape", "cpu_model", "host_cpus")}
        line["cpu_baseline"]["sample"] = (cb.get("sample_short") or cb.get("sample", ""))[:200]
    if res.get("multi_gpu"):
        m = res["multi_gpu"]
        line["multi_gpu"] = {k: m.get(k) for k in ("headline_exchange", "layout", "behind_c_abi", "overlapped", "second_pass", "step_ms", "render_ms_per_step",
                                                   "exchange_alone_ms_per_step", "hidden_ms_per_step", "bytes_sent_per_rank_per_step",
                                                   "predicted_exchange_ms_at_xgmi_peak", "bgr8", "predicted", "fallback") if m.get(k) is not None}
    line["details"] = "bench_details.json (+ stderr): every note and configs[] at full precision"
    out = json.dumps(compact(line, 5), separators=(",", ":"))
    if len(out) >= LINE_LIMIT:  # never let extras cost the parse: drop the nested tables first, the flat scalars stay
        for k in ("multi_gpu_emulated", "per_config"):
            line["roofline"].pop(k, None)
            out = json.dumps(compact(line, 5), separators=(",", ":"))
            if len(out) < LINE_LIMIT:
                break
        if len(out) >= LINE_LIMIT:  # ... then the flat scalars of everything but the BASELINE configs
            keep = {"frac_unprimed", "frac_measured"} | {p + c for p in ("frac_", "fps_", "frac_measured_") for c in ("c3", "c4", "c5")}
            line["roofline"] = {k: v for k, v in line["roofline"].items() if not k.startswith(("frac_", "fps_")) or k in keep}
            out = json.dumps(compact(line, 5), separators=(",", ":"))
    sys.stdout.flush()
    print(out, flush=True)


def multi_gpu_budget(args, world, wl_name):
    """HBM the N > 1 loop allocates per rank, checked BEFORE anything is allocated (the in-place exchange keeps 2 gathered
    buffers of world x shard each; the headline's 8-bit ones and the float planes' are not alive together)"""
    from srz import parallel, scenes
    wl = scenes.WORKLOADS[wl_name]()
    lay = parallel.shard_layout(wl.height, 0, world)
    n_frames = args.frames * world
    shard_planes = n_frames * 16 * lay["local_rows"] * wl.width
    shard_bgr8 = n_frames * 3 * lay["local_rows"] * wl.width
    planes_case = 2 * shard_planes                                   # Case.out (n_out = 2): the rank's own float planes
    peak = planes_case + max(2 * world * shard_bgr8, 2 * world * shard_planes)
    inputs = n_frames * (wl.frame(0).n_tris * (96 + 36 + 8 + 2 + 40) + 8 * lay["local_rows"] * wl.width)  # records, dense positions, boxes, entries, lists
    return {"frames_per_step": n_frames, "shard_bytes_planes": shard_planes, "shard_bytes_bgr8": shard_bgr8,
            "gathered_buffers_bytes_planes": 2 * world * shard_planes, "gathered_buffers_bytes_bgr8": 2 * world * shard_bgr8,
            "peak_bytes_estimate": peak + inputs, "hbm_bytes": HBM_BYTES}


def predicted_exchange(shard_bytes, n_frames_total):
    """every rank sends its shard once to each of the N - 1 peers over that peer's own xGMI link, so bytes per link
    per step = shard bytes whatever N, and a step cannot be faster than that (render hidden under the exchange)"""
    ms = shard_bytes / (XGMI_LINK_GBS * 1e9) * 1e3
    return {"exchange_ms_at_xgmi_peak": ms, "frames_per_sec_if_exchange_bound": n_frames_total / (ms * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=15,
                    help="untimed steps first; the first ~13 steps after idle run up to 10 %% slower (clock ramp, first-touch "
                         "of the record pool): tools/step_series_probe.py prints the series")
    ap.add_argument("--frames", type=int, default=256, help="frames per step per GPU")
    ap.add_argument("--workload", default="spot_texture_1024")
    ap.add_argument("--scope", choices=["raster", "draw"], default="raster",
                    help="raster: post-MVP triangle streams resident in HBM (BASELINE's hot path); "
                         "draw: meshes + per-frame matrices resident, the vertex stage (k_vertex) is timed too")
    ap.add_argument("--exchange", choices=["bgr8", "planes", "both"], default="both",
                    help="N>1 only. planes: all-gather the 4 float planes (16 B/px: z + m_channels) — the headline; bgr8: resolve to "
                         "8-bit on the device and all-gather display()'s image (3 B/px); both: the headline exchanges the planes and, "
                         "with --full, a second, shorter pass times bgr8 (multi_gpu.bgr8)")
    ap.add_argument("--exchange-layout", choices=["shards", "rows"], default="shards",
                    help="N>1 only. shards: render into the rank's slot of the gathered buffer, ONE in-place all-gather, no second "
                         "pass (frames stay in rank-major shard order); rows: all-gather + a HIP de-interleave pass (row-major frames)")
    ap.add_argument("--lanes", type=int, default=0,
                    help="N=1: the batch is rendered as this many runs of whole frames on streams of their own "
                         "(srz.parallel.LaneRenderer: consecutive steps overlap at their edges); 1 = one frameset on one "
                         "stream; 0 = two lanes for steps of >= 64 frames, else one")
    ap.add_argument("--no-overlap", action="store_true", help="N>1 only: render and exchange back to back on one stream")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beside the headline too: the unprimed region, the counting pass (Mfragments/s), the "
                         "one-stream per-kernel split; at N=1 the other BASELINE configs / scope draw / the README loop / the "
                         "tolerance mode / the emulated N-GPU shards and the CPU baseline; at N>1 the exchange alone and bgr8. "
                         "Without it a run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write a seeded sample of what the last one computed to DIR/*.npy (dump_outputs)")
    ap.add_argument("--no-extras", action="store_true", help="with --full, N=1: skip the other BASELINE configs / scope draw / the README loop")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-budget-s", type=float, default=12.0)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # ---- no launcher around us: start the ranks ourselves, BEFORE torch / HIP are touched in this process ----------------------
    # (SRZ_BENCH_FORCE_LAUNCHER=1: take this path at N = 1 too — one child that runs the N > 1 code at world 1: tests)
    force = os.environ.get("SRZ_BENCH_FORCE_LAUNCHER") == "1"
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or force):
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        args.gpus = world  # (the launcher decides)
    multi_path = world > 1 or (force and os.environ.get("SRZ_BENCH_LAUNCHED") == "1")

    # the reference's published protocol through the C++ API: a child process, before this one initialises the GPU
    loop_rec = readme_loop() if (args.full and world == 1 and not multi_path and not args.no_extras) else None

    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        sys.exit("bench.py needs an MI355X (no CPU fallback exists for the product path)")
    import srz
    from srz import abi, parallel  # noqa: F401

    torch.cuda.set_device(local_rank)
    if multi_path:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        budget = multi_gpu_budget(args, world, args.workload)
        free_b, total_b = torch.cuda.mem_get_info()
        if budget["peak_bytes_estimate"] > 0.85 * total_b:
            sys.exit(f"bench.py: --frames {args.frames} x {world} ranks needs ~{budget['peak_bytes_estimate'] / 1e9:.0f} GB per GPU "
                     f"(2 x world x shard gathered buffers), the device has {total_b / 1e9:.0f} GB: lower --frames")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    def fence():
        torch.cuda.synchronize()
        if multi_path:
            dist.barrier()
            torch.cuda.synchronize()

    ctx = srz.Context(local_rank, rank, world)
    comm, comm_note = (None, None) if not multi_path else make_comm(ctx, dist, torch, rank, world)

    case = Case(ctx, torch, args.workload, args.frames, args.scope, world, n_out=2 if multi_path else 1, stats=args.full)
    fs, stats = case.fs, case.stats
    if stats is None:
        frag_total, vis_total = None, None
    elif multi_path:
        st = torch.tensor([stats["fragments"], stats["visible"]], dtype=torch.int64, device="cuda")
        dist.all_reduce(st)
        frag_total, vis_total = int(st[0]), int(st[1])
    else:
        frag_total, vis_total = stats["fragments"], stats["visible"]

    multi = None
    if not multi_path:
        dt, kt, per_step = time_single_gpu(case, args.steps, args.warmup, fence, args.lanes, unprimed=args.full, split=False)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, case.out[0])
        if args.full:
            one_stream_split(case, args.steps, fence, kt)
            ctx.set_kernel_timing(0)
    else:
        head_x = "bgr8" if args.exchange == "bgr8" else "planes"
        dt, kt, per_step, multi = time_multi_gpu(case, comm, dist, args.steps, args.warmup, fence, head_x,
                                                 args.no_overlap, args.exchange_layout, rank, exchange_alone=args.full)
        last_full = multi.pop("last_full")
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, last_full)
        del last_full
        multi["headline_exchange"] = head_x
        multi["why"] = ("planes = z + the three float m_channels, what draw() leaves and what north_star's parity is stated on (z bit-exact): "
                        "the headline at every N; bgr8 = display()'s m_frameBuffer after convertTo(CV_8UC3) (src/Render.cpp:61-62 of the "
                        "reference), 3 B/px, reported beside it and never as `value` unless --exchange bgr8 is asked for")
        multi["budget"] = budget
        multi["predicted"] = {"bgr8": predicted_exchange(budget["shard_bytes_bgr8"], case.n_frames),
                              "planes": predicted_exchange(budget["shard_bytes_planes"], case.n_frames),
                              "source": "DESIGN.md §6: shard bytes / 153 GB/s per xGMI link; render (≈ the N = 1 step) hidden under it"}
        if args.full and args.exchange == "both":  # display()'s 8-bit image beside the headline
            torch.cuda.empty_cache()
            k2 = max(3, args.steps // 2)
            dt2, kt2, _, m2 = time_multi_gpu(case, comm, dist, k2, min(args.warmup, 2), fence, "bgr8", args.no_overlap,
                                             args.exchange_layout, rank)
            m2.pop("last_full")
            multi["bgr8"] = {"frames_per_sec": case.n_frames * k2 / dt2, "steps": k2, "ms_per_step": dt2 / k2 * 1e3,
                             "render_ms_per_step": m2["render_ms_per_step"], "exchange_alone_ms_per_step": m2["exchange_alone_ms_per_step"],
                             "hidden_ms_per_step": m2["hidden_ms_per_step"], "bytes_sent_per_rank_per_step": m2["bytes_sent_per_rank_per_step"]}
        if comm_note:
            multi["fallback"] = comm_note

    res = None
    if rank == 0:
        rec = case_record(case, args.steps, dt, kt, per_step, frag_total, vis_total)
        pm = pmc_counters(args.workload, case.n_frames, args.scope) if not multi_path else None
        traffic, traffic_src = (pm["hbm_bytes_per_step"], f"profiles/{pm['from']}") if pm else (None, None)
        roof = rec["roofline"]
        roof.update({"traffic": traffic,
                     "traffic_source": (f"{traffic_src}: FETCH_SIZE x2 + WRITE_SIZE of rocprofv3 --pmc passes of this command with --lanes 1 "
                                        "(same bytes per step, kernels not overlapped), per step (not measured in this run; "
                                        "kernel sources' hash checked)") if traffic else None,
                     "kernel_source_hash": kernel_source_hash(),
                     "frac_of_measured_copy_6290": roof["achieved"] / HBM_MEASURED_COPY_GBS if roof["achieved"] is not None else None,
                     "kernel": "hot path = k_setup + k_bin + k_raster (+ k_raster_slow) + k_shade in line, k_clear beside k_raster/k_shade "
                               "on a second stream (one launch each per lane per step)",
                     "launches_timed": kt["launches"],
                     "note": "rank 0's shard. launch_ms = device time of the timed region (HIP events: first launch set's start to "
                             "the last one's end) / steps — the lanes' launch sets overlap, lane_launch_ms is one lane's own "
                             "start-to-end; one_stream = the batch in one piece on one stream, measured after the timed region "
                             "(where the per-kernel split comes from). algorithmic bytes = "
                             "16*W*rows + 96*N_tri + 24*N_lights + min(3*texW*texH, 3*textured_px) per frame"})
        udt = kt.get("unprimed_dt")
        res = {
            "metric": "frames_per_sec", "value": rec["frames_per_sec"], "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "priming_steps": kt.get("priming_steps", max(0, PRIME_TO - args.warmup)),
            "ms_per_step": rec["ms_per_step"],
            "value_unprimed": (case.n_frames * args.steps / udt) if udt else None,
            "ms_per_step_unprimed": (udt / args.steps * 1e3) if udt else None,
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": args.workload, "width": fs.width, "height": fs.height,
                       "frames_per_step": case.n_frames, "frames_per_step_per_gpu": args.frames,
                       "triangles_per_frame": case.tris_per_frame, "lights": len(case.frames[0].lights), "scope": args.scope,
                       "sharding": "whole frames on 1 GPU" if not multi_path else
                       f"32-row bands round-robin over {world} GPUs + RCCL all-gather of {multi['headline_exchange']}, layout {args.exchange_layout} (timed)"},
            "mfragments_per_sec": rec["mfragments_per_sec"], "fragments_per_frame": rec["fragments_per_frame"],
            "visible_pixels_per_frame": rec["visible_pixels_per_frame"],
            "ms_per_step_p10_median_p90": rec["ms_per_step_p10_median_p90"], "us_per_frame_median": rec["us_per_frame_median"],
            "roofline": roof, "valu": rec["valu"],
            "reference_published": {"fps": 58.6, "note": "README.md:619-629, i7-12800HX/MSVC, spot+crate 5-mesh scene, "
                                    "draw() incl. vertex stage — different workload/hardware, not reproducible here"},
        }
        if multi:
            res["multi_gpu"] = multi
    case.close()

    # ---- N = 1: the other GPU configs of BASELINE.json + configs[1] at scope draw, each outside the headline's timed region
    extras = []
    if args.full and not multi_path and not args.no_extras:
        todo = [(w, f, s, "raster", args.lanes, 0) for (w, f, s) in EXTRA_CASES if w != args.workload]
        todo.append((args.workload, args.frames, max(5, args.steps // 2), "draw" if args.scope == "raster" else "raster", args.lanes, 0))
        # the headline workload once more the other way (one frameset on one stream / two lanes on two streams)
        todo.append((args.workload, args.frames, args.steps, args.scope, 2 if args.lanes == 1 else 1, 0))
        # the tolerance mode (SRZ_OPT_APPROX_SHADE: the reference's own arithmetic class) on the configs it is for
        todo += [(w, f, s, "raster", args.lanes, 1) for (w, f, s) in APPROX_CASES]
        per_config = {}
        for (w, f, s, scope, n_lanes, approx) in todo:
            try:
                if approx:
                    ctx.set_option(abi.OPT_APPROX_SHADE, 1)
                c = Case(ctx, torch, w, f, scope, 1)
                d, k, ps = time_single_gpu(c, s, 15 if w == args.workload else 8, fence, n_lanes)
                extras.append(case_record(c, s, d, k, ps, c.stats["fragments"], c.stats["visible"]))
                extras[-1]["approx_shade"] = bool(approx)
                if approx:
                    extras[-1]["valu"] = None  # (the instruction counters in profiles/ are the exact builds')
                c.close()
            except Exception as e:  # noqa: BLE001  (an extra must never cost the headline line)
                extras.append({"workload": w, "scope": scope, "error": str(e)[:200]})
            finally:
                if approx:
                    ctx.set_option(abi.OPT_APPROX_SHADE, 0)
            if approx:
                per_config[w + ":approx"] = per_config_summary(extras[-1])
            elif w in PER_CONFIG and scope == "raster":
                per_config[w] = per_config_summary(extras[-1])
            elif w == args.workload and scope == "draw":
                per_config[w + ":draw"] = per_config_summary(extras[-1])
            elif w == args.workload and scope == args.scope:
                per_config[w + f":lanes{n_lanes}"] = per_config_summary(extras[-1])
        if loop_rec is not None:
            extras.append(loop_rec)
            per_config["readme_spot_crate_1024:readme_loop"] = per_config_summary(loop_rec)
        res["roofline"]["per_config"] = per_config
        # the render-side term of the N-GPU job, measured on this one GPU
        try:
            res["roofline"]["multi_gpu_emulated"] = emulate_shards(srz, torch, local_rank, fence, args)
        except Exception as e:  # noqa: BLE001
            res["roofline"]["multi_gpu_emulated"] = {"error": str(e)[:200]}
    if args.full and not multi_path and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(args.workload, args.cpu_budget_s)
    if rank == 0:
        emit(res, extras)
    if comm is not None:
        comm.close()
    if multi_path:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
