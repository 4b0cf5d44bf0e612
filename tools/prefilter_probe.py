"""The cube prefilter (srz_cube_prefilter / srz_cube_prefilter_grad) timed on its own, beside a dense-matrix baseline in torch.

    python tools/prefilter_probe.py [rounds] [--out FILE]

Legs, at C = 3 and one frame: the irradiance cube COSINE 64 -> 8, and the specular levels GGX 128 -> 128 and 64 -> 64 at roughness
0.25 and 1, each forward and backward, cmin 0.  Beside them, for context, what a caller without the pass would write: the dense
weight matrix [6 n_dst^2, 6 n_src^2] built ONCE, outside the timing, and one matmul per call (forward W @ src, backward W^T @ g) —
for the legs whose matrix fits (128 -> 128 is 9.7 G entries: left out).  After 5 warm-up rounds the legs alternate in one process,
each timed with device events on its own; the median of the rounds (default 20) is reported with p10 and p90, the pairs per second
(6 n_dst^2 * 6 n_src^2 per call: skipped pairs are visited too), and the share of the vector ALU's plain issue rate (1024 SIMDs x
16 lanes x 2.4 GHz = 39.3 T lane-operations / s; the 157.3 TFLOPS figure counts a packed fma as four) that the VALU operations
counted per pair in k_prefilter's source imply: 9 + 2 C for COSINE, 23 + 2 C for GGX (the IEEE division taken as 11).  Prints one
JSON line and writes it to --out.  Nothing is asserted: one box, no timing gate."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "software-rasterizer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import srz  # noqa: E402
from srz import abi  # noqa: E402
from srz.visibility import cube_dirs  # noqa: E402

C, WARMUP = 3, 5
ISSUE_RATE = 1024 * 16 * 2.4e9
LEGS = [("cosine_64to8", abi.PREFILTER_COSINE, 64, 8, 1.0), ("ggx_128to128_r0.25", abi.PREFILTER_GGX, 128, 128, 0.25),
        ("ggx_128to128_r1", abi.PREFILTER_GGX, 128, 128, 1.0), ("ggx_64to64_r0.25", abi.PREFILTER_GGX, 64, 64, 0.25),
        ("ggx_64to64_r1", abi.PREFILTER_GGX, 64, 64, 1.0)]
DENSE_MAX = 1 << 30  # entries of a weight matrix the baseline builds


def pct(xs, p):
    return float(np.percentile(np.asarray(xs, np.float64), p))


def texel_geometry(n):
    """(d [6 n n, 3], jac [6 n n]) in float32 torch, the midpoint geometry of include/srz.h (not bit-exact: context only)"""
    c = (2.0 * torch.arange(n, dtype=torch.float32, device="cuda") + 1.0) / n - 1.0
    t, s = torch.meshgrid(c, c, indexing="ij")
    jac = (1.0 + s * s + t * t) ** -1.5
    return cube_dirs(n, "cuda").reshape(-1, 3).contiguous(), jac.reshape(-1).repeat(6).contiguous()


def dense_matrix(kind, n_src, n_dst, roughness):
    do, _ = texel_geometry(n_dst)
    di, jac = texel_geometry(n_src)
    c = (do @ di.T).clamp_(max=1.0)
    w = torch.where(c > 0, c * jac[None, :], torch.zeros((), device="cuda"))
    if kind == abi.PREFILTER_GGX:
        a2 = max(roughness, 0.0625) ** 4
        w /= ((0.5 * c + 0.5) * (a2 - 1.0) + 1.0) ** 2
    del c
    return w / w.sum(1, keepdim=True)


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 20
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    ctx = srz.Context(0)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    calls, pairs, ops, keep = {}, {}, {}, []
    for name, kind, n_src, n_dst, r in LEGS:
        src = torch.rand((6, n_src, n_src, C), device="cuda")
        dst, den = torch.empty((6, n_dst, n_dst, C), device="cuda"), torch.empty((6, n_dst, n_dst), device="cuda")
        g, gsrc = torch.randn((6, n_dst, n_dst, C), device="cuda"), torch.empty_like(src)
        nbytes = ctx.cube_prefilter_work_bytes(n_src, n_dst, C, 1)
        work = torch.empty((nbytes // 4,), device="cuda")
        keep += [src, dst, den, g, gsrc, work]
        a = (src.data_ptr(), dst.data_ptr(), den.data_ptr(), g.data_ptr(), gsrc.data_ptr(), work.data_ptr())
        calls[name + "_forward"] = lambda a=a, k=(n_src, n_dst, kind, r, nbytes): ctx.cube_prefilter(a[0], k[0], a[1], k[1], C, 1, k[2], k[3], 0.0, a[2],
                                                                                                     a[5], k[4], sp)
        calls[name + "_backward"] = lambda a=a, k=(n_src, n_dst, kind, r, nbytes): ctx.cube_prefilter_grad(a[3], a[2], k[0], k[1], C, 1, k[2], k[3], 0.0,
                                                                                                           a[4], a[5], k[4], sp)
        n_pairs = 36 * n_src ** 2 * n_dst ** 2
        for leg in ("_forward", "_backward"):
            pairs[name + leg] = n_pairs
            ops[name + leg] = (9 if kind == abi.PREFILTER_COSINE else 23) + 2 * C
        if n_pairs <= DENSE_MAX:
            w = dense_matrix(kind, n_src, n_dst, r)
            keep.append(w)
            calls[name + "_torch_forward"] = lambda w=w, src=src: torch.matmul(w, src.view(-1, C))
            calls[name + "_torch_backward"] = lambda w=w, g=g: torch.matmul(w.T, g.view(-1, C))
            pairs[name + "_torch_forward"] = pairs[name + "_torch_backward"] = n_pairs
    for _ in range(WARMUP):  # clock ramp, first launches (the forward writes the den the backward reads)
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
    row = {"rounds": rounds, "channels": C}
    for k, evs in times.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        med = float(np.median(ms))
        row[k] = {"ms_median": med, "ms_p10": pct(ms, 10), "ms_p90": pct(ms, 90), "pairs": pairs[k], "gpairs_per_s": pairs[k] / med / 1e6}
        if k in ops:
            row[k]["valu_ops_per_pair"] = ops[k]
            row[k]["valu_issue_share"] = pairs[k] * ops[k] / (med * 1e-3) / ISSUE_RATE
    print(json.dumps(row), flush=True)
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
