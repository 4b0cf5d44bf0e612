"""The motion pass's test reference (tests/motion_ref.c holds the arithmetic): the positions of the TARGET frame, per pixel (owner id
word, alpha, beta) of the frame, and the target frame's id and z planes → the five planes of every group, as uint32 words.  Built and
loaded like tests/gbufref.py's library; nothing of the product is involved."""
import ctypes as C
import os
import subprocess

import numpy as np

from srz import abi
from support import build_c, ref_lib, word_planes

GROUPS = ((abi.MV_FLOW, (0, 1)), (abi.MV_DEPTH, (2,)), (abi.MV_TARGET, (3, 4)))
INF_WORD = 0x7f800000
vp = C.c_void_p
SIGNATURES = {"mr_motion": (None, [vp, C.c_uint32, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp])}


def lib(tmpdir):
    return ref_lib("motion_ref", tmpdir, SIGNATURES)


def planes_of(what):
    """indices into the five planes of the groups in `what`, in buffer order"""
    return [i for bit, idx in GROUPS if what & bit for i in idx]


def _inputs(pos, vis_words, target_words, prefill):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    (_, ids, al, be), (rows, W) = word_planes(vis_words)
    (tz, tid, _, _), target_shape = word_planes(target_words)
    assert target_shape == (rows, W)
    out = np.zeros((5, rows, W), np.uint32) if prefill is None else np.array(prefill, np.uint32, copy=True, order="C")
    assert out.shape == (5, rows, W)
    return pos, [ids, al, be, tid, tz], out


def expected(tmpdir, pos, vis_words, target_words, fused=True, prefill=None):
    """pos: the target frame's positions [n, 9] (triangle t there stands for triangle t of the frame); vis_words: [4, H, W] uint32 of
    the frame's visibility buffer (planes z, id, alpha, beta); target_words: the target frame's → [5, H, W] uint32: dx dy | z' |
    tid tz.  prefill: [5, H, W] uint32 the planes start from (not fused: nobody's words stay)."""
    pos, planes, out = _inputs(pos, vis_words, target_words, prefill)
    rows, W = out.shape[1:]
    keep = pos if len(pos) else np.zeros((1, 9), np.float32)
    lib(tmpdir).mr_motion(keep.ctypes.data, len(pos), W, rows, *(p.ctypes.data for p in planes), int(fused), out.ctypes.data)
    return out


def nobody(shape, fused=True, fill=0):
    """the five planes of a frame without a target frame: zeros when fused, else the prefill"""
    return np.full((5,) + tuple(shape), 0 if fused else fill, np.uint32)


def expected_sanitized(tmpdir, pos, vis_words, target_words, fused=True, prefill=None):
    """expected() through the same source built as a program with AddressSanitizer and UBSan (float-cast-overflow included: a NaN or a
    huge coordinate converted to an integer is a report) on heap blocks of exactly the arrays' sizes; any report fails the run"""
    exe = os.path.join(str(tmpdir), "motion_ref_asan")
    if not os.path.exists(exe):
        build_c("motion_ref", exe, "-O1", "-g", "-DMOTION_REF_MAIN", "-fsanitize=address,undefined,float-cast-overflow",
                "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
    pos, planes, out = _inputs(pos, vis_words, target_words, prefill)
    rows, W = out.shape[1:]
    src, dst = os.path.join(str(tmpdir), "motion_in.bin"), os.path.join(str(tmpdir), "motion_out.bin")
    with open(src, "wb") as f:
        f.write(np.uint32([len(pos), W, rows, int(fused)]).tobytes() + pos.tobytes())
        for p in planes:
            f.write(p.tobytes())
        f.write(out.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    return np.fromfile(dst, np.uint32).reshape(5, rows, W)


# ---- the frames the CPU test (tests/test_motion_ref.py) and the GPU test (tests/test_gpu_motion.py) share ------------------------------
TRANSLATION = (5, -3, 1.0)  # (k, m, dz)


def translation_frames(seed=0, n=70, w=96, h=80):
    """(frame, the frame moved by TRANSLATION).  Every coordinate is a multiple of 1/8 and at least 8 pixels from every edge in both
    frames, so that A - P is exact and the same in both, every product of two such differences is exact too (multiples of 1/64 below
    2^14), and no bounding box is clamped: alpha, beta, the coverage tests and the class split of a pixel (x, y) of the frame are those
    of (x + k, y + m) of the moved one, bit for bit.  Every triangle is flat in depth at a level of its own (1 + index, exact with dz),
    so that no depth comparison between two triangles is near a tie in either frame."""
    from support import frame
    k, m, dz = TRANSLATION
    rng = np.random.default_rng([seed, 4711])
    t = np.zeros(n, abi.TRI_DTYPE)
    c = rng.uniform([20, 25], [w - 26, h - 22], (n, 1, 2))
    xy = np.round((c + rng.uniform(-1, 1, (n, 3, 2)) * rng.uniform(3, 14, (n, 1, 1))) * 8) / 8
    lo, hi = np.array([8.0 - min(k, 0), 8.0 - min(m, 0)]), np.array([w - 9.0 - max(k, 0), h - 9.0 - max(m, 0)])
    xy = np.clip(xy, lo, hi)
    ab, ac = xy[:, 1] - xy[:, 0], xy[:, 2] - xy[:, 0]
    swap = (ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]) > 0  # kept: cross(B - A, C - A).z < 0 for the eye at (0, 0, 1)
    xy[swap] = xy[swap][:, [0, 2, 1]]
    t["pos"][:, :, :2] = xy
    t["pos"][:, :, 2] = (1.0 + np.arange(n))[:, None]
    t["nrm"] = [0, 0, -1]
    moved = t.copy()
    moved["pos"] += np.float32([k, m, dz])
    for a in (t, moved):
        p = a["pos"]
        assert (p[..., 0] >= 8).all() and (p[..., 0] <= w - 9).all() and (p[..., 1] >= 8).all() and (p[..., 1] <= h - 9).all()
        assert (p[..., :2] * 8 == np.round(p[..., :2] * 8)).all()
    return frame(t, w, h), frame(moved, w, h)


def hostile_target_positions(pos, w, h):
    """a copy of positions [n, 9] with hostile x / y (and some z), dealt by triangle index so that every value is there: NaN, +-inf,
    +-1e30 in one, two or three vertices, and, in all three vertices at once (so that the interpolated coordinate is the value within
    an ulp or two), values at and one ulp to either side of the borders of the image's nearest-sample range (-0.5, W - 0.5, H - 0.5)
    and of its first and last sample.  Every fifth triangle stays as it is."""
    out = np.array(pos, np.float32, copy=True).reshape(-1, 3, 3)
    wild = np.float32([np.nan, np.inf, -np.inf, 1e30, -1e30])

    def around(values):
        vs = []
        for v in np.float32(values):
            vs += [v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))]
        return np.float32(vs)
    edges = (around([-0.5, w - 0.5, 0.0, w - 1.0]), around([-0.5, h - 0.5, 0.0, h - 1.0]))
    for i in range(len(out)):
        kind, j = i % 5, i // 5
        if kind == 0:
            continue
        if kind in (1, 2):  # a wild value in 1..3 vertices of x (kind 1) or y (kind 2), in every third of them in a z as well
            for v in range(1 + (j // len(wild)) % 3):
                out[i, (v + j) % 3, kind - 1] = wild[j % len(wild)]
            if j % 3 == 2:
                out[i, j % 3, 2] = wild[(j + 1) % len(wild)]
        else:  # a border value in all three vertices of x (kind 3) or y (kind 4)
            e = edges[kind - 3]
            out[i, :, kind - 3] = e[j % len(e)]
    return out.reshape(-1, 9)


def rotated(pos, first):
    """positions [n, 9] with component `first` (0 x, 1 y) of every vertex in the z slot (the other two moved up in turn): the z'
    plane of expected() on them is x' (y') — the same three-term sum — as a float32, which dx = x' - x no longer shows"""
    p = np.asarray(pos, np.float32).reshape(-1, 3, 3)
    order = [(first + 1) % 3, (first + 2) % 3, first]
    return np.ascontiguousarray(p[:, :, order]).reshape(-1, 9)
