"""The SH9 passes' test reference (tests/sh_ref.c holds the arithmetic, stated once in a `real` type and built as binary32 — the rule
itself — and as binary64): a cube → nine coefficients per channel in the header's fixed tree, its backward gather, the coefficients
evaluated at each pixel's normal, and that pass's backward with the coefficient gradient accumulated in double with sum |term| and
counts.  Built and loaded like tests/lightref.py's library; nothing of the product is involved.  Also here: the same rules in torch
float64 ops (autograd differentiates them), and what the CPU and GPU tests share."""
import ctypes as C
import math

import numpy as np

from support import ref_lib

OWNED, LIT = 1, 2  # classify()'s pixel bits
IRRADIANCE, RADIANCE = 0, 1
SH_MAX_CH = 7
# the header's constants, as the binary32 values they are
YC = np.array([float.fromhex(h) for h in ("0x1.20dd76p-2", "0x1.f45438p-2", "0x1.17b142p+0", "0x1.42f602p-2", "0x1.17b142p-1")], np.float64)
HC = np.array([float.fromhex(h) for h in ("0x1.20dd76p-2", "0x1.4d8d7ap-2", "0x1.17b142p-2", "0x1.42f602p-4", "0x1.17b142p-3")], np.float64)
CIDX = np.array([0, 1, 1, 1, 2, 2, 3, 2, 4])
FOURPI = float(np.float32(12.566371))
vp, u32 = C.c_void_p, C.c_uint32
SIGNATURES = {}
for _b in ("sr32_", "sr64_"):
    SIGNATURES[_b + "cube_sh"] = (None, [u32, u32, u32, vp, vp, vp])
    SIGNATURES[_b + "cube_sh_grad"] = (None, [u32, u32, u32, vp, vp, vp])
    SIGNATURES[_b + "forward"] = (None, [C.c_size_t, u32, vp, vp, vp, u32, C.c_int, C.c_int, vp])
    SIGNATURES[_b + "grad"] = (None, [C.c_size_t, u32, vp, vp, vp, u32, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp])
    SIGNATURES[_b + "classify"] = (None, [C.c_size_t, u32, vp, vp, vp])


def lib(tmpdir):
    return ref_lib("sh_ref", tmpdir, SIGNATURES)


def _p(a):
    return a.ctypes.data if a is not None else None


def _fn(tmpdir, name, dtype):
    return getattr(lib(tmpdir), ("sr32_" if dtype == np.float32 else "sr64_") + name)


# ------------------------------------------------------------------------------------------------ the cube pass
def cube_sh(tmpdir, cube, dtype=np.float32):
    """cube [frames, 6, n, n, C] → (sh [frames, 9, C], den [1]) of dtype, in the fixed tree"""
    cube = np.ascontiguousarray(cube, dtype)
    frames, six, n, n2, ch = cube.shape
    assert six == 6 and n == n2 and 1 <= ch <= SH_MAX_CH
    sh, den = np.zeros((frames, 9, ch), dtype), np.zeros(1, dtype)
    _fn(tmpdir, "cube_sh", dtype)(n, ch, frames, _p(cube), _p(sh), _p(den))
    return sh, den


def cube_sh_grad(tmpdir, gsh, den, n, dtype=np.float32):
    """gsh [frames, 9, C], den [1] → gsrc [frames, 6, n, n, C] of dtype"""
    gsh, den = np.ascontiguousarray(gsh, dtype), np.ascontiguousarray(den, dtype).reshape(1)
    frames, nine, ch = gsh.shape
    assert nine == 9
    gsrc = np.zeros((frames, 6, n, n, ch), dtype)
    _fn(tmpdir, "cube_sh_grad", dtype)(n, ch, frames, _p(gsh), _p(den), _p(gsrc))
    return gsrc


# ------------------------------------------------------------------------------------------------ the pixel pass
def _args(ids, nrm, sh, dtype):
    ids = np.ascontiguousarray(ids, np.uint32)
    nrm = np.ascontiguousarray(nrm, dtype)
    assert nrm.shape == (3,) + ids.shape, (nrm.shape, ids.shape)
    sh = np.ascontiguousarray(sh, dtype)
    assert sh.ndim == 2 and sh.shape[0] == 9 and 1 <= sh.shape[1] <= SH_MAX_CH
    return ids, nrm, sh, sh.shape[1]


def _fresh(shape, prefill, dtype):
    if prefill is None:
        return np.zeros(shape, dtype)
    assert dtype == np.float32
    return np.array(prefill, np.uint32, copy=True, order="C").view(np.float32)


def forward(tmpdir, n_tris, ids, nrm, sh, kind, fused=True, prefill=None, dtype=np.float32):
    """ids [rows, W] uint32 (plane 1 of one frame's visibility buffer), nrm [3, rows, W], sh [9, C] → [C, rows, W] of dtype.
    prefill: [C, rows, W] uint32 words the float32 planes start from (not fused: nobody's words stay)."""
    ids, nrm, sh, ch = _args(ids, nrm, sh, dtype)
    out = _fresh((ch,) + ids.shape, prefill, dtype)
    _fn(tmpdir, "forward", dtype)(ids.size, n_tris, _p(ids), _p(nrm), _p(sh), ch, kind, int(fused), _p(out))
    return out


class Grad:
    """the coefficient gradient of any number of frames, accumulated in double: .gsum [9, C] float64, .gabs the sums of |term|,
    .count [9, C] the contributing pixels per entry"""

    def __init__(self, n_ch):
        self.gsum, self.gabs, self.count = np.zeros((9, n_ch), np.float64), np.zeros((9, n_ch), np.float64), np.zeros((9, n_ch), np.uint32)

    def bound(self, extra=0):
        """per entry: gamma_n * sum |term|, gamma_n = n u / (1 - n u), u = 2^-24, n the entry's contributing pixels (+ extra: further
        roundings of the same sum, such as adding the ranks' or frames' partial results): the bound of any summation tree"""
        n = (self.count.astype(np.float64) + extra) * 2.0 ** -24
        return n / (1.0 - n) * self.gabs


def grad(tmpdir, n_tris, ids, nrm, sh, kind, gout, into=None, fused=True, prefill=None, want_terms=False, dtype=np.float32):
    """one frame's share: adds into `into` (a Grad, or None) and returns gnrm [3, rows, W], and with want_terms the per-pixel terms
    [9, C, rows, W] too"""
    ids, nrm, sh, ch = _args(ids, nrm, sh, dtype)
    gout = np.ascontiguousarray(gout, dtype)
    assert gout.shape == (ch,) + ids.shape
    gnrm = _fresh(nrm.shape, prefill, dtype)
    terms = np.zeros((9, ch) + ids.shape, dtype) if want_terms else None
    _fn(tmpdir, "grad", dtype)(ids.size, n_tris, _p(ids), _p(nrm), _p(sh), ch, kind, _p(gout), int(fused), _p(gnrm),
                               _p(into.gsum) if into else None, _p(into.gabs) if into else None, _p(into.count) if into else None, _p(terms))
    return (gnrm, terms) if want_terms else gnrm


def classify(tmpdir, n_tris, ids, nrm):
    """[rows, W] uint8: OWNED | LIT by the binary32 rule"""
    ids = np.ascontiguousarray(ids, np.uint32)
    nrm = np.ascontiguousarray(nrm, np.float32)
    cls = np.zeros(ids.shape, np.uint8)
    lib(tmpdir).sr32_classify(ids.size, n_tris, _p(ids), _p(nrm), _p(cls))
    return cls


# ------------------------------------------------------------------------------------------------ the rules in numpy / torch float64
def basis(d, consts=YC, xp=np):
    """[9, ...] : consts[k] * p_k(d) for unit vectors d [3, ...] (numpy or torch by xp)"""
    x, y, z = d[0], d[1], d[2]
    one = xp.ones_like(x)
    p = [one, y, z, x, x * y, y * z, 3.0 * z * z - 1.0, x * z, x * x - y * y]
    return xp.stack([float(consts[CIDX[k]]) * p[k] for k in range(9)])


def cube_geometry(n):
    """(d [3, 6, n, n], jac [6, n, n]) float64: the texel geometry of srz_cube_prefilter's header text"""
    c = (2.0 * np.arange(n) + 1.0) / n - 1.0
    t, s = np.meshgrid(c, c, indexing="ij")  # [y, x]
    one = np.ones_like(s)
    p = np.stack([np.stack(v) for v in ((one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one))])  # [6, 3, n, n]
    inv = 1.0 / np.sqrt(s * s + t * t + 1.0)
    return np.ascontiguousarray((p * inv).transpose(1, 0, 2, 3)), np.broadcast_to(inv ** 3, (6, n, n)).copy()


def torch_cube_rule(cube):
    """cube_sh's rule in torch ops of the cube's dtype, torch's own summation order: [..., 6, n, n, C] → [..., 9, C]"""
    import torch
    n = cube.shape[-2]
    d, jac = cube_geometry(n)
    w = torch.as_tensor(basis(d) * jac, dtype=cube.dtype, device=cube.device)  # [9, 6, n, n]
    den = torch.as_tensor(jac.sum(), dtype=cube.dtype, device=cube.device)
    return FOURPI * torch.einsum("kfyx,...fyxc->...kc", w, cube) / den


def torch_rule(sh, nrm, kind):
    """srz_frameset_sh's rule on planes [..., 3, rows, W] with torch ops in the tensors' dtype, every pixel taken as owned; sh [9, C]
    or [frames, 9, C] (then nrm [frames, 3, rows, W]).  Differentiable by autograd: the lit branch is held by torch.where on a
    detached condition, exactly the derivative the backward states."""
    import torch
    nn = (nrm * nrm).sum(-3, keepdim=True)
    lit = (nn.detach() > 0) & (nn.detach() < float("inf"))
    N = nrm / torch.where(lit, nn, torch.ones_like(nn)).sqrt()
    e = basis(N.movedim(-3, 0), YC if kind == RADIANCE else HC, torch)  # [9, ..., rows, W]
    if sh.dim() == 3:
        out = torch.einsum("kfyx,fkc->fcyx", e, sh)
    else:
        out = torch.einsum("k...yx,kc->...cyx", e, sh)
    return torch.where(lit, out, torch.zeros((), dtype=nrm.dtype, device=nrm.device))



# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
def make_sh(seed, n_ch, frames=None):
    """coefficients [9, C] (or [frames, 9, C]) float32: a positive DC term and smaller higher bands, deterministic"""
    rng = np.random.default_rng([seed, n_ch])
    n = 1 if frames is None else frames
    sh = rng.normal(0, 0.4, (n, 9, n_ch))
    sh[:, 0] = rng.uniform(1.0, 3.0, (n, n_ch))
    sh = np.ascontiguousarray(sh, np.float32)
    return sh[0] if frames is None else sh


def make_planes(seed, shape, n_ch):
    """(nrm [3, rows, W], gout [C, rows, W]) float32: normals of any length and every direction, gout normal"""
    rng = np.random.default_rng([seed, n_ch, *shape])
    rows, W = shape
    nrm = rng.normal(0, 1.0, (3, rows, W)) * rng.uniform(0.5, 3.0, (1, rows, W))
    gout = rng.normal(0, 1, (n_ch, rows, W))
    return np.ascontiguousarray(nrm, np.float32), np.ascontiguousarray(gout, np.float32)


SPECIAL_NORMALS = np.float32([
    [0.0, 0.0, 0.0], [-0.0, 0.0, -0.0],                        # zero: not lit
    [1e-40, -3e-42, 2e-41], [1e-30, 0.0, 0.0],                 # all subnormal / tiny: nn underflows to 0, not lit
    [1e-40, 1.0, -2.0],                                        # one subnormal component among ordinary ones: lit
    [3e38, 1.0, 0.0], [1e20, -1e20, 1e19],                     # huge: nn overflows to inf, not lit
    [1e18, 1e18, -1e18],                                       # large and finite: lit
    [np.inf, 0.0, 1.0], [0.0, -np.inf, 0.0], [np.nan, 1.0, 0.0], [1.0, 2.0, np.nan],  # inf and NaN: not lit
    [0.0, 0.0, 1.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0],        # the axes: polynomials exactly 0
])


def hostile_planes(rng, shape, n_ch):
    """(nrm, gout) by hand: make_planes with every SPECIAL_NORMALS row at a pixel in three, and non-finite gout at one pixel in
    twenty"""
    nrm, gout = make_planes(int(rng.integers(1 << 30)), shape, n_ch)
    hit = rng.random(shape) < 1 / 3
    pick = rng.integers(0, len(SPECIAL_NORMALS), shape)
    nrm[:, hit] = SPECIAL_NORMALS[pick[hit]].T
    bad = rng.random((n_ch,) + shape) < 0.05
    gout[bad] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 3e38, -0.0, 1e-40]), int(bad.sum()))
    return nrm, gout


def make_cube(seed, n, n_ch, frames=1):
    """[frames, 6, n, n, C] float32: positive radiance with some spread"""
    rng = np.random.default_rng([seed, n, n_ch, frames])
    return np.ascontiguousarray(rng.uniform(0.0, 2.0, (frames, 6, n, n, n_ch)) ** 2, np.float32)


def same_words(a, b):
    """bit-equal float32 arrays, except that a NaN on one side is any NaN on the other"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


assert math.isclose(FOURPI, 4 * math.pi, rel_tol=1e-7)
