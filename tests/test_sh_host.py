"""not-gpu: the SH9 passes' six entry points are declared, exported and bound, their argument tables agree with the header's
prototypes, the header states the constants and the rules, and without a context the calls refuse."""
import ctypes
import os
import re
import struct

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_cube_sh_work_bytes", "srz_cube_sh", "srz_cube_sh_grad", "srz_frameset_sh", "srz_frameset_sh_work_bytes",
                "srz_frameset_sh_grad")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"size_t\s+srz_cube_sh_work_bytes\s*\(uint32_t n,\s*uint32_t n_ch,\s*uint32_t tex_frames\)", code)
    assert re.search(r"int\s+srz_cube_sh\s*\(srz_ctx\s*\*ctx,\s*const float\s*\*d_src,\s*uint32_t n,\s*uint32_t n_ch,\s*uint32_t tex_frames,\s*"
                     r"float\s*\*d_sh,\s*float\s*\*d_den,\s*void\s*\*d_work,\s*size_t work_bytes,\s*void\s*\*stream\)", code)
    assert re.search(r"int\s+srz_cube_sh_grad\s*\(srz_ctx\s*\*ctx,\s*const float\s*\*d_gsh,\s*const float\s*\*d_den,\s*uint32_t n,\s*uint32_t n_ch,\s*"
                     r"uint32_t tex_frames,\s*float\s*\*d_gsrc,\s*void\s*\*d_work,\s*size_t work_bytes,\s*void\s*\*stream\)", code)
    assert re.search(r"int\s+srz_frameset_sh\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*const void\s*\*d_nrm,\s*"
                     r"const float\s*\*d_sh,\s*uint32_t n_ch,\s*uint32_t sh_frames,\s*uint32_t kind,\s*void\s*\*d_out,\s*size_t out_bytes,\s*"
                     r"uint32_t flags,\s*void\s*\*stream\)", code)
    assert re.search(r"size_t\s+srz_frameset_sh_work_bytes\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*uint32_t n_ch\)", code)
    assert re.search(r"int\s+srz_frameset_sh_grad\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*const void\s*\*d_nrm,\s*"
                     r"const float\s*\*d_sh,\s*uint32_t n_ch,\s*uint32_t sh_frames,\s*uint32_t kind,\s*const void\s*\*d_gout,\s*void\s*\*d_gnrm,\s*"
                     r"float\s*\*d_gsh,\s*void\s*\*d_work,\s*size_t work_bytes,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER
    assert "(additive, same version) SH9 lighting" in HEADER
    assert re.search(r"#define\s+SRZ_SH_MAX_CH\s+7\b", code)
    assert re.search(r"#define\s+SRZ_SH_IRRADIANCE\s+0u", code) and re.search(r"#define\s+SRZ_SH_RADIANCE\s+1u", code)
    # the rules' pieces are stated: the polynomials, the fixed trees, the division, the backward's order, reproducibility
    for words in ("p = 1, y, z, x, x * y, y * z, fmaf(3.0f * z, z, -1.0f), x * z, fmaf(x, x, -(y * y))", "0, 1, 1, 1, 2, 2, 3, 2, 4",
                  "b_k = Yc[k] * p_k(d);  w_k = jac * b_k", "lane j of 64 takes the columns j, j + 64", "v = v + v[lane ^ o], o = 32, 16, 8,",
                  "sh[k][c] = (FOURPI * num) / den", "q[k][c] = (FOURPI * gsh[k][c]) / den", "NO CLAMP",
                  "gN_x = fmaf(2.0f * x, gp_8, fmaf(gp_7, z, fmaf(gp_4, y, gp_3)))", "gN_y = fmaf(-2.0f * y, gp_8, fmaf(gp_5, z, fmaf(gp_4, x, gp_1)))",
                  "gN_z = fmaf(6.0f * z, gp_6, fmaf(gp_7, x, fmaf(gp_5, y, gp_2)))", "gn_i = (gN_i - N_i * d) * inl",
                  "srz_frameset_light_grad's FIXED tree, word for word", "BIT-REPRODUCIBLE", "WRITTEN, not added into"):
        assert words in HEADER, words


def test_the_constants_are_the_nearest_binary32():
    """every constant the header states, as a hex literal and as a bit pattern, is the binary32 nearest to the binary64 value; the
    H's products are taken in binary64 and rounded once; the reference carries the same values"""
    import math

    import numpy as np

    import shref
    pi = math.pi
    yc = [math.sqrt(1 / (4 * pi)), math.sqrt(3 / (4 * pi)), math.sqrt(15 / (4 * pi)), math.sqrt(5 / (16 * pi)), math.sqrt(15 / (16 * pi))]
    h = [yc[0], yc[1] * 2 / 3, yc[2] / 4, yc[3] / 4, yc[4] / 4]
    bits = (0x3e906ebb, 0x3efa2a1c, 0x3f8bd8a1, 0x3ea17b01, 0x3f0bd8a1)
    for i in range(5):
        for name, v, table in (("Yc", yc[i], shref.YC), ("H", h[i], shref.HC)):
            lit = re.search(r"\b%s%d = [^;]*?(0x1\.[0-9a-f]+p[+-]\d+)f" % (name, i), HEADER).group(1)
            assert float.fromhex(lit) == float(np.float32(v)) == table[i], (name, i)
        assert struct.unpack("<I", struct.pack("<f", yc[i]))[0] == bits[i] and "(0x%08x)" % bits[i] in HEADER
    assert "FOURPI = 12.566371f = 0x1.921fb6p+3f" in HEADER and float.fromhex("0x1.921fb6p+3") == float(np.float32(4 * pi)) == shref.FOURPI


def test_binding_and_library_export_them():
    import srz
    from srz import abi
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("sh", "sh_grad", "sh_work_bytes"):
        assert callable(getattr(srz.FrameSet, method))
    for method in ("cube_sh", "cube_sh_grad", "cube_sh_work_bytes"):
        assert callable(getattr(srz.Context, method))
    from srz import visibility
    for fn in ("sh_light", "sh_light_grad", "cube_sh", "cube_sh_grad"):
        assert callable(getattr(visibility, fn))
    torch = __import__("torch")
    assert issubclass(visibility._ShLight, torch.autograd.Function) and issubclass(visibility._CubeSh, torch.autograd.Function)
    assert abi.SH_MAX_CH == 7 and (abi.SH_IRRADIANCE, abi.SH_RADIANCE) == (0, 1)


def test_argument_tables_match_the_prototypes():
    import srz
    from srz import abi
    L = srz.lib()
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    kinds = {"uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t}
    tables = (abi.CUBE_SH_WORK_BYTES_ARGTYPES, abi.CUBE_SH_ARGTYPES, abi.CUBE_SH_GRAD_ARGTYPES, abi.SH_ARGTYPES, abi.SH_WORK_BYTES_ARGTYPES,
              abi.SH_GRAD_ARGTYPES)
    for name, table in zip(ENTRY_POINTS, tables):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert want == table == list(getattr(L, name).argtypes), name
    assert len(abi.SH_ARGTYPES) == 12 and len(abi.SH_GRAD_ARGTYPES) == 15 and len(abi.CUBE_SH_ARGTYPES) == 10
    assert L.srz_frameset_sh_work_bytes.restype is ctypes.c_size_t and L.srz_cube_sh_work_bytes.restype is ctypes.c_size_t


def test_without_a_context_they_refuse():
    import srz
    L = srz.lib()
    E = srz.abi.SRZ_E_INVALID
    assert L.srz_cube_sh(None, None, 8, 3, 1, None, None, None, 0, None) == E
    assert L.srz_cube_sh_grad(None, None, None, 8, 3, 1, None, None, 0, None) == E
    assert L.srz_frameset_sh(None, None, None, None, None, 3, 1, 0, None, 0, 0, None) == E
    assert L.srz_frameset_sh_grad(None, None, None, None, None, 3, 1, 0, None, None, None, None, 0, 0, None) == E
    assert L.srz_frameset_sh_work_bytes(None, None, 3) == 0


def test_cube_work_bytes_needs_no_context_and_refuses_sizes_out_of_range():
    """[frame][face][row][K] row partials, [frame][face][K] and [frame][K] behind them, K = 9 n_ch + 1"""
    import srz
    L = srz.lib()
    assert L.srz_cube_sh_work_bytes(8, 3, 2) == 2 * (6 * 8 + 7) * 28 * 4
    assert L.srz_cube_sh_work_bytes(1, 1, 1) == 13 * 10 * 4
    for n, c, f in ((0, 3, 1), (srz.abi.TEX_MAX_SIZE + 1, 3, 1), (8, 0, 1), (8, 8, 1), (8, 3, 0), (8, 3, 65537)):
        assert L.srz_cube_sh_work_bytes(n, c, f) == 0, (n, c, f)
    assert L.srz_cube_sh_work_bytes(srz.abi.TEX_MAX_SIZE, 7, 1) > 0


def test_wrapper_argument_checks_need_no_device():
    """the torch layer refuses what it can judge without a device before anything reaches the library: the normals (its first
    clause), a cube and a coefficient gradient on the host.  tests/test_gpu_sh_refusals.py has the clauses behind them."""
    import pytest
    import torch
    from srz import visibility

    class FS:
        n_frames = 2

        def interpolate_shape(self, c):
            return (2, c, 8, 8)
    sh = torch.zeros(9, 3)
    for nrm in (None, torch.zeros(2, 3, 8, 8), torch.zeros((2, 4, 8, 8), device="meta"), torch.zeros((2, 3, 8, 8), device="meta", dtype=torch.float64)):
        with pytest.raises(ValueError, match="sh_light: nrm must be a CUDA float32 tensor \\(2, 3, 8, 8\\)"):
            visibility.sh_light(FS(), None, sh, nrm)
    with pytest.raises(ValueError, match="cube_sh: a cube is a CUDA float32 tensor"):
        visibility.cube_sh(object(), torch.zeros(6, 4, 4, 3))
    with pytest.raises(ValueError, match="cube_sh_grad: gsh must be a CUDA float32 tensor"):
        visibility.cube_sh_grad(object(), torch.zeros(9, 3), torch.zeros(1), 4)
