"""not-gpu: the image-based-lighting passes' five entry points are declared, exported and bound, their argument tables agree with the
header's prototypes, the header states the rules, and without a context the calls refuse."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_frameset_reflect", "srz_frameset_reflect_grad", "srz_brdf_table", "srz_frameset_ibl", "srz_frameset_ibl_grad")


def test_header_states_the_rules_under_the_same_abi_version():
    assert "#define SRZ_ABI_VERSION 7" in HEADER and "#define SRZ_BRDF_TABLE_MAX 64u" in HEADER
    assert "(additive, same version) image-based lighting over a visibility buffer, with gradients" in HEADER
    for words in ("R_c = fmaf(t2, N_c, -Vd_c)", "Plane 3 is the RAW nv, not clamped", "THERE IS NO EYE GRADIENT in this ABI",
                  "minus the sum of that frame's d_gpos", "xi = fmaf(-q, q, 1)", "s = (a2 * xi) / fmaf(-xi, 1 - a2, 1)",
                  "take = vh > 0 && nl > 0", "A = fmaf(ra, wr, A)", "The sums run in THIS order whatever the launch shape",
                  "nvc = nv > 0 ? (nv < 1 ? nv : 1) : 0", "x0 = min((int)floorf(x), n - 2)", "out_c = fmaf(cdif_c, irr_c, spec_c * sc_c)",
                  "NO PLANE VALUE MAKES A PASS READ OUTSIDE THE TABLE", "d_gtab is ADDED INTO", "n 2^-24 / (1 - n 2^-24) * sum |term|",
                  "NO TRANSCENDENTAL FUNCTION"):
        assert words in HEADER, words


def test_binding_and_library_export_them():
    import srz
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("reflect", "reflect_grad", "ibl", "ibl_grad"):
        assert callable(getattr(srz.FrameSet, method))
    assert callable(srz.Context.brdf_table) and srz.abi.BRDF_TABLE_MAX == 64
    from srz import visibility
    for fn in ("reflect", "reflect_grad", "ibl", "ibl_grad", "brdf_table"):
        assert callable(getattr(visibility, fn))
    torch = __import__("torch")
    assert issubclass(visibility._Reflect, torch.autograd.Function) and issubclass(visibility._Ibl, torch.autograd.Function)


def test_argument_tables_match_the_prototypes():
    import srz
    from srz import abi
    L = srz.lib()
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    kinds = {"uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t}
    tables = (abi.REFLECT_ARGTYPES, abi.REFLECT_GRAD_ARGTYPES, abi.BRDF_TABLE_ARGTYPES, abi.IBL_ARGTYPES, abi.IBL_GRAD_ARGTYPES)
    for name, table in zip(ENTRY_POINTS, tables):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert want == table == list(getattr(L, name).argtypes), name


def test_without_a_context_they_refuse():
    import srz
    L, E = srz.lib(), srz.abi.SRZ_E_INVALID
    assert L.srz_frameset_reflect(None, None, None, None, None, None, 1, None, 0, 0, None) == E
    assert L.srz_frameset_reflect_grad(None, None, None, None, None, None, 1, None, None, None, 0, None) == E
    assert L.srz_brdf_table(None, None, 0, 8, 16, None) == E
    assert L.srz_frameset_ibl(None, None, None, None, None, None, None, None, None, 8, None, 0, 0, None) == E
    assert L.srz_frameset_ibl_grad(None, None, None, None, None, None, None, None, None, 8, None, None, None, None, None, None, None, 0, None) == E


def test_wrapper_argument_checks_need_no_device():
    """the torch layer refuses malformed arguments before anything reaches the library"""
    import torch
    from srz import visibility

    class FS:
        n_frames = 2

        def interpolate_shape(self, c):
            return (2, c, 8, 8)
    z = lambda c: torch.zeros(2, c, 8, 8)  # noqa: E731
    with pytest.raises(ValueError):
        visibility.reflect_grad(FS(), None, z(3), z(3), torch.zeros(3), z(4), want_gnrm=False, want_gpos=False)
    with pytest.raises(ValueError):
        visibility._reflect_args(FS(), z(3), z(3), torch.zeros(3))  # not on the device
    with pytest.raises(ValueError):
        visibility.ibl_grad(FS(), None, None, z(2), z(1), z(3), z(3), torch.zeros(4, 4, 2), z(3), want_gmat=False, want_gnv=False,
                            want_girr=False, want_gspec=False, want_gtab=False)  # (gbase without base is not a wish)
    with pytest.raises(ValueError):
        visibility._ibl_args(FS(), None, z(2), z(1), z(3), z(3), torch.zeros(4, 4, 2))  # not on the device
    for n, m in ((1, 8), (65, 8), (8, 0), (8, 257)):
        with pytest.raises(ValueError):
            visibility.brdf_table(None, n, m)
