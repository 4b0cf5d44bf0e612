"""not-gpu: the four entry points of tangent-space normal mapping are declared, exported and bound, their argument tables agree with
the header's prototypes, and without a context they refuse."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_mesh_tangents", "srz_mesh_tangents_grad", "srz_frameset_normal_map", "srz_frameset_normal_map_grad")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(srz_ctx\s*\*ctx," % name, code), name
    assert "#define SRZ_ABI_VERSION 7" in HEADER
    assert "(additive, same version) tangent-space normal mapping over a visibility buffer" in HEADER
    # the rules' pieces are stated: the weighting, the handedness convention, both orders of operations, what has no gradient
    for words in ("Tf  = e1 * dv2 - e2 * dv1", "S = S + s * Tf;   D = D + det", "w * cross(N, t) points along +v", "TO THE POSITIONS ONLY",
                  "its w float is NEVER READ", "co = s * (dv1 - dv2)", "R_c = fmaf(m.x, T_c, fmaf(m.y, B_c, m.z * N_c))",
                  "gN_c = (gN_c - gTp_c * d) + gd * t_c", "there is no gradient to the handedness", "SRZ_OPT_APPROX_SHADE has no effect"):
        assert words in HEADER, words


def test_binding_and_library_export_them():
    import srz
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("mesh_tangents", "mesh_tangents_grad"):
        assert callable(getattr(srz.Context, method))
    for method in ("normal_map", "normal_map_grad"):
        assert callable(getattr(srz.FrameSet, method))
    from srz import visibility
    assert callable(visibility.mesh_tangents) and callable(visibility.normal_map) and callable(visibility.normal_map_grad)
    Function = __import__("torch").autograd.Function
    assert issubclass(visibility._MeshTangents, Function) and issubclass(visibility._NormalMap, Function)


def test_argument_tables_match_the_prototypes():
    import srz
    from srz import abi
    L = srz.lib()
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    kinds = {"uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t, "int": ctypes.c_int}
    tables = (abi.MESH_TANGENTS_ARGTYPES, abi.MESH_TANGENTS_GRAD_ARGTYPES, abi.NORMAL_MAP_ARGTYPES, abi.NORMAL_MAP_GRAD_ARGTYPES)
    for name, table in zip(ENTRY_POINTS, tables):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert want == table == list(getattr(L, name).argtypes), name
    assert [len(t) for t in tables] == [10, 12, 10, 12]


def test_without_a_context_they_refuse():
    import srz
    L, E = srz.lib(), srz.abi.SRZ_E_INVALID
    assert L.srz_mesh_tangents(None, 0, None, 3, 1, None, 2, None, 4, None) == E
    assert L.srz_mesh_tangents_grad(None, 0, None, 3, 1, None, 2, None, 4, None, None, None) == E
    assert L.srz_frameset_normal_map(None, None, None, None, None, None, None, 0, 0, None) == E
    assert L.srz_frameset_normal_map_grad(None, None, None, None, None, None, None, None, None, None, 0, None) == E


def test_wrapper_argument_checks_need_no_device():
    """the torch layer refuses malformed planes before anything reaches the library"""
    import pytest
    import torch
    from srz import visibility

    class FS:
        n_frames = 2

        def interpolate_shape(self, c):
            return (2, c, 8, 8)
    with pytest.raises(ValueError):
        visibility.normal_map_grad(FS(), None, None, None, None, None, False, False, False)
    n, t, m = torch.zeros(2, 3, 8, 8), torch.zeros(2, 4, 8, 8), torch.zeros(2, 3, 8, 8)
    for bad in ((n, n, m), (t, t, m), (n, t, t), (n.double(), t, m)):  # (and every tensor is on the CPU: refused as well)
        with pytest.raises(ValueError):
            visibility.normal_map(FS(), None, *bad)
