"""not-gpu: the composite pass's two entry points are declared, exported and bound, their argument tables agree with the header's
prototypes, the layer struct mirrors the header's, the header states the rule, and without a context the calls refuse."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_frameset_composite", "srz_frameset_composite_grad")


def test_header_states_the_rule_under_the_same_abi_version():
    assert "#define SRZ_ABI_VERSION 7" in HEADER and "#define SRZ_COMPOSITE_MAX 8" in HEADER
    assert "(additive, same version) compositing depth layers front to back, with gradients" in HEADER
    for words in ("w = a * T;   acc_c = acc_c + col_c * w   for every channel c;   T = T * (1 - a)", "acc_c = acc_c + bg_c * T",
                  "THERE IS NO CLAMP OF a AND NO", "EARLY EXIT at T == 0", "EVERY WORD OF d_out IN THE SHARD'S OWNED ROWS IS WRITTEN",
                  "THE LAYERS NEED NOT COME FROM ONE PEEL CHAIN", "never reach a result", "gbg_c = g_c * T_n",
                  "S = fmaf(g_c, bg_c, S) for c = 0, 1, .. in channel order", "FROM LAST TO FIRST", "d = fmaf(g_c, col_c, d) for c = 0, 1, ..",
                  "gcol_c = g_c * w_k", "galpha = T_k * (d - S)", "S = fmaf(a, d, (1 - a) * S)", "No division appears, so a = 1 is an ordinary value",
                  "+0 where", "BIT-REPRODUCIBLE", "d_gbg without d_bg", "inputs may alias each other"):
        assert words in HEADER, words


def test_binding_and_library_export_them():
    import srz
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("composite", "composite_grad"):
        assert callable(getattr(srz.FrameSet, method))
    assert srz.abi.COMPOSITE_MAX == 8
    from srz import visibility
    for fn in ("composite_layers", "composite_grad", "composite"):
        assert callable(getattr(visibility, fn))
    torch = __import__("torch")
    assert issubclass(visibility._CompositeLayers, torch.autograd.Function)
    assert "composite_layers" in visibility.composite.__doc__


def test_argument_tables_match_the_prototypes():
    import srz
    from srz import abi
    L = srz.lib()
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    kinds = {"uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t}
    for name, table in zip(ENTRY_POINTS, (abi.COMPOSITE_ARGTYPES, abi.COMPOSITE_GRAD_ARGTYPES)):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert want == table == list(getattr(L, name).argtypes), name


def test_the_layer_struct_mirrors_the_headers():
    from srz import abi
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    body = re.search(r"typedef struct srz_composite_layer \{(.*?)\} srz_composite_layer;", code, flags=re.S).group(1)
    fields = [f.split()[-1].lstrip("*") for f in body.split(";") if f.strip()]
    assert fields == [name for name, _ in abi.SrzCompositeLayer._fields_] == ["vis", "color", "alpha", "opacity", "_pad"]
    assert ctypes.sizeof(abi.SrzCompositeLayer) == 32 and abi.SrzCompositeLayer.opacity.offset == 24
    arr = abi.composite_layers_array([(16, 32, None, 0.5), (48, 64, 80, 0.0)])
    assert (arr[0].vis, arr[0].color, arr[0].alpha, arr[0].opacity) == (16, 32, None, 0.5) and arr[1].alpha == 80


def test_without_a_context_they_refuse():
    import srz
    L, E = srz.lib(), srz.abi.SRZ_E_INVALID
    assert L.srz_frameset_composite(None, None, None, 1, 3, None, 0, None, 0, 0, None) == E
    assert L.srz_frameset_composite_grad(None, None, None, 1, 3, None, 0, None, None, None, None, 0, None) == E


def test_wrapper_argument_checks_need_no_device():
    """the torch layer refuses malformed arguments before anything reaches the library"""
    import torch
    from srz import visibility

    class FS:
        n_frames = 2
        out_shape = (2, 4, 8, 8)

        def interpolate_shape(self, c):
            return (2, c, 8, 8)
    z = lambda c: torch.zeros(2, c, 8, 8)  # noqa: E731
    with pytest.raises(ValueError):
        visibility.composite_layers(FS(), [z(4)], [z(3), z(3)], [0.5])  # the counts differ
    with pytest.raises(ValueError):
        visibility.composite_layers(FS(), [], [], [])
    with pytest.raises(ValueError):
        visibility.composite_layers(FS(), [z(4)] * 9, [z(3)] * 9, [0.5] * 9)  # above COMPOSITE_MAX
    with pytest.raises(ValueError):
        visibility.composite_layers(FS(), [z(4)], [z(3)], [0.5])  # not on the device
    with pytest.raises(ValueError):
        visibility.composite_grad(FS(), [z(4)], [z(3)], [0.5], z(3))  # not on the device
