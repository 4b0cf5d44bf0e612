"""not-gpu: the attribute interpolation's three entry points are declared, exported and bound, and the Python side agrees with the
header on the channel cap."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_frameset_interpolate_bytes", "srz_frameset_interpolate", "srz_frameset_interpolate_grad")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"size_t\s+srz_frameset_interpolate_bytes\s*\(\s*const srz_ctx\s*\*\w*,\s*const srz_frameset\s*\*\w*,\s*uint32_t \w+\)", code)
    assert re.search(r"int\s+srz_frameset_interpolate\s*\([^)]*const float\s*\*d_attr,\s*uint32_t n_ch,\s*uint32_t attr_frames,\s*"
                     r"uint32_t attr_tris,\s*void\s*\*d_out,\s*size_t out_bytes,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert re.search(r"int\s+srz_frameset_interpolate_grad\s*\([^)]*const void\s*\*d_gout,\s*const float\s*\*d_attr,\s*uint32_t n_ch,\s*"
                     r"uint32_t attr_frames,\s*uint32_t attr_tris,\s*float\s*\*d_gattr,\s*void\s*\*d_gbary,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER and "(additive, same version) caller attributes over a visibility buffer" in HEADER
    assert "NOT BIT-REPRODUCIBLE" in HEADER


def test_binding_and_library_export_them():
    import srz
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("interpolate", "interpolate_bytes", "interpolate_shape", "interpolate_grad"):
        assert callable(getattr(srz.FrameSet, method))
    from srz import visibility
    assert callable(visibility.interpolate) and callable(visibility.interpolate_bary_grad)
    L = srz.lib()
    assert L.srz_frameset_interpolate_bytes(None, None, 0) == 0 and L.srz_frameset_interpolate_bytes(None, None, 65) == 0
    assert L.srz_frameset_interpolate_bytes(None, None, 4) == 0
    assert L.srz_frameset_interpolate(None, None, None, None, 4, 1, 1, None, 0, 0, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_frameset_interpolate_grad(None, None, None, None, None, 4, 1, 1, None, None, 0, None) == srz.abi.SRZ_E_INVALID


def test_channel_cap_equals_the_headers():
    from srz import abi
    m = re.search(r"#define SRZ_ATTR_MAX_CH\s+(\d+)u", HEADER)
    assert m and int(m.group(1)) == abi.ATTR_MAX_CH == 64
