"""not-gpu: the motion pass's two entry points are declared, exported and bound, and the Python side agrees with the header on the
group constants."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_frameset_motion_bytes", "srz_frameset_motion")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"size_t\s+srz_frameset_motion_bytes\s*\(\s*const srz_ctx\s*\*\w*,\s*const srz_frameset\s*\*\w*,\s*uint32_t \w+\)", code)
    assert re.search(r"int\s+srz_frameset_motion\s*\([^)]*uint32_t what,\s*int delta,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER and "(additive, same version) the motion pass" in HEADER
    assert "LINEAR IN SCREEN SPACE" in HEADER


def test_binding_and_library_export_them():
    import srz
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("motion", "motion_bytes", "motion_shape"):
        assert callable(getattr(srz.FrameSet, method))
    assert srz.lib().srz_frameset_motion_bytes(None, None, 7) == 0
    assert srz.lib().srz_frameset_motion(None, None, None, None, 0, 7, 1, 0, None) == srz.abi.SRZ_E_INVALID


def test_group_constants_equal_the_headers():
    from srz import abi
    for name in ("FLOW", "DEPTH", "TARGET"):
        m = re.search(r"#define SRZ_MV_%s\s+(\d+)u" % name, HEADER)
        assert m and int(m.group(1)) == getattr(abi, "MV_" + name), name
    assert (abi.MV_FLOW, abi.MV_DEPTH, abi.MV_TARGET, abi.MV_ALL) == (1, 2, 4, 7)
