"""not-gpu: the position gradient's entry point is declared under the same ABI version, exported and bound, and refuses an all-null
call."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
NAME = "srz_frameset_position_grad"


def test_header_declares_the_entry_point_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"int\s+srz_frameset_position_grad\s*\(\s*srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*"
                     r"const void\s*\*d_gbary,\s*const void\s*\*d_gz,\s*uint32_t pos_tris,\s*float\s*\*d_gpos,\s*void\s*\*d_gpix,\s*"
                     r"uint32_t flags,\s*void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER and "(additive, same version) position gradients of a visibility buffer" in HEADER
    assert "(coarse-grained) device memory" in HEADER[HEADER.index("POSITION GRADIENTS"):HEADER.index("int srz_frameset_position_grad")]


def test_binding_and_library_export_it():
    import srz
    from srz import visibility
    lib = ctypes.CDLL(srz.LIB_PATH)
    assert NAME in srz.EXPORTS and hasattr(lib, NAME)
    assert callable(srz.FrameSet.position_grad)
    for fn in ("position_grad", "interpolate_geo", "depth"):
        assert callable(getattr(visibility, fn))
    L = srz.lib()
    assert L.srz_abi_version() == 7
    assert L.srz_frameset_position_grad(None, None, None, None, None, 0, None, None, 0, None) == srz.abi.SRZ_E_INVALID
