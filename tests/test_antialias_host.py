"""not-gpu: the silhouette antialiasing entry points are declared under the same ABI version, exported and bound, and refuse an
all-null call."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
NAMES = ("srz_frameset_antialias", "srz_frameset_antialias_grad")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"int\s+srz_frameset_antialias\s*\(\s*srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*const void\s*\*d_in,\s*"
                     r"uint32_t n_ch,\s*void\s*\*d_out,\s*size_t out_bytes,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert re.search(r"int\s+srz_frameset_antialias_grad\s*\(\s*srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*const void\s*\*d_in,\s*"
                     r"const void\s*\*d_gout,\s*uint32_t n_ch,\s*void\s*\*d_gin,\s*uint32_t pos_tris,\s*float\s*\*d_gpos,\s*uint32_t flags,\s*"
                     r"void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER and "(additive, same version) silhouette antialiasing of a visibility buffer" in HEADER
    comment = HEADER[HEADER.index("SILHOUETTE ANTIALIASING"):HEADER.index("int srz_frameset_antialias(")]
    assert "(coarse-grained) device memory" in comment and "n_ch = 4" in comment and "DO reach results" in comment


def test_binding_and_library_export_them():
    import srz
    from srz import visibility
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in NAMES:
        assert name in srz.EXPORTS and hasattr(lib, name)
    assert callable(srz.FrameSet.antialias) and callable(srz.FrameSet.antialias_grad)
    assert callable(visibility.antialias) and callable(visibility.antialias_grad)
    L = srz.lib()
    assert L.srz_abi_version() == 7
    assert L.srz_frameset_antialias(None, None, None, None, 0, None, 0, 0, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_frameset_antialias_grad(None, None, None, None, None, 0, None, 0, None, 0, None) == srz.abi.SRZ_E_INVALID
