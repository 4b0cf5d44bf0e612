"""not-gpu: the texture pass's two entry points are declared, exported and bound, and the Python side agrees with the header on the
modes and on the size cap."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_frameset_texture", "srz_frameset_texture_grad")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"int\s+srz_frameset_texture\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*const void\s*\*d_uv,\s*"
                     r"const float\s*\*d_tex,\s*uint32_t tex_w,\s*uint32_t tex_h,\s*uint32_t n_ch,\s*uint32_t tex_frames,\s*uint32_t mode,\s*"
                     r"void\s*\*d_out,\s*size_t out_bytes,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert re.search(r"int\s+srz_frameset_texture_grad\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*const void\s*\*d_uv,\s*"
                     r"const void\s*\*d_gout,\s*const float\s*\*d_tex,\s*uint32_t tex_w,\s*uint32_t tex_h,\s*uint32_t n_ch,\s*uint32_t tex_frames,\s*"
                     r"uint32_t mode,\s*float\s*\*d_gtex,\s*void\s*\*d_guv,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER and "(additive, same version) caller textures over a visibility buffer" in HEADER
    assert HEADER.count("NOT BIT-REPRODUCIBLE") >= 4  # gattr, gpos twice, gtex


def test_binding_and_library_export_them():
    import srz
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("texture", "texture_grad"):
        assert callable(getattr(srz.FrameSet, method))
    from srz import visibility
    assert callable(visibility.texture) and callable(visibility.texture_grad)
    L = srz.lib()
    assert len(L.srz_frameset_texture.argtypes) == 14 and len(L.srz_frameset_texture_grad.argtypes) == 15
    assert L.srz_frameset_texture(None, None, None, None, None, 4, 4, 3, 1, 0, None, 0, 0, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_frameset_texture_grad(None, None, None, None, None, None, 4, 4, 3, 1, 0, None, None, 0, None) == srz.abi.SRZ_E_INVALID


def test_constants_equal_the_headers():
    from srz import abi
    for name, value in (("SRZ_TEX_CLAMP", abi.TEX_CLAMP), ("SRZ_TEX_WRAP", abi.TEX_WRAP), ("SRZ_TEX_MAX_SIZE", abi.TEX_MAX_SIZE)):
        m = re.search(r"#define %s\s+(\d+)u" % name, HEADER)
        assert m and int(m.group(1)) == value, name
    assert (abi.TEX_CLAMP, abi.TEX_WRAP, abi.TEX_MAX_SIZE) == (0, 1, 16384)
