"""not-gpu: the cube lookup's two entry points are declared, exported and bound, their argument tables agree with the header's
prototypes, and without a context they refuse."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_frameset_texture_cube", "srz_frameset_texture_cube_grad")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"int\s+srz_frameset_texture_cube\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*const void\s*\*d_dir,\s*"
                     r"const float\s*\*d_tex,\s*uint32_t n,\s*uint32_t n_ch,\s*uint32_t tex_frames,\s*void\s*\*d_out,\s*size_t out_bytes,\s*"
                     r"uint32_t flags,\s*void\s*\*stream\)", code)
    assert re.search(r"int\s+srz_frameset_texture_cube_grad\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*"
                     r"const void\s*\*d_dir,\s*const void\s*\*d_gout,\s*const float\s*\*d_tex,\s*uint32_t n,\s*uint32_t n_ch,\s*"
                     r"uint32_t tex_frames,\s*float\s*\*d_gtex,\s*void\s*\*d_gdir,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER
    assert "(additive, same version) cube-map lookup by direction over a visibility buffer" in HEADER
    assert HEADER.count("NOT BIT-REPRODUCIBLE") >= 5  # gattr, gpos twice, gtex, the cube's gtex
    # the rule's pieces are stated: the face order, the seam table's 24 rows, the choice at the vertices, subnormals
    for words in ("+X -X +Y -Y +Z -Z", "table of 24 rows", "That is a CHOICE", "SUBNORMALS are numbers"):
        assert words in HEADER, words


def test_binding_and_library_export_them():
    import srz
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("texture_cube", "texture_cube_grad"):
        assert callable(getattr(srz.FrameSet, method))
    from srz import visibility
    assert callable(visibility.texture_cube) and callable(visibility.texture_cube_grad) and callable(visibility.cube_dirs)
    assert issubclass(visibility._TextureCube, __import__("torch").autograd.Function)


def test_argument_tables_match_the_prototypes():
    import srz
    from srz import abi
    L = srz.lib()
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    kinds = {"uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t}
    for name, table in ((ENTRY_POINTS[0], abi.TEXTURE_CUBE_ARGTYPES), (ENTRY_POINTS[1], abi.TEXTURE_CUBE_GRAD_ARGTYPES)):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert want == table == list(getattr(L, name).argtypes), name
    assert len(abi.TEXTURE_CUBE_ARGTYPES) == 12 and len(abi.TEXTURE_CUBE_GRAD_ARGTYPES) == 13


def test_without_a_context_they_refuse():
    import srz
    L = srz.lib()
    assert L.srz_frameset_texture_cube(None, None, None, None, None, 4, 3, 1, None, 0, 0, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_frameset_texture_cube_grad(None, None, None, None, None, None, 4, 3, 1, None, None, 0, None) == srz.abi.SRZ_E_INVALID


def test_wrapper_argument_checks_need_no_device():
    """the torch layer refuses a malformed cube before anything reaches the library"""
    import pytest
    import torch
    from srz import visibility

    class FS:
        n_frames = 2

        def interpolate_shape(self, c):
            return (2, c, 8, 8)
    for bad in (torch.zeros(6, 4, 4, 3), torch.zeros(5, 4, 4, 3, device="meta")):
        with pytest.raises(ValueError):
            visibility._cube_dims(FS(), bad)
    with pytest.raises(ValueError):
        visibility.texture_cube_grad(FS(), None, None, None, None, want_gtex=False, want_gdir=False)
