"""not-gpu: the mipmapped cube lookup's seven entry points are declared, exported and bound, their argument tables agree with the
header's prototypes, the two pure host functions are the 2D ones on the cube viewed as 6 * tex_frames textures of n x n, and without
a context the others refuse."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_cube_mip_levels", "srz_cube_mip_bytes", "srz_cube_mip_build", "srz_cube_mip_fold", "srz_frameset_texture_cube_mip",
                "srz_frameset_texture_cube_mip_grad", "srz_frameset_cube_level")
SIZES = (1, 2, 6, 8, 96, 16384, 16385)


def test_header_states_the_rules_under_the_same_abi_version():
    assert "#define SRZ_ABI_VERSION 7" in HEADER
    assert "(additive, same version) mipmapped cube-map lookup by direction and level" in HEADER
    assert "a cube has no mip pyramid here" not in HEADER and "MIPMAPPED CUBE-MAP LOOKUP" in HEADER
    for words in ("Level l + 1 exists iff n_l > 1 and n_l is even", "if (!(lam > 0.0f))", "else if (lam >= (float)(L - 1))",
                  "out = c_l0 when f == 0 (level l0 + 1 is not read), else out = fmaf(f, c_(l0+1) - c_l0, c_l0)",
                  "lam >= 0.0f && lam < (float)(L - 1)", "RIGHT-HAND derivative", "sx = (dsc - s * dma) * inv", "6 * tex_frames > 65536"):
        assert words in HEADER, words


def test_binding_and_library_export_them():
    import srz
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("texture_cube_mip", "texture_cube_mip_grad", "cube_level"):
        assert callable(getattr(srz.FrameSet, method))
    for method in ("cube_mip_build", "cube_mip_fold"):
        assert callable(getattr(srz.Context, method))
    from srz import visibility
    for fn in ("cube_mip_build", "cube_mip_views", "cube_level", "texture_cube_mip_grad", "texture_cube_mip"):
        assert callable(getattr(visibility, fn))
    assert issubclass(visibility._TextureCubeMip, __import__("torch").autograd.Function)


def test_argument_tables_match_the_prototypes():
    import srz
    from srz import abi
    L = srz.lib()
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    kinds = {"uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t}
    tables = (abi.CUBE_MIP_LEVELS_ARGTYPES, abi.CUBE_MIP_BYTES_ARGTYPES, abi.CUBE_MIP_BUILD_ARGTYPES, abi.CUBE_MIP_FOLD_ARGTYPES,
              abi.TEXTURE_CUBE_MIP_ARGTYPES, abi.TEXTURE_CUBE_MIP_GRAD_ARGTYPES, abi.CUBE_LEVEL_ARGTYPES)
    for name, table in zip(ENTRY_POINTS, tables):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert want == table == list(getattr(L, name).argtypes), name
    assert L.srz_cube_mip_levels.restype is ctypes.c_uint32 and L.srz_cube_mip_bytes.restype is ctypes.c_size_t


@pytest.mark.parametrize("n", SIZES)
def test_levels_and_bytes_are_the_2d_functions_on_the_reshaped_cube(n):
    import srz
    import cubemipref
    most = srz.cube_mip_levels(n)
    assert most == srz.mip_levels(n, n)
    assert most == (0 if n > srz.abi.TEX_MAX_SIZE else cubemipref.n_levels(n))
    for L in range(0, most + 2):
        for n_ch, tf in ((1, 1), (5, 3), (srz.abi.ATTR_MAX_CH, 2), (0, 1), (srz.abi.ATTR_MAX_CH + 1, 1), (3, 0)):
            got = srz.cube_mip_bytes(n, n_ch, tf, L)
            assert got == srz.mip_bytes(n, n, n_ch, 6 * tf, L), (n, L, n_ch, tf)
            if 2 <= L <= most and 1 <= n_ch <= srz.abi.ATTR_MAX_CH and tf >= 1:
                assert got == 4 * n_ch * tf * sum(6 * (n >> l) ** 2 for l in range(1, L))
            else:
                assert got == 0


def test_levels_by_hand_and_the_frame_limit():
    import srz
    assert [srz.cube_mip_levels(n) for n in (1, 2, 5, 6, 8, 64, 96, 16384, 16385, 0)] == [1, 2, 1, 2, 4, 7, 6, 15, 0, 0]
    # 6 * tex_frames <= 65536: 10922 frames are the most
    assert srz.cube_mip_bytes(2, 1, 10922, 2) == 4 * 6 * 10922 and srz.cube_mip_bytes(2, 1, 10923, 2) == 0
    assert srz.cube_mip_bytes(2, 1, 2 ** 32 - 1, 2) == 0  # (no wrap of 6 * tex_frames)
    # the concatenated pyramid of one frame stays below 2^31 texels at the largest cube: what the backward's table keys need
    assert sum(6 * (16384 >> l) ** 2 for l in range(15)) < 2 ** 31


def test_without_a_context_they_refuse():
    import srz
    L, E = srz.lib(), srz.abi.SRZ_E_INVALID
    assert L.srz_cube_mip_build(None, None, 4, 3, 1, 2, None, 0, None) == E
    assert L.srz_cube_mip_fold(None, None, 0, 4, 3, 1, 2, None, None) == E
    assert L.srz_frameset_texture_cube_mip(None, None, None, None, None, None, 4, 3, 1, None, 2, None, 0, 0, None) == E
    assert L.srz_frameset_texture_cube_mip_grad(None, None, None, None, None, None, None, None, 4, 3, 1, 2, None, None, None, None, 0, None) == E
    assert L.srz_frameset_cube_level(None, None, None, None, None, 4, 2, None, 0, 0, None) == E


def test_wrapper_argument_checks_need_no_device():
    """the torch layer refuses malformed arguments before anything reaches the library"""
    import torch
    from srz import visibility

    class FS:
        n_frames = 2

        def interpolate_shape(self, c):
            return (2, c, 8, 8)
    with pytest.raises(ValueError):
        visibility._cube_mip_dims((6, 8, 8, 3), 5)  # 8: 4 levels
    with pytest.raises(ValueError):
        visibility._cube_mip_dims((6, 8, 4, 3), None)
    assert visibility._cube_mip_dims((2, 6, 8, 8, 3), None) == (2, 8, 3, 4)
    with pytest.raises(ValueError):
        visibility._lam_arg(FS(), torch.zeros(2, 1, 8, 8), 2)  # not on the device
    assert visibility._lam_arg(FS(), None, 1) is None
    with pytest.raises(ValueError):
        visibility.texture_cube_mip_grad(FS(), None, None, None, None, None, want_gtex=False, want_gdir=False, want_glam=False)
    flat = torch.arange(6 * (16 + 4 + 1) * 3, dtype=torch.float32)
    v = visibility.cube_mip_views(flat, (6, 8, 8, 3))
    assert [tuple(x.shape) for x in v] == [(6, 4, 4, 3), (6, 2, 2, 3), (6, 1, 1, 3)] and v[1].ravel()[0] == 6 * 16 * 3
