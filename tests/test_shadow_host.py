"""not-gpu: the shadow lookup's two entry points are declared, exported and bound, their argument tables agree with the header's
prototypes, without a context they refuse, and the torch wrappers' own argument checks run without a device."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_frameset_shadow", "srz_frameset_shadow_grad")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"int\s+srz_frameset_shadow\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*const void\s*\*d_sc,\s*"
                     r"const float\s*\*d_map,\s*uint32_t map_w,\s*uint32_t map_h,\s*uint32_t map_frames,\s*float bias,\s*float width,\s*"
                     r"void\s*\*d_out,\s*size_t out_bytes,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert re.search(r"int\s+srz_frameset_shadow_grad\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*const void\s*\*d_sc,\s*"
                     r"const void\s*\*d_gout,\s*const float\s*\*d_map,\s*uint32_t map_w,\s*uint32_t map_h,\s*uint32_t map_frames,\s*float bias,\s*"
                     r"float width,\s*float\s*\*d_gmap,\s*void\s*\*d_gsc,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER
    assert "(additive, same version) shadow-map lookup over a visibility buffer" in HEADER
    # the rule's pieces are stated: the texel grid, the clamp, outside corners, both tests, the ramp's gradient, gmap's bound
    for words in ("CENTRES ON THE INTEGERS", "fx = fminf(fmaxf(sx, -1.0f), (float)W)", "OUTSIDE the map", "v = e >= 0.0f ? 1.0f : 0.0f",
                  "q = e / width + 0.5f", "d_rc = moving_rc ? (w_rc * g) / width : 0.0f", "gsd = -(((d00 + d01) + d10) + d11)",
                  "d_gmap is NOT BIT-REPRODUCIBLE"):
        assert words in HEADER, words


def test_binding_and_library_export_them():
    import srz
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("shadow", "shadow_grad"):
        assert callable(getattr(srz.FrameSet, method))
    from srz import visibility
    assert callable(visibility.shadow) and callable(visibility.shadow_grad)
    assert issubclass(visibility._Shadow, __import__("torch").autograd.Function)
    for words in ("depth(fs_l, vis_l, pos_l)", "interpolate(fs_cam, vis_cam, pos_l.view(n, T, 3, 3))", "its own light() call", "interpolate_persp"):
        assert words in visibility.shadow.__doc__, words


def test_argument_tables_match_the_prototypes():
    import srz
    from srz import abi
    L = srz.lib()
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    kinds = {"uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    for name, table in ((ENTRY_POINTS[0], abi.SHADOW_ARGTYPES), (ENTRY_POINTS[1], abi.SHADOW_GRAD_ARGTYPES)):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert want == table == list(getattr(L, name).argtypes), name
    assert len(abi.SHADOW_ARGTYPES) == 14 and len(abi.SHADOW_GRAD_ARGTYPES) == 15


def test_without_a_context_they_refuse():
    import srz
    L = srz.lib()
    assert L.srz_frameset_shadow(None, None, None, None, None, 4, 4, 1, 0.0, 0.0, None, 0, 0, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_frameset_shadow_grad(None, None, None, None, None, None, 4, 4, 1, 0.0, 1.0, None, None, 0, None) == srz.abi.SRZ_E_INVALID


class FS:
    """what the wrappers ask of a set before anything reaches the library"""
    n_frames = 2

    def interpolate_shape(self, c):
        return (2, c, 8, 8)


def meta(*shape, dtype=None):
    import torch
    return torch.zeros(shape, dtype=dtype or torch.float32, device="meta")


def test_map_checks_need_no_device():
    """each refusal is the one meant: a meta tensor has the shape and dtype asked about, and is refused for being off the device last"""
    import torch
    from srz import visibility as V
    with pytest.raises(ValueError, match="float32 tensor"):  # wrong dtype
        V._map_dims(FS(), meta(4, 4, dtype=torch.float64))
    for shape in ((4,), (2, 3, 4, 4), (2, 1, 1, 4, 4)):  # wrong shape
        with pytest.raises(ValueError, match="float32 tensor"):
            V._map_dims(FS(), meta(*shape))
    for shape in ((3, 4, 4), (5, 1, 4, 4)):  # wrong frame count
        with pytest.raises(ValueError, match="frames, the set 2"):
            V._map_dims(FS(), meta(*shape))
    with pytest.raises(ValueError, match="texels"):
        V._map_dims(FS(), meta(0, 4))
    with pytest.raises(ValueError, match="texels"):
        V._map_dims(FS(), meta(2, 4, V.abi.TEX_MAX_SIZE + 1))
    for shape in ((4, 6), (2, 4, 6), (2, 1, 4, 6)):  # well-formed, and only then: not on the device
        with pytest.raises(ValueError, match="on the device"):
            V._map_dims(FS(), meta(*shape))


def test_coordinate_and_ramp_checks_need_no_device():
    import torch
    from srz import visibility as V
    with pytest.raises(ValueError, match="sc must be a float32 tensor"):
        V._sc_arg(FS(), meta(2, 3, 8, 8, dtype=torch.float16))
    for shape in ((2, 2, 8, 8), (3, 3, 8, 8), (2, 3, 8, 4), (3, 8, 8)):
        with pytest.raises(ValueError, match="sc must be a float32 tensor"):
            V._sc_arg(FS(), meta(*shape))
    with pytest.raises(ValueError, match="on the device"):
        V._sc_arg(FS(), meta(2, 3, 8, 8))
    for bias, width in ((0.0, -1.0), (0.0, -1e-30), (0.0, float("nan")), (0.0, float("inf")), (float("nan"), 1.0), (float("-inf"), 1.0)):
        with pytest.raises(ValueError, match="finite"):
            V._ramp_args(bias, width)
    assert V._ramp_args(0, 0) == (0.0, 0.0) and V._ramp_args(-0.5, 2) == (-0.5, 2.0)


def test_the_calls_refuse_before_anything_reaches_the_library():
    """shadow and shadow_grad themselves, handed what a caller might: ValueError, not a crash in ctypes or an error from the device"""
    from srz import visibility as V
    fs, good_map, good_sc = FS(), meta(2, 4, 4), meta(2, 3, 8, 8)
    with pytest.raises(ValueError, match="neither gmap nor gsc"):
        V.shadow_grad(fs, None, good_map, good_sc, meta(2, 1, 8, 8), 0.0, 1.0, want_gmap=False, want_gsc=False)
    for width in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="finite"):
            V.shadow(fs, None, good_map, good_sc, 0.0, width)
        with pytest.raises(ValueError, match="finite"):
            V.shadow_grad(fs, None, good_map, good_sc, meta(2, 1, 8, 8), 0.0, width)
    with pytest.raises(ValueError, match="frames, the set 2"):
        V.shadow(fs, None, meta(3, 4, 4), good_sc, 0.0, 1.0)
    with pytest.raises(ValueError, match="frames, the set 2"):
        V.shadow_grad(fs, None, meta(3, 4, 4), good_sc, meta(2, 1, 8, 8), 0.0, 1.0)
