"""not-gpu: the mip entry points are declared, exported and bound with the argument counts of the header; the Python side agrees with
the header on the level cap; the two pure host functions — srz_texture_mip_levels and srz_texture_mip_bytes — return what
include/srz.h says, with no GPU involved."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
# entry point -> its argument count
ENTRY_POINTS = {"srz_texture_mip_levels": 2, "srz_texture_mip_bytes": 5, "srz_texture_mip_build": 10, "srz_texture_mip_fold": 10,
                "srz_frameset_interpolate_deriv": 11, "srz_frameset_texture_mip": 17, "srz_frameset_texture_mip_grad": 19}
LEVELS = {(1024, 1024): 11, (16384, 16384): 15, (100, 70): 2, (96, 64): 6, (32, 8): 6, (5, 7): 1, (1, 1): 1, (0, 4): 0, (16385, 2): 0}


def py_sizes(w, h):
    """the chain of level sizes by the header's rule, in Python"""
    out = [(w, h)]
    while (w > 1 or h > 1) and (w % 2 == 0 or w == 1) and (h % 2 == 0 or h == 1):
        w, h = max(1, w // 2), max(1, h // 2)
        out.append((w, h))
    return out


def test_header_declares_the_entry_points_under_the_same_abi_version():
    for name, n_args in ENTRY_POINTS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, CODE)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
    assert "#define SRZ_ABI_VERSION 7" in HEADER and "(additive, same version) mipmapped texture sampling over a visibility buffer" in HEADER
    assert re.search(r"#define SRZ_TEX_MAX_LEVELS\s+15u", HEADER)
    assert HEADER.count("NOT BIT-REPRODUCIBLE") >= 5  # gattr, gpos twice, gtex, gtex and gmip of the mip pass
    assert "LAMBDA IS HELD\n * FIXED" in HEADER or "LAMBDA IS HELD FIXED" in HEADER
    assert "PIECEWISE-LINEAR" in HEADER


def test_binding_and_library_export_them():
    import srz
    from srz import abi, visibility
    lib = ctypes.CDLL(srz.LIB_PATH)
    L = srz.lib()
    for name, n_args in ENTRY_POINTS.items():
        assert name in srz.EXPORTS and hasattr(lib, name)
        assert len(getattr(L, name).argtypes) == n_args, name
    for method in ("interpolate_deriv", "texture_mip", "texture_mip_grad"):
        assert callable(getattr(srz.FrameSet, method))
    for method in ("mip_build", "mip_fold"):
        assert callable(getattr(srz.Context, method))
    for fn in ("interpolate_deriv", "mip_build", "mip_views", "texture_mip_grad", "texture_mip"):
        assert callable(getattr(visibility, fn))
    assert callable(srz.mip_levels) and callable(srz.mip_bytes)
    assert abi.TEX_MAX_LEVELS == 15 == srz.mip_levels(abi.TEX_MAX_SIZE, abi.TEX_MAX_SIZE)


def test_null_arguments_are_invalid():
    import srz
    L, E = srz.lib(), srz.abi.SRZ_E_INVALID
    assert L.srz_texture_mip_build(None, None, 4, 4, 3, 1, 2, None, 0, None) == E
    assert L.srz_texture_mip_fold(None, None, 0, 4, 4, 3, 1, 2, None, None) == E
    assert L.srz_frameset_interpolate_deriv(None, None, None, None, 2, 1, 1, None, 0, 0, None) == E
    assert L.srz_frameset_texture_mip(None, None, None, None, None, None, 4, 4, 3, 1, 0, None, 2, None, 0, 0, None) == E
    assert L.srz_frameset_texture_mip_grad(None, None, None, None, None, None, None, None, 4, 4, 3, 1, 0, 2, None, None, None, 0, None) == E


def test_mip_levels():
    import srz
    for (w, h), n in LEVELS.items():
        assert srz.mip_levels(w, h) == n, (w, h)
        if n:
            assert len(py_sizes(w, h)) == n
    assert py_sizes(96, 64)[-1] == (3, 2) and py_sizes(32, 8)[3:] == [(4, 1), (2, 1), (1, 1)]
    for (w, h) in ((64, 64), (2, 2), (1, 16384), (16384, 1), (6, 4), (12, 1), (7, 8), (8, 7), (16384, 16382)):
        assert srz.mip_levels(w, h) == len(py_sizes(w, h)), (w, h)
    assert srz.mip_levels(4, 0) == 0 and srz.mip_levels(2, 16385) == 0


@pytest.mark.parametrize("w,h", [(1024, 1024), (100, 70), (96, 64), (32, 8), (5, 7), (1, 1), (64, 64), (16384, 16384), (1, 4096)])
def test_mip_bytes_is_the_sum_over_the_levels(w, h):
    import srz
    from srz import abi
    chain = py_sizes(w, h)
    for n_ch, frames in ((1, 1), (3, 1), (5, 2), (64, 9)):
        for n_levels in range(1, len(chain) + 1):
            want = sum(frames * hl * wl * n_ch * 4 for (wl, hl) in chain[1:n_levels])
            assert srz.mip_bytes(w, h, n_ch, frames, n_levels) == want, (n_ch, frames, n_levels)
        assert srz.mip_bytes(w, h, n_ch, frames, 1) == 0
        assert srz.mip_bytes(w, h, n_ch, frames, 0) == 0 and srz.mip_bytes(w, h, n_ch, frames, len(chain) + 1) == 0
    assert srz.mip_bytes(w, h, 0, 1, len(chain)) == 0 and srz.mip_bytes(w, h, abi.ATTR_MAX_CH + 1, 1, len(chain)) == 0
    assert srz.mip_bytes(w, h, 3, 0, len(chain)) == 0 and srz.mip_bytes(0, h, 3, 1, 2) == 0 and srz.mip_bytes(w, abi.TEX_MAX_SIZE + 1, 3, 1, 2) == 0
