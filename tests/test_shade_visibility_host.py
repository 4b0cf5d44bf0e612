"""not-gpu: shading a visibility buffer from the host side — both entry points in header, library and binding, their argument checks
without a device; and the premise of relighting checked on the CPU oracle: lights, ka / ks / p and the shader type change the colour
only, never the z plane or which pixels are covered."""
import ctypes
import os
import re

import numpy as np
import pytest

import scenes
from srz import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_exported_and_bound():
    import srz
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "srz.h")).read(), flags=re.S)
    assert re.search(r"int\s+srz_frameset_shade_visibility\s*\(\s*srz_ctx\s*\*\s*ctx\s*,\s*srz_frameset\s*\*\s*fs\s*,\s*const\s+void\s*\*\s*d_vis\s*,"
                     r"\s*void\s*\*\s*d_out\s*,\s*size_t\s+out_bytes\s*,\s*uint32_t\s+flags\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert re.search(r"int\s+srz_frameset_update_shading\s*\(\s*srz_ctx\s*\*\s*ctx\s*,\s*srz_frameset\s*\*\s*fs\s*,\s*const\s+srz_frame\s*\*\s*frames\s*,"
                     r"\s*int\s+n_frames\s*\)\s*;", src)
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ("srz_frameset_shade_visibility", "srz_frameset_update_shading"):
        assert hasattr(lib, name)
        assert name in srz.EXPORTS
        assert getattr(srz.lib(), name).argtypes is not None
    assert callable(srz.FrameSet.shade_visibility) and callable(srz.FrameSet.update_shading)


def test_null_ctx_or_set_is_invalid_without_a_device():
    import srz
    L = srz.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert L.srz_frameset_shade_visibility(None, None, p, p, 256, abi.FUSED_CLEAR, None) == abi.SRZ_E_INVALID
    assert L.srz_frameset_shade_visibility(None, ctypes.c_void_p(16), p, p, 256, 0, None) == abi.SRZ_E_INVALID
    assert L.srz_frameset_update_shading(None, None, None, 0) == abi.SRZ_E_INVALID


def relit(f, lights, ka, ks, p, shader):
    return abi.Frame(f.width, f.height, tuple(f.c.eye), np.asarray(lights, np.float32).reshape(-1, 2, 3),
                     [(shader, scenes.TEX_SPOT, f.tris[0])], f.c.flags, ka=ka, ks=ks, p=p)


@pytest.mark.parametrize("a", [0, 9])
def test_relighting_keeps_z_and_coverage(orc, a):
    f = scenes.config2(a, size=256)
    rc, ref, _ = orc.draw(f)
    assert rc == 0
    L = np.array([[[0.5, -0.4, 0.8], [30, 60, 90]], [[-0.2, 0.9, 0.3], [80, 80, 80]], [[0.0, 0.0, 1.2], [10, 10, 10]]], np.float32)
    for g in (relit(f, L[:2], (0.1, 0.2, 0.3), (0.5, 0.6, 0.7), 32.0, abi.SHADER_TEXTURE),
              relit(f, L[1:], (0.005, 0.005, 0.005), (0.7937, 0.7937, 0.7937), 7.5, abi.SHADER_PHONG),
              relit(f, L[:2], (0.005, 0.005, 0.005), (0.7937, 0.7937, 0.7937), 150.0, abi.SHADER_NORMAL)):
        rc, r2, _ = orc.draw(g)
        assert rc == 0
        assert np.array_equal(ref[0].view(np.uint32), r2[0].view(np.uint32))
        cov = np.isfinite(ref[0])
        assert np.array_equal(cov, np.isfinite(r2[0])) and cov.any()
        assert any(not np.array_equal(x[cov], y[cov]) for x, y in zip(ref[1:], r2[1:]))  # (the colour did change)
