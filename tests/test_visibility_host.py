"""not-gpu: the visibility buffer's host side — the entry point in header, library and binding; srz.visibility's decode and
batch_of; and the test reference of tests/test_gpu_visibility.py checked against the CPU oracle before any GPU runs it."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import scenes
import visref
from srz import abi
from support import frame, soup

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_exported_and_bound():
    import srz
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "srz.h")).read(), flags=re.S)
    assert re.search(r"int\s+srz_frameset_render_visibility\s*\(\s*srz_ctx\s*\*\s*ctx\s*,\s*srz_frameset\s*\*\s*fs\s*,\s*void\s*\*\s*d_out\s*,"
                     r"\s*size_t\s+out_bytes\s*,\s*uint32_t\s+flags\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert hasattr(ctypes.CDLL(srz.LIB_PATH), "srz_frameset_render_visibility")
    assert "srz_frameset_render_visibility" in srz.EXPORTS
    assert srz.lib().srz_frameset_render_visibility.argtypes is not None
    assert callable(srz.FrameSet.render_visibility)


def test_null_ctx_or_set_is_invalid_without_a_device():
    import srz
    L = srz.lib()
    buf = (ctypes.c_float * 64)()
    assert L.srz_frameset_render_visibility(None, None, ctypes.addressof(buf), 256, abi.FUSED_CLEAR, None) == abi.SRZ_E_INVALID
    assert L.srz_frameset_render_visibility(None, ctypes.c_void_p(16), ctypes.addressof(buf), 256, 0, None) == abi.SRZ_E_INVALID


def _buffer(z, ids, al, be):
    return torch.stack([torch.as_tensor(np.asarray(z, np.float32)), torch.as_tensor(np.asarray(ids, np.uint32).view(np.float32)),
                        torch.as_tensor(np.asarray(al, np.float32)), torch.as_tensor(np.asarray(be, np.float32))])[None]


def test_decode_on_a_hand_built_buffer():
    from srz import visibility
    x, y = np.uint32([1053831802, 1055500889]).view(np.float32)  # a pair on which the two gamma rules differ
    a = np.float32([[0.25, x], [0.0, 0.3]])
    b = np.float32([[0.5, y], [0.0, 0.3]])
    ids = [[1, 0x80000000 | 6], [0, 0x7fffffff]]
    z = [[0.5, 2.0], [np.inf, -1.0]]
    v = visibility.decode(_buffer(z, ids, a, b))
    assert v.tri.dtype == torch.int64 and v.tri[0].tolist() == [[0, 5], [-1, 0x7ffffffe]]
    assert v.s_class[0].tolist() == [[False, True], [False, False]]
    assert torch.equal(v.z[0], torch.tensor(z, dtype=torch.float32))
    g = v.gamma[0].numpy()
    # V: 1 - (a + b); S: (1 - a) - b, each a float32 rounding; nobody: 0
    assert g[0, 0].view(np.uint32) == (np.float32(1) - (a[0, 0] + b[0, 0])).view(np.uint32)
    assert g[0, 1].view(np.uint32) == ((np.float32(1) - a[0, 1]) - b[0, 1]).view(np.uint32)
    assert g[1, 0] == 0 and g[1, 1].view(np.uint32) == (np.float32(1) - (a[1, 1] + b[1, 1])).view(np.uint32)
    assert g[0, 1] != np.float32(1) - (x + y)  # (the class decides)
    with pytest.raises(ValueError):
        visibility.decode(torch.zeros(3, 2, 2))


def test_batch_of():
    from srz import visibility
    t = np.zeros(1, abi.TRI_DTYPE)
    f = frame([(abi.SHADER_NORMAL, -1, np.repeat(t, 3)), (abi.SHADER_NORMAL, -1, t[:0]), (abi.SHADER_PHONG, -1, np.repeat(t, 2))])
    got = visibility.batch_of(f, torch.tensor([[-1, 0, 2], [3, 4, 1]]))
    assert got.tolist() == [[-1, 0, 0], [2, 2, 0]]
    assert visibility.batch_of([5, 1], torch.tensor([4, 5, -1])).tolist() == [0, 1, -1]  # a sceneset's draws: face counts
    with pytest.raises(IndexError):
        visibility.batch_of(f, torch.tensor([5]))


def check_reference(tmp_path, orc, f, planes_init=None):
    """decoded owners + the helper's alpha / beta reproduce the oracle's z plane bit for bit on every pixel it changed"""
    ref = visref.Reference(tmp_path, f)
    words, out, amb, zz, own = ref.expected(orc, planes_init)
    assert amb == 0, f"{amb} pixels decode ambiguously"
    assert own.any()
    zo = np.ascontiguousarray(out[0], np.float32).view(np.uint32)
    bad = own & (zz.view(np.uint32) != zo)
    assert not bad.any(), f"per-class z differs from the oracle at {int(bad.sum())} pixels, first {np.argwhere(bad)[:4].tolist()}"
    return ref, words


@pytest.mark.parametrize("seed", range(8))
def test_reference_reproduces_oracle_z_on_soups(tmp_path, orc, seed):
    zs = np.array([1.0, 2.0, 2.0, 3.0, 0.5], np.float32)  # repeated depths: ties (V first wins, S last wins)
    t = soup(seed, 120, 96, 80, zs, big=seed % 4 == 1)
    for flags in (abi.FUSED_CLEAR, abi.FUSED_CLEAR | abi.UNIFIED):
        check_reference(tmp_path, orc, frame(t, 96, 80, flags=flags))


def test_reference_in_accumulate_mode(tmp_path, orc):
    rng = np.random.default_rng(7)
    t = soup(3, 100, 96, 80, np.array([1.0, 2.0, 3.0], np.float32))
    init = (rng.uniform(0.5, 4.0, (80, 96)).astype(np.float32),) + tuple(rng.uniform(0, 255, (80, 96)).astype(np.float32) for _ in range(3))
    ref, words = check_reference(tmp_path, orc, frame(t, 96, 80, flags=0), init)
    keep = words[1] == np.ascontiguousarray(init[1]).view(np.uint32)
    assert keep.any() and not keep.all()


@pytest.mark.parametrize("angle", [0, 7])
def test_reference_on_spot(tmp_path, orc, angle):
    check_reference(tmp_path, orc, scenes.config2(angle, size=512, shader=abi.SHADER_NORMAL))


def test_reference_on_config3_and_config5(tmp_path, orc):
    """the two-mesh 1080p frame and the eight stacked spots (heavy overdraw, ~47 k triangles) decode without ambiguity"""
    check_reference(tmp_path, orc, scenes.config3(2))
    check_reference(tmp_path, orc, scenes.config5(3, size=1024))
