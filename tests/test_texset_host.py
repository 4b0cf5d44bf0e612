"""not-gpu: the texture-set pass's two entry points are declared, exported and bound, their argument tables agree with the header's
prototypes, the slot struct mirrors the header's (size and offsets), the constants agree, the header states the slot rule, and
without a context the calls refuse."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
ENTRY_POINTS = ("srz_frameset_texture_set", "srz_frameset_texture_set_grad")


def test_header_states_the_slot_rule_under_the_same_abi_version():
    assert "#define SRZ_ABI_VERSION 7" in HEADER
    assert "(additive, same version) texture sets: each pixel's caller texture picked by its owner's batch, with gradients" in HEADER
    for words in ("s = b < n_batch_slot ? d_batch_slot[b] : SRZ_TEXSET_NONE",
                  "If s >= n_slots (so in particular SRZ_TEXSET_NONE) the pixel is UNSAMPLED in srz_frameset_texture's sense",
                  "every channel of out\n * is 0 (written: the pixel has an owner), guv = (0, 0), no add",
                  "No byte of the map makes a pass read or write outside its", "the host cannot validate device bytes and does not try",
                  "word\n * for word, with slot s's d_tex, tex_w, tex_h, tex_frames and mode", "Two slots MAY share one d_tex",
                  "ONE map for every frame of the set", "the value SRZ_GB_BATCH writes minus 1", "HOST array of srz_texset_slot",
                  "d_guv needs every\n * slot's d_tex", "NOT BIT-REPRODUCIBLE, within srz_frameset_texture_grad's bound",
                  "d_gtex ranges that overlap each other included", "n_batch_slot 0 or\n * above 65536"):
        assert words in HEADER, words


def test_the_constants_agree():
    from srz import abi
    assert re.search(r"#define SRZ_TEXSET_MAX\s+8u\b", CODE) and abi.TEXSET_MAX == 8
    assert re.search(r"#define SRZ_TEXSET_NONE\s+0xffu\b", CODE) and abi.TEXSET_NONE == 0xff
    assert abi.TEXSET_MAX << 28 <= 1 << 31 and abi.TEX_MAX_SIZE ** 2 == 1 << 28  # eight slots of 2^28 texels fit a 32-bit key with 0 free


def test_binding_and_library_export_them():
    import srz
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("texture_set", "texture_set_grad"):
        assert callable(getattr(srz.FrameSet, method))
    from srz import visibility
    for fn in ("texture_set", "texture_set_grad"):
        assert callable(getattr(visibility, fn))
    torch = __import__("torch")
    assert issubclass(visibility._TextureSet, torch.autograd.Function)


def test_argument_tables_match_the_prototypes():
    import srz
    from srz import abi
    L = srz.lib()
    kinds = {"uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t}
    for name, table in zip(ENTRY_POINTS, (abi.TEXTURE_SET_ARGTYPES, abi.TEXTURE_SET_GRAD_ARGTYPES)):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, CODE).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert want == table == list(getattr(L, name).argtypes), name
    names = [p.split()[-1].lstrip("*") for p in re.search(r"\bsrz_frameset_texture_set\s*\(([^)]*)\)", CODE).group(1).split(",")]
    assert names == ["ctx", "fs", "d_vis", "d_uv", "slots", "n_slots", "d_batch_slot", "n_batch_slot", "n_ch", "d_out", "out_bytes", "flags", "stream"]
    names = [p.split()[-1].lstrip("*") for p in re.search(r"\bsrz_frameset_texture_set_grad\s*\(([^)]*)\)", CODE).group(1).split(",")]
    assert names == ["ctx", "fs", "d_vis", "d_uv", "d_gout", "slots", "n_slots", "d_batch_slot", "n_batch_slot", "n_ch", "d_guv", "flags", "stream"]


def test_the_slot_struct_mirrors_the_headers():
    from srz import abi
    body = re.search(r"typedef struct srz_texset_slot \{(.*?)\} srz_texset_slot;", CODE, flags=re.S).group(1)
    fields = [name.strip().lstrip("*") for f in body.split(";") if f.strip() for name in f.split(None, 1)[1].replace("float", "").split(",")]
    assert fields == [name for name, _ in abi.SrzTexsetSlot._fields_] == ["d_tex", "d_gtex", "tex_w", "tex_h", "tex_frames", "mode"]
    S = abi.SrzTexsetSlot
    assert ctypes.sizeof(S) == 32
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16, 20, 24, 28]
    arr = abi.texset_slots_array([(16, None, 5, 7, 1, abi.TEX_WRAP), (48, 64, 33, 1, 2, abi.TEX_CLAMP)])
    assert (arr[0].d_tex, arr[0].d_gtex, arr[0].tex_w, arr[0].tex_h, arr[0].tex_frames, arr[0].mode) == (16, None, 5, 7, 1, 1)
    assert (arr[1].d_tex, arr[1].d_gtex, arr[1].tex_w, arr[1].tex_h, arr[1].tex_frames, arr[1].mode) == (48, 64, 33, 1, 2, 0)


def test_without_a_context_they_refuse():
    import srz
    L, E = srz.lib(), srz.abi.SRZ_E_INVALID
    assert L.srz_frameset_texture_set(None, None, None, None, None, 1, None, 1, 3, None, 0, 0, None) == E
    assert L.srz_frameset_texture_set_grad(None, None, None, None, None, None, 1, None, 1, 3, None, 0, None) == E


def test_wrapper_argument_checks_need_no_device():
    """the torch layer refuses malformed arguments before anything reaches the library"""
    import torch
    from srz import visibility

    class FS:
        n_frames = 2
        out_shape = (2, 4, 8, 8)

        def interpolate_shape(self, c):
            return (2, c, 8, 8)
    t, uv, vis = torch.zeros(5, 7, 3), torch.zeros(2, 2, 8, 8), torch.zeros(2, 4, 8, 8)
    for texs, batch_slot in (([], [0]), ([t], [0])):  # host tensors: uv is refused first, whatever the textures are
        with pytest.raises(ValueError, match="texture_set: uv"):
            visibility.texture_set(FS(), vis, texs, uv, batch_slot)
    with pytest.raises(ValueError, match="texture_set: batch_slot must be on the device"):  # a uint8 map is taken as it is
        visibility.texture_set(FS(), vis, [t], uv, torch.zeros(3, dtype=torch.uint8))
    # (the counts — more than abi.TEXSET_MAX textures, an empty map — are the library's to refuse: tests/test_gpu_texture_set_refusals.py)
    with pytest.raises(ValueError):
        visibility.texture_set_grad(FS(), vis, [t], uv, torch.zeros(2, 3, 8, 8), [0])
