"""not-gpu: the lighting pass's three entry points are declared, exported and bound, their argument tables agree with the header's
prototypes, and without a context they refuse."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_frameset_light", "srz_frameset_light_work_bytes", "srz_frameset_light_grad")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"int\s+srz_frameset_light\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*const void\s*\*d_nrm,\s*"
                     r"const void\s*\*d_pos,\s*const void\s*\*d_kd,\s*const float\s*\*d_par,\s*uint32_t n_lights,\s*uint32_t par_frames,\s*"
                     r"uint32_t p,\s*void\s*\*d_out,\s*size_t out_bytes,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert re.search(r"size_t\s+srz_frameset_light_work_bytes\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*uint32_t n_lights\)", code)
    assert re.search(r"int\s+srz_frameset_light_grad\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*const void\s*\*d_nrm,\s*"
                     r"const void\s*\*d_pos,\s*const void\s*\*d_kd,\s*const float\s*\*d_par,\s*uint32_t n_lights,\s*uint32_t par_frames,\s*"
                     r"uint32_t p,\s*const void\s*\*d_gout,\s*void\s*\*d_gnrm,\s*void\s*\*d_gpos,\s*void\s*\*d_gkd,\s*float\s*\*d_gpar,\s*"
                     r"void\s*\*d_work,\s*size_t work_bytes,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER
    assert "(additive, same version) Blinn-Phong lighting pass over a visibility buffer" in HEADER
    assert re.search(r"#define\s+SRZ_LIGHT_MAX\s+8\b", code) and re.search(r"#define\s+SRZ_LIGHT_PAR\(n_lights\)\s+\(9u \+ 6u \* \(n_lights\)\)", code)
    # the rule's pieces are stated: the deliberate differences, the fixed tree, reproducibility, the order of the shared fold
    for words in ("DELIBERATELY DIFFERENT", "NO CLAMP", "acc_c = acc_c + (kd_c * fmaf(E_c, cd, ka_c * I_c) + (ks_c * E_c) * sp)", "FIXED tree",
                  "BIT-REPRODUCIBLE for a given shard", "in frame order, from +0", "WRITTEN, not added into"):
        assert words in HEADER, words


def test_binding_and_library_export_them():
    import srz
    from srz import abi
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("light", "light_grad", "light_work_bytes"):
        assert callable(getattr(srz.FrameSet, method))
    from srz import visibility
    assert callable(visibility.light) and callable(visibility.light_grad) and callable(visibility.light_params)
    assert issubclass(visibility._Light, __import__("torch").autograd.Function)
    assert abi.LIGHT_MAX == 8 and abi.light_par(1) == 15 and abi.light_par(8) == 57


def test_argument_tables_match_the_prototypes():
    import srz
    from srz import abi
    L = srz.lib()
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    kinds = {"uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t}
    for name, table in zip(ENTRY_POINTS, (abi.LIGHT_ARGTYPES, abi.LIGHT_WORK_BYTES_ARGTYPES, abi.LIGHT_GRAD_ARGTYPES)):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert want == table == list(getattr(L, name).argtypes), name
    assert len(abi.LIGHT_ARGTYPES) == 14 and len(abi.LIGHT_GRAD_ARGTYPES) == 19
    assert L.srz_frameset_light_work_bytes.restype is ctypes.c_size_t


def test_without_a_context_they_refuse():
    import srz
    L = srz.lib()
    assert L.srz_frameset_light(None, None, None, None, None, None, None, 1, 1, 5, None, 0, 0, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_frameset_light_grad(None, None, None, None, None, None, None, 1, 1, 5, None, None, None, None, None, None, 0, 0,
                                     None) == srz.abi.SRZ_E_INVALID
    assert L.srz_frameset_light_work_bytes(None, None, 3) == 0


def test_wrapper_argument_checks_need_no_device():
    """the torch layer packs the parameter block and refuses malformed pieces before anything reaches the library"""
    import pytest
    import torch
    from srz import visibility

    class FS:
        n_frames = 2

        def interpolate_shape(self, c):
            return (2, c, 8, 8)
    lights, v = torch.arange(18.0).reshape(3, 6), torch.tensor([1.0, 2.0, 3.0])
    block = visibility.light_params(FS(), lights, v, v + 3, v + 6)
    assert tuple(block.shape) == (1, 27) and block[0, :9].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9] and block[0, 9:].tolist() == list(range(18))
    per = visibility.light_params(FS(), lights, torch.stack([v, -v]), v, v)  # per frame as soon as one piece is
    assert tuple(per.shape) == (2, 27) and per[1, :3].tolist() == [-1, -2, -3] and torch.equal(per[0, 3:], per[1, 3:])
    for bad in (dict(lights=torch.zeros(9, 6)), dict(lights=torch.zeros(3, 5)), dict(lights=torch.zeros(3, 3, 6)), dict(eye=torch.zeros(4)),
                dict(ka=torch.zeros(3, 3))):
        args = dict(lights=lights, eye=v, ka=v, ks=v)
        args.update(bad)
        with pytest.raises(ValueError):
            visibility.light_params(FS(), args["lights"], args["eye"], args["ka"], args["ks"])
    with pytest.raises(ValueError):
        visibility.light_grad(FS(), None, None, None, None, block, 5, None, False, False, False, False)
