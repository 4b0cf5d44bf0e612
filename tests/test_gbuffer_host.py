"""not-gpu: the G-buffer's two entry points are declared, exported and bound, and the Python side agrees with the header on the
group constants and on the order of the planes."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_frameset_gbuffer_bytes", "srz_frameset_gbuffer")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"size_t\s+srz_frameset_gbuffer_bytes\s*\(\s*const srz_ctx\s*\*\w*,\s*const srz_frameset\s*\*\w*,\s*uint32_t \w+\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER and "(additive, same version) the G-buffer" in HEADER


def test_binding_and_library_export_them():
    import srz
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("gbuffer", "gbuffer_bytes", "gbuffer_shape"):
        assert callable(getattr(srz.FrameSet, method))


def test_group_constants_equal_the_headers():
    from srz import abi
    for name in ("NORMAL", "UV", "BATCH", "ALBEDO"):
        m = re.search(r"#define SRZ_GB_%s\s+(\d+)u" % name, HEADER)
        assert m and int(m.group(1)) == getattr(abi, "GB_" + name), name
    assert (abi.GB_NORMAL, abi.GB_UV, abi.GB_BATCH, abi.GB_ALBEDO) == (1, 2, 4, 8)


def test_plane_order_of_all_15_masks():
    from srz import abi
    from srz.visibility import gbuffer_planes
    groups = ((abi.GB_NORMAL, ["nx", "ny", "nz"]), (abi.GB_UV, ["u", "v"]), (abi.GB_BATCH, ["batch"]),
              (abi.GB_ALBEDO, ["albedo0", "albedo1", "albedo2"]))
    for what in range(1, 16):
        want = [n for bit, names in groups if what & bit for n in names]
        assert list(gbuffer_planes(what)) == want, what
    assert list(gbuffer_planes(15)) == ["nx", "ny", "nz", "u", "v", "batch", "albedo0", "albedo1", "albedo2"]
    for bad in (0, 16, 31):
        with pytest.raises(ValueError):
            gbuffer_planes(bad)


def test_decode_returns_views():
    import torch
    from srz import abi
    from srz.visibility import gbuffer_decode
    buf = torch.arange(2 * 9 * 3 * 4, dtype=torch.int32).reshape(2, 9, 3, 4)
    buf[:, 5] = torch.tensor([0, 1, 2, 7])
    g = gbuffer_decode(buf, abi.GB_ALL)
    assert g["normal"].shape == (2, 3, 3, 4) and g["uv"].shape == (2, 2, 3, 4) and g["albedo"].shape == (2, 3, 3, 4)
    assert g["batch"].dtype == torch.int32 and g["batch"][0, 0].tolist() == [-1, 0, 1, 6]
    for key, first in (("normal", 0), ("uv", 3), ("albedo", 6)):
        assert g[key].dtype == torch.float32 and g[key].data_ptr() == buf[:, first:].data_ptr()  # a view: no copy
    part = gbuffer_decode(buf[:, :3], abi.GB_UV | abi.GB_BATCH)
    assert set(part) == {"uv", "batch"} and part["uv"].data_ptr() == buf.data_ptr()
    with pytest.raises(ValueError):
        gbuffer_decode(buf, abi.GB_UV)
