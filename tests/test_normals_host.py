"""not-gpu: the four entry points of the vertex normals and the per-vertex attributes are declared under the same ABI version,
exported and bound, and refuse an all-null call."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
NAMES = ("srz_mesh_normals", "srz_mesh_normals_grad", "srz_sceneset_corner_attr", "srz_sceneset_corner_attr_grad")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    u, f, cf, s = r"uint32_t\s+", r"float\s*\*", r"const float\s*\*", r",\s*"
    head = r"srz_ctx\s*\*ctx" + s + r"int mesh_id" + s + cf + "d_pos" + s + u + "pos_stride" + s + u + "n_sets" + s
    assert re.search(r"int\s+srz_mesh_normals\s*\(\s*" + head + f + "d_nrm" + s + u + "nrm_stride" + s + r"void\s*\*stream\)", code)
    assert re.search(r"int\s+srz_mesh_normals_grad\s*\(\s*" + head + cf + "d_gnrm" + s + u + "gnrm_stride" + s + f + "d_work" + s + f + "d_gpos" + s
                     + r"void\s*\*stream\)", code)
    head = r"srz_ctx\s*\*ctx" + s + r"srz_frameset\s*\*fs" + s + r"int mesh_id" + s
    assert re.search(r"int\s+srz_sceneset_corner_attr\s*\(\s*" + head + cf + "d_attr" + s + u + "n_ch" + s + u + "attr_frames" + s + f + "d_out" + s
                     + u + "pos_tris" + s + r"void\s*\*stream\)", code)
    assert re.search(r"int\s+srz_sceneset_corner_attr_grad\s*\(\s*" + head + cf + "d_gout" + s + u + "n_ch" + s + f + "d_gattr" + s + u + "pos_tris" + s
                     + r"void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER
    assert "(additive, same version) vertex normals and per-vertex attributes on the device, with gradients" in HEADER
    rule = HEADER[HEADER.index("VERTEX NORMALS of a slot's faces"):HEADER.index("int srz_mesh_normals(")]
    assert "NOT THE LOADER'S RULE" in rule and "no atomics" in rule and "len2 <= FLT_MAX" in rule


def test_binding_and_library_export_them():
    import srz
    from srz import visibility
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in NAMES:
        assert name in srz.EXPORTS and hasattr(lib, name), name
    for cls, fn in ((srz.Context, "mesh_normals"), (srz.Context, "mesh_normals_grad"), (srz.FrameSet, "corner_attr"), (srz.FrameSet, "corner_attr_grad")):
        assert callable(getattr(cls, fn))
    for fn in ("mesh_normals", "refresh_normals", "corner_attr"):
        assert callable(getattr(visibility, fn))
    L = srz.lib()
    assert L.srz_abi_version() == 7
    assert L.srz_mesh_normals(None, 0, None, 0, 0, None, 0, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_mesh_normals_grad(None, 0, None, 0, 0, None, 0, None, None, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_sceneset_corner_attr(None, None, 0, None, 0, 0, None, 0, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_sceneset_corner_attr_grad(None, None, 0, None, 0, None, 0, None) == srz.abi.SRZ_E_INVALID
