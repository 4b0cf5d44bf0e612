"""not-gpu: the two entry points of the mesh Laplacian are declared under the same ABI version with the rule's sentences beside them,
exported and bound, their constants agree between the header and the binding, and they refuse a call without a context."""
import ctypes
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
NAMES = ("srz_mesh_laplacian", "srz_mesh_laplacian_grad")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    u, f, cf, s = r"uint32_t\s+", r"float\s*\*", r"const float\s*\*", r",\s*"
    head = r"srz_ctx\s*\*\s*(?:ctx)?" + s + r"int mesh_id" + s
    tail = u + "n_ch" + s + u + "n_sets" + s + "int kind" + s + cf + "d_wpos" + s + u + "wpos_stride" + s
    assert re.search(r"int\s+srz_mesh_laplacian\s*\(\s*" + head + cf + "d_x" + s + u + "x_stride" + s + tail + f + "d_out" + s + u + "out_stride" + s
                     + r"void\s*\*stream\)", code)
    assert re.search(r"int\s+srz_mesh_laplacian_grad\s*\(\s*" + head + cf + "d_gout" + s + u + "gout_stride" + s + tail + f + "d_gx" + s + u
                     + "gx_stride" + s + r"void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER
    assert "(additive, same version) the mesh Laplacian over a slot's connectivity: umbrella, graph and cotangent, with gradients" in HEADER


def test_the_constants_agree():
    from srz import abi
    for name, value in (("UMBRELLA", 0), ("GRAPH", 1), ("COTAN", 2)):
        assert re.search(rf"#define\s+SRZ_LAP_{name}\s+{value}\b", HEADER) and getattr(abi, "LAP_" + name) == value
    assert abi.LAP_MAX_CH == 64 and len(abi.MESH_LAPLACIAN_ARGTYPES) == 12


def test_the_header_states_the_rule():
    flow = lambda text: re.sub(r"\s*\n \*\s*", " ", text)  # noqa: E731  (a comment's line breaks are not the sentence's)
    rule = flow(HEADER[HEADER.index("THE MESH LAPLACIAN over a slot's connectivity"):HEADER.index("int srz_mesh_laplacian(")])
    for sentence in ("in float32, nothing fused", "S = S + (x[a] + x[b])", "out[v] = x[v] - S / n_v", "otherwise out[v] = +0",
                     "out[v] = n_v * x[v] - S", "ok = d2 > 0 && d2 <= FLT_MAX", "ia = 1.0f / sqrtf(d2)",
                     "acc = acc + (cot_b * (x[v] - x[a]) + cot_a * (x[v] - x[b]))", "out[v] = 0.5f * acc", "SKIPPED, never multiplied by zero",
                     "symmetric in the bits", "no atomics", "DETERMINISTIC, bit for bit", "NO in-place record form",
                     "to the vertex itself and to its neighbours only", "n_ch is 1 .. 64", "n_ch must be 3 and n_sets 1",
                     "No input value makes the pass read or write outside its buffers"):
        assert sentence in rule, sentence
    back = flow(HEADER[HEADER.index("THE BACKWARD of srz_mesh_laplacian"):HEADER.index("int srz_mesh_laplacian_grad(")])
    for sentence in ("THE EXACT TRANSPOSE", "neither x nor a workspace", "IS the forward rule applied to gout", "the same kernel, the same",
                     "T = T + (gout[a] / n_a + gout[b] / n_b)", "gx[v] = (n_v > 0 ? gout[v] : +0) - T", "EVERY element", "no atomics",
                     "DETERMINISTIC, bit for bit", "a null d_gout"):
        assert sentence in back, sentence


def test_binding_and_library_export_them():
    import srz
    from srz import visibility
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in NAMES:
        assert name in srz.EXPORTS and hasattr(lib, name), name
    for fn in ("mesh_laplacian", "mesh_laplacian_grad"):
        assert callable(getattr(srz.Context, fn))
    for fn in ("mesh_laplacian", "mesh_solve", "_cg"):
        assert callable(getattr(visibility, fn))
    assert list(inspect.signature(visibility.mesh_laplacian).parameters) == ["ctx", "slot", "x", "kind", "wpos", "stream"]
    assert list(inspect.signature(visibility.mesh_solve).parameters) == ["ctx", "slot", "b", "lam", "kind", "wpos", "iters", "tol", "stream"]
    assert inspect.signature(visibility.mesh_laplacian).parameters["kind"].default == "umbrella"
    assert inspect.signature(visibility.mesh_solve).parameters["kind"].default == "graph"
    assert list(inspect.signature(visibility._cg).parameters) == ["apply", "b", "iters", "tol"]
    for fn in (visibility.mesh_laplacian, visibility.mesh_solve):  # the two uses, in both docstrings
        assert "reg   = (mesh_laplacian(ctx, slot, verts) ** 2).sum()" in fn.__doc__
        assert "verts = mesh_solve(ctx, slot, u, 10.0); ... loss(verts).backward()" in fn.__doc__
    L = srz.lib()
    assert L.srz_abi_version() == 7
    assert L.srz_mesh_laplacian.argtypes == srz.abi.MESH_LAPLACIAN_ARGTYPES == L.srz_mesh_laplacian_grad.argtypes
    # without a context: SRZ_E_INVALID whatever else is passed, nothing dereferenced
    assert L.srz_mesh_laplacian(None, 0, None, 0, 0, 0, 0, None, 0, None, 0, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_mesh_laplacian_grad(None, 0, None, 0, 0, 0, 0, None, 0, None, 0, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_mesh_laplacian(None, 7, 4096, 3, 3, 1, 2, 4096, 3, 8192, 3, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_mesh_laplacian_grad(None, 7, 4096, 3, 3, 1, 0, None, 0, 8192, 3, None) == srz.abi.SRZ_E_INVALID
