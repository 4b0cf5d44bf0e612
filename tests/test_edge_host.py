"""not-gpu: the two entry points of the mesh edge terms are declared under the same ABI version with the rules' sentences beside them,
exported and bound, their constants agree between the header and the binding, the torch layer has the five functions without a
refusal of its own, and the entry points refuse a call without a context."""
import ctypes
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
NAMES = ("srz_mesh_edges", "srz_mesh_edges_grad")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    u, f, cf, s = r"uint32_t\s+", r"float\s*\*", r"const float\s*\*", r",\s*"
    head = r"srz_ctx\s*\*\s*(?:ctx)?" + s + r"int mesh_id" + s + cf + "d_pos" + s + u + "pos_stride" + s + u + "n_sets" + s + "int kind" + s
    assert re.search(r"int\s+srz_mesh_edges\s*\(\s*" + head + f + "d_out" + s + u + "out_stride" + s + r"void\s*\*stream\)", code)
    assert re.search(r"int\s+srz_mesh_edges_grad\s*\(\s*" + head + cf + "d_gout" + s + u + "gout_stride" + s + f + "d_work" + s + f + "d_gpos" + s
                     + r"void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER
    assert "(additive, same version) the mesh edge terms over a slot's connectivity: edge count, edge length and normal consistency" in HEADER


def test_the_constants_agree():
    from srz import abi
    for name, value in (("COUNT", 0), ("LENGTH", 1), ("DIHEDRAL", 2)):
        assert re.search(rf"#define\s+SRZ_EDGE_{name}\s+{value}\b", HEADER) and getattr(abi, "EDGE_" + name) == value
    assert len(abi.MESH_EDGES_ARGTYPES) == 9 and len(abi.MESH_EDGES_GRAD_ARGTYPES) == 11


def test_the_header_states_the_rules():
    # (a comment's line breaks and the spaces that align its cases are not the sentence's)
    flow = lambda text: re.sub(r" +", " ", re.sub(r"\s*\n \*\s*", " ", text))  # noqa: E731
    rule = flow(HEADER[HEADER.index("THE MESH EDGE TERMS over a slot's connectivity"):HEADER.index("int srz_mesh_edges(")])
    for sentence in ("EDGE j of a face (i0, i1, i2) lies opposite corner j", "a_j = i[(j + 1) % 3] and b_j = i[(j + 2) % 3]",
                     "THE NEIGHBOURS OF (f, j)", "has the SHORTER corner list, a_j on a tie", "in list order", "g == f: no entry",
                     "g[(k + 1) % 3] == o: the entry (g, (k + 2) % 3)", "else g[(k + 2) % 3] == o: the entry (g, (k + 1) % 3)",
                     "ONE entry per corner, never two", "follows this rule as written", "in float32, nothing fused",
                     "out[f][j] = (float)(1 + the number of entries)", "Positions are not read; n_sets must be 1",
                     "d = p[b_j] - p[a_j]; out[f][j] = sqrtf(dot3(d, d))", "N = cross(p[i1] - p[i0], p[i2] - p[i0])",
                     "ok = d2 > 0 && d2 <= FLT_MAX", "r = 1.0f / sqrtf(d2)", "f not ok: out[f][j] = +0",
                     "acc = acc + (1.0f - dot3(n_f, n_g))", "SKIPPED, never multiplied by zero", "the same word from both sides",
                     "no atomics", "DETERMINISTIC, bit for bit", "A slot with no faces is not an error",
                     "to the faces that name the vertex and to their edge neighbours only",
                     "No input value makes the pass read or write outside its buffers", "an unknown kind", "COUNT with n_sets != 1",
                     "out_stride below 3", "not 4-byte aligned"):
        assert sentence in rule, sentence
    back = flow(HEADER[HEADER.index("THE BACKWARD of srz_mesh_edges"):HEADER.index("int srz_mesh_edges_grad(")])
    for sentence in ("EVERY element written", "zeros for a slot with no faces", "it may be null there", "COUNT has no backward",
                     "v is the b end of edge j1 = (k + 1) % 3 and the a end of edge j2 = (k + 2) % 3",
                     "LIVE when len_j > 0 && len_j <= FLT_MAX", "u_j = d_j * (1.0f / len_j)", "acc = acc + gout[f][j1] * u_j1",
                     "acc = acc - gout[f][j2] * u_j2", "s = w[f][j] + w[g][j']", "H = H - n_g * s", "t = dot3(n_f, H)",
                     "gN[f] = (H - n_f * t) * r_f", "srz_mesh_normals_grad's phase 2 with G = gN of the corner's own face",
                     "k == 0: acc = acc + cross(b - c', G)", "k == 1: acc = acc + cross(c' - a, G)", "k == 2: acc = acc + cross(G, b - a)",
                     "no atomics", "DETERMINISTIC, bit for bit", "a null d_work under DIHEDRAL", "gout_stride below 3"):
        assert sentence in back, sentence


def test_binding_and_library_export_them():
    import srz
    from srz import visibility
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in NAMES:
        assert name in srz.EXPORTS and hasattr(lib, name), name
    for fn in ("mesh_edges", "mesh_edges_grad"):
        assert callable(getattr(srz.Context, fn))
    want = {"mesh_edge_counts": ["ctx", "slot", "stream"], "mesh_edge_lengths": ["ctx", "slot", "pos", "stream"],
            "mesh_normal_consistency": ["ctx", "slot", "pos", "stream"], "mesh_edge_loss": ["ctx", "slot", "pos", "target", "stream"],
            "mesh_normal_loss": ["ctx", "slot", "pos", "stream"]}
    for fn, params in want.items():
        assert list(inspect.signature(getattr(visibility, fn)).parameters) == params, fn
    assert inspect.signature(visibility.mesh_edge_loss).parameters["target"].default == 0.0
    L = srz.lib()
    assert L.srz_abi_version() == 7
    assert L.srz_mesh_edges.argtypes == srz.abi.MESH_EDGES_ARGTYPES and L.srz_mesh_edges_grad.argtypes == srz.abi.MESH_EDGES_GRAD_ARGTYPES
    # without a context: SRZ_E_INVALID whatever else is passed, nothing dereferenced
    assert L.srz_mesh_edges(None, 0, None, 0, 0, 0, None, 0, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_mesh_edges_grad(None, 0, None, 0, 0, 0, None, 0, None, None, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_mesh_edges(None, 7, 4096, 3, 1, 2, 8192, 3, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_mesh_edges_grad(None, 7, 4096, 3, 1, 1, 8192, 3, None, 16384, None) == srz.abi.SRZ_E_INVALID


def test_the_new_layer_has_no_refusal_of_its_own():
    """every tensor goes through _sets_arg: the five functions and the Function behind them raise nothing themselves"""
    from srz import visibility
    for fn in ("_face_field", "mesh_edge_counts", "_MeshEdges", "mesh_edge_lengths", "mesh_normal_consistency", "mesh_edge_loss", "mesh_normal_loss"):
        src = inspect.getsource(getattr(visibility, fn))
        assert "raise " not in src, fn
    assert "_sets_arg(sctx, slot, pos, \"pos\", who)" in inspect.getsource(visibility._MeshEdges)
