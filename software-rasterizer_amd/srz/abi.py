"""ctypes mirror of include/srz.h (the C ABI of the raster + fragment-shade stage).

Pure data definitions: no library is loaded here, so the oracle wrapper (tests only) and the
product binding (srz/__init__.py) can both build identical `srz_frame` inputs.
"""
import ctypes as C

import numpy as np

SRZ_ABI_VERSION = 7  # = include/srz.h; srz.lib() refuses a library that reports another one
SRZ_OK = 0
SRZ_E_INVALID, SRZ_E_NODEVICE, SRZ_E_NOMEM, SRZ_E_TEXTURE, SRZ_E_PRIMITIVE = -1, -2, -3, -4, -5
SHADER_NORMAL, SHADER_TEXTURE, SHADER_PHONG, SHADER_DISPLACEMENT, SHADER_BUMP = 0, 1, 2, 3, 4
PRIMITIVE_LINES, PRIMITIVE_TRIANGLES = 0, 1
EXACT_SPLIT, UNIFIED, FUSED_CLEAR, ORDERED_RASTER, NO_Z_READBACK = 0, 1, 2, 4, 8
EXCHANGE_PLANES, EXCHANGE_BGR8 = 0, 1
OPT_POOL_LAZY, OPT_APPROX_SHADE = 1, 2  # srz_set_option
GB_NORMAL, GB_UV, GB_BATCH, GB_ALBEDO = 1, 2, 4, 8  # srz_frameset_gbuffer: the groups of `what` (3, 2, 1, 3 planes, in this order)
GB_ALL = GB_NORMAL | GB_UV | GB_BATCH | GB_ALBEDO
MV_FLOW, MV_DEPTH, MV_TARGET = 1, 2, 4  # srz_frameset_motion: the groups of `what` (2, 1, 2 planes, in this order)
MV_ALL = MV_FLOW | MV_DEPTH | MV_TARGET
ATTR_MAX_CH = 64  # srz_frameset_interpolate: the most channels of one call (SRZ_ATTR_MAX_CH)
TEX_CLAMP, TEX_WRAP = 0, 1  # srz_frameset_texture: `mode` (SRZ_TEX_CLAMP, SRZ_TEX_WRAP)
TEX_MAX_SIZE = 16384  # srz_frameset_texture: the largest tex_w and tex_h (SRZ_TEX_MAX_SIZE)
LIGHT_MAX = 8  # srz_frameset_light: the most lights of one call (SRZ_LIGHT_MAX)


def light_par(n_lights):
    """floats of one parameter frame of srz_frameset_light: eye[3] ka[3] ks[3], then n_lights x {pos[3], intensity[3]} (SRZ_LIGHT_PAR)"""
    return 9 + 6 * n_lights


def microfacet_par(n_lights):
    """floats of one parameter frame of srz_frameset_microfacet: eye[3] amb[3], then n_lights x {pos[3], intensity[3]}
    (SRZ_MICROFACET_PAR)"""
    return 6 + 6 * n_lights
# the prototypes of srz_frameset_texture / _texture_grad (argtypes; both return int), set on the library by srz.lib()
TEXTURE_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                    C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
TEXTURE_GRAD_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                         C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
TEX_MAX_LEVELS = 15  # the most levels of a mip pyramid, level 0 included (SRZ_TEX_MAX_LEVELS)
# the prototypes of the mip entry points (argtypes; the two helpers return uint32 / size_t, the others int), set by srz.lib()
_vp, _u32 = C.c_void_p, C.c_uint32
MIP_LEVELS_ARGTYPES = [_u32, _u32]
MIP_BYTES_ARGTYPES = [_u32, _u32, _u32, _u32, _u32]
MIP_BUILD_ARGTYPES = [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, C.c_size_t, _vp]
MIP_FOLD_ARGTYPES = [_vp, _vp, C.c_size_t, _u32, _u32, _u32, _u32, _u32, _vp, _vp]
INTERPOLATE_DERIV_ARGTYPES = [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, C.c_size_t, _u32, _vp]
TEXTURE_MIP_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, C.c_size_t, _u32, _vp]
TEXTURE_MIP_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _u32, _vp]
# the prototypes of srz_frameset_texture_cube / _texture_cube_grad (argtypes; both return int), set by srz.lib()
TEXTURE_CUBE_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, C.c_size_t, _u32, _vp]
TEXTURE_CUBE_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp]
# the prototypes of srz_frameset_background / _background_work_bytes (returns size_t) / _background_grad (argtypes), set by srz.lib()
BG_NOBODY, BG_ALL = 0, 1  # srz_frameset_background: `where` (SRZ_BG_NOBODY, SRZ_BG_ALL)
BACKGROUND_ARGTYPES = [_vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _vp, C.c_size_t, _u32, _vp]
BACKGROUND_WORK_BYTES_ARGTYPES = [_vp, _vp]
BACKGROUND_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, C.c_size_t, _u32, _vp]
# the prototypes of the cube pyramid's entry points srz_cube_mip_levels (returns uint32) / _bytes (size_t) / _build / _fold and of
# srz_frameset_texture_cube_mip / _texture_cube_mip_grad / srz_frameset_cube_level (argtypes), set by srz.lib()
CUBE_MIP_LEVELS_ARGTYPES = [_u32]
CUBE_MIP_BYTES_ARGTYPES = [_u32, _u32, _u32, _u32]
CUBE_MIP_BUILD_ARGTYPES = [_vp, _vp, _u32, _u32, _u32, _u32, _vp, C.c_size_t, _vp]
CUBE_MIP_FOLD_ARGTYPES = [_vp, _vp, C.c_size_t, _u32, _u32, _u32, _u32, _vp, _vp]
TEXTURE_CUBE_MIP_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _u32, _vp, C.c_size_t, _u32, _vp]
TEXTURE_CUBE_MIP_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _u32, _vp]
CUBE_LEVEL_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, C.c_size_t, _u32, _vp]
# the prototypes of srz_frameset_light / _light_work_bytes (returns size_t) / _light_grad (argtypes), set by srz.lib()
LIGHT_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, C.c_size_t, _u32, _vp]
LIGHT_WORK_BYTES_ARGTYPES = [_vp, _vp, _u32]
LIGHT_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _u32, _vp]
# the prototypes of srz_frameset_microfacet / _microfacet_work_bytes (returns size_t) / _microfacet_grad (argtypes), set by srz.lib()
MICROFACET_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, C.c_size_t, _u32, _vp]
MICROFACET_WORK_BYTES_ARGTYPES = [_vp, _vp, _u32]
MICROFACET_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _u32, _vp]
# the prototypes of srz_mesh_tangents / _tangents_grad and srz_frameset_normal_map / _normal_map_grad (argtypes; all return int)
MESH_TANGENTS_ARGTYPES = [_vp, C.c_int, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp]
MESH_TANGENTS_GRAD_ARGTYPES = [_vp, C.c_int, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp]
NORMAL_MAP_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _u32, _vp]
NORMAL_MAP_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]
# srz_mesh_laplacian / _laplacian_grad: `kind` (SRZ_LAP_*), the most channels of one call, and the prototype the two share
LAP_UMBRELLA, LAP_GRAPH, LAP_COTAN = 0, 1, 2
LAP_MAX_CH = 64
MESH_LAPLACIAN_ARGTYPES = [_vp, C.c_int, _vp, _u32, _u32, _u32, C.c_int, _vp, _u32, _vp, _u32, _vp]
# srz_mesh_edges / _edges_grad: `kind` (SRZ_EDGE_*) and the two prototypes
EDGE_COUNT, EDGE_LENGTH, EDGE_DIHEDRAL = 0, 1, 2
MESH_EDGES_ARGTYPES = [_vp, C.c_int, _vp, _u32, _u32, C.c_int, _vp, _u32, _vp]
MESH_EDGES_GRAD_ARGTYPES = [_vp, C.c_int, _vp, _u32, _u32, C.c_int, _vp, _u32, _vp, _vp, _vp]
# the prototypes of srz_frameset_shadow / _shadow_grad (argtypes; both return int), set by srz.lib()
SHADOW_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, C.c_float, C.c_float, _vp, C.c_size_t, _u32, _vp]
SHADOW_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, C.c_float, C.c_float, _vp, _vp, _u32, _vp]
# the prototypes of srz_frameset_perspective / _perspective_grad / _interpolate_deriv_persp (argtypes; all return int), set by srz.lib()
PERSPECTIVE_ARGTYPES = [_vp, _vp, _vp, _vp, _u32, _u32, _vp, C.c_size_t, _u32, _vp]
PERSPECTIVE_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _vp]
INTERPOLATE_DERIV_PERSP_ARGTYPES = [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _u32, _u32, _u32, _vp, C.c_size_t, _u32, _vp]
# the prototypes of srz_cube_prefilter_work_bytes (returns size_t) / srz_cube_prefilter / _prefilter_grad (argtypes), set by srz.lib()
PREFILTER_COSINE, PREFILTER_GGX = 0, 1  # SRZ_PREFILTER_*
CUBE_PREFILTER_WORK_BYTES_ARGTYPES = [_u32, _u32, _u32, _u32]
CUBE_PREFILTER_ARGTYPES = [_vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, C.c_float, C.c_float, _vp, _vp, C.c_size_t, _vp]
CUBE_PREFILTER_GRAD_ARGTYPES = [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, C.c_float, C.c_float, _vp, _vp, C.c_size_t, _vp]
# the prototypes of srz_cube_sh_work_bytes (returns size_t) / srz_cube_sh / _cube_sh_grad and of srz_frameset_sh / _sh_work_bytes
# (returns size_t) / _sh_grad (argtypes), set by srz.lib()
SH_MAX_CH = 7  # srz_cube_sh, srz_frameset_sh: the most channels of one call (SRZ_SH_MAX_CH)
SH_IRRADIANCE, SH_RADIANCE = 0, 1  # srz_frameset_sh: `kind` (SRZ_SH_*)
CUBE_SH_WORK_BYTES_ARGTYPES = [_u32, _u32, _u32]
CUBE_SH_ARGTYPES = [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, C.c_size_t, _vp]
CUBE_SH_GRAD_ARGTYPES = [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, C.c_size_t, _vp]
SH_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, C.c_size_t, _u32, _vp]
SH_WORK_BYTES_ARGTYPES = [_vp, _vp, _u32]
SH_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, C.c_size_t, _u32, _vp]
# the prototypes of srz_frameset_reflect / _reflect_grad / srz_brdf_table / srz_frameset_ibl / _ibl_grad (argtypes; all return int)
BRDF_TABLE_MAX = 64  # srz_brdf_table, srz_frameset_ibl: the largest table side (SRZ_BRDF_TABLE_MAX)
REFLECT_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, C.c_size_t, _u32, _vp]
REFLECT_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _vp]
BRDF_TABLE_ARGTYPES = [_vp, _vp, C.c_size_t, _u32, _u32, _vp]
IBL_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, C.c_size_t, _u32, _vp]
IBL_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]
# the prototypes of srz_frameset_composite / _composite_grad (argtypes; both return int), set by srz.lib()
COMPOSITE_MAX = 8  # srz_frameset_composite: the most layers of one call (SRZ_COMPOSITE_MAX)
COMPOSITE_ARGTYPES = [_vp, _vp, _vp, _u32, _u32, _vp, _u32, _vp, C.c_size_t, _u32, _vp]
COMPOSITE_GRAD_ARGTYPES = [_vp, _vp, _vp, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _vp, _u32, _vp]
# the prototypes of srz_frameset_texture_set / _texture_set_grad (argtypes; both return int), set on the library by srz.lib()
TEXSET_MAX = 8  # srz_frameset_texture_set: the most slots of one call (SRZ_TEXSET_MAX)
TEXSET_NONE = 0xff  # the conventional "no slot" byte of the batch -> slot map (SRZ_TEXSET_NONE)
TEXTURE_SET_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _vp, C.c_size_t, _u32, _vp]
TEXTURE_SET_GRAD_ARGTYPES = [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _vp, _u32, _vp]

# numpy view of srz_tri (96 B): pos[3][3], nrm[3][3], uv[3][2]
TRI_DTYPE = np.dtype([("pos", "<f4", (3, 3)), ("nrm", "<f4", (3, 3)), ("uv", "<f4", (3, 2))])
LIGHT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("intensity", "<f4", (3,))])
VERTEX_DTYPE = np.dtype([("pos", "<f4", (3,)), ("nrm", "<f4", (3,)), ("uv", "<f4", (2,))])
assert TRI_DTYPE.itemsize == 96 and LIGHT_DTYPE.itemsize == 24 and VERTEX_DTYPE.itemsize == 32


class SrzBatch(C.Structure):
    _fields_ = [("shader", C.c_int32), ("tex_id", C.c_int32), ("n_tris", C.c_uint32), ("_pad", C.c_uint32),
                ("tris", C.c_void_p)]


class SrzFrame(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("eye", C.c_float * 3), ("ka", C.c_float * 3),
                ("ks", C.c_float * 3), ("p", C.c_float), ("kh", C.c_float), ("kn", C.c_float),
                ("n_lights", C.c_uint32), ("n_batches", C.c_uint32), ("lights", C.c_void_p),
                ("batches", C.c_void_p), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class SrzMeshDraw(C.Structure):
    _fields_ = [("mesh_id", C.c_int32), ("shader", C.c_int32), ("tex_id", C.c_int32), ("_pad", C.c_int32),
                ("ndc_mvp", C.c_float * 16), ("normal_m", C.c_float * 16)]


class SrzSceneFrame(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("eye", C.c_float * 3), ("ka", C.c_float * 3),
                ("ks", C.c_float * 3), ("p", C.c_float), ("kh", C.c_float), ("kn", C.c_float),
                ("zscale", C.c_float), ("zoffset", C.c_float), ("n_lights", C.c_uint32), ("n_draws", C.c_uint32),
                ("lights", C.c_void_p), ("draws", C.c_void_p), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class SrzCompositeLayer(C.Structure):
    """srz_composite_layer: one layer of srz_frameset_composite (three device pointers; alpha None: the scalar opacity)"""
    _fields_ = [("vis", C.c_void_p), ("color", C.c_void_p), ("alpha", C.c_void_p), ("opacity", C.c_float), ("_pad", C.c_uint32)]


def composite_layers_array(layers):
    """layers: (vis_ptr, color_ptr, alpha_ptr or None, opacity) per layer → a ctypes array of srz_composite_layer"""
    arr = (SrzCompositeLayer * max(1, len(layers)))()
    for i, (vis, color, alpha, opacity) in enumerate(layers):
        arr[i] = SrzCompositeLayer(vis or None, color or None, alpha or None, float(opacity), 0)
    return arr


class SrzTexsetSlot(C.Structure):
    """srz_texset_slot: one texture of srz_frameset_texture_set (d_gtex: the backward's, None = this slot's gradient is not wanted)"""
    _fields_ = [("d_tex", C.c_void_p), ("d_gtex", C.c_void_p), ("tex_w", C.c_uint32), ("tex_h", C.c_uint32),
                ("tex_frames", C.c_uint32), ("mode", C.c_uint32)]


def texset_slots_array(slots):
    """slots: (tex_ptr or None, gtex_ptr or None, tex_w, tex_h, tex_frames, mode) per slot → a ctypes array of srz_texset_slot"""
    arr = (SrzTexsetSlot * max(1, len(slots)))()
    for i, (tex, gtex, w, h, frames, mode) in enumerate(slots):
        arr[i] = SrzTexsetSlot(tex or None, gtex or None, int(w), int(h), int(frames), int(mode))
    return arr


class SrzStats(C.Structure):
    _fields_ = [("n_tris", C.c_uint64), ("n_culled", C.c_uint64), ("pixel_tests", C.c_uint64),
                ("fragments", C.c_uint64), ("shaded", C.c_uint64), ("visible", C.c_uint64),
                ("visible_textured", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# Shader statics of the reference (src/Shader.cpp:7-12)
DEFAULT_KA = (0.005, 0.005, 0.005)
DEFAULT_KS = (0.7937, 0.7937, 0.7937)
DEFAULT_P, DEFAULT_KH, DEFAULT_KN = 150.0, 0.2, 0.1


class Frame:
    """Python-side owner of one srz_frame and the numpy arrays it points into."""

    def __init__(self, width, height, eye, lights, batches, flags=0, ka=DEFAULT_KA, ks=DEFAULT_KS, p=DEFAULT_P,
                 kh=DEFAULT_KH, kn=DEFAULT_KN):
        """lights: array-like (n,2,3) or LIGHT_DTYPE; batches: list of (shader, tex_id, tris[TRI_DTYPE])."""
        self.lights = np.ascontiguousarray(np.asarray(lights, dtype=np.float32).reshape(-1, 6)).view(LIGHT_DTYPE).reshape(-1) \
            if not (isinstance(lights, np.ndarray) and lights.dtype == LIGHT_DTYPE) else np.ascontiguousarray(lights)
        self.tris = []
        self._batches = (SrzBatch * max(1, len(batches)))()
        for i, (shader, tex_id, tris) in enumerate(batches):
            t = np.ascontiguousarray(tris)
            if t.dtype != TRI_DTYPE:
                t = np.ascontiguousarray(np.asarray(t, dtype=np.float32).reshape(-1, 24)).view(TRI_DTYPE).reshape(-1)
            self.tris.append(t)
            self._batches[i] = SrzBatch(int(shader), int(tex_id), len(t), 0, t.ctypes.data if len(t) else None)
        f = SrzFrame()
        f.width, f.height = int(width), int(height)
        f.eye[:] = [float(x) for x in eye]
        f.ka[:] = [float(x) for x in ka]
        f.ks[:] = [float(x) for x in ks]
        f.p, f.kh, f.kn = float(p), float(kh), float(kn)
        f.n_lights, f.n_batches = len(self.lights), len(batches)
        f.lights = self.lights.ctypes.data if len(self.lights) else None
        f.batches = C.cast(self._batches, C.c_void_p).value
        f.flags = int(flags)
        self.c = f

    @property
    def width(self):
        return self.c.width

    @property
    def height(self):
        return self.c.height

    @property
    def n_tris(self):
        return sum(len(t) for t in self.tris)

    def with_flags(self, flags):
        self.c.flags = int(flags)
        return self


class SceneFrame:
    """Python-side owner of one srz_scene_frame (meshes by slot + the vertex-stage matrices)."""

    def __init__(self, width, height, eye, lights, draws, zscale, zoffset, flags=0, ka=DEFAULT_KA, ks=DEFAULT_KS,
                 p=DEFAULT_P, kh=DEFAULT_KH, kn=DEFAULT_KN):
        """draws: list of (mesh_id, shader, tex_id, ndc_mvp[16], normal_m[16])."""
        self.lights = np.ascontiguousarray(np.asarray(lights, dtype=np.float32).reshape(-1, 6)).view(LIGHT_DTYPE).reshape(-1)
        self._draws = (SrzMeshDraw * max(1, len(draws)))()
        for i, (mesh_id, shader, tex_id, mvp, nm) in enumerate(draws):
            d = self._draws[i]
            d.mesh_id, d.shader, d.tex_id = int(mesh_id), int(shader), int(tex_id)
            d.ndc_mvp[:] = [float(x) for x in np.asarray(mvp, np.float32).reshape(16)]
            d.normal_m[:] = [float(x) for x in np.asarray(nm, np.float32).reshape(16)]
        f = SrzSceneFrame()
        f.width, f.height = int(width), int(height)
        f.eye[:] = [float(x) for x in eye]
        f.ka[:] = [float(x) for x in ka]
        f.ks[:] = [float(x) for x in ks]
        f.p, f.kh, f.kn = float(p), float(kh), float(kn)
        f.zscale, f.zoffset = float(zscale), float(zoffset)
        f.n_lights, f.n_draws = len(self.lights), len(draws)
        f.lights = self.lights.ctypes.data if len(self.lights) else None
        f.draws = C.cast(self._draws, C.c_void_p).value
        f.flags = int(flags)
        self.c = f

    @property
    def width(self):
        return self.c.width

    @property
    def height(self):
        return self.c.height


def scene_frames_array(frames):
    arr = (SrzSceneFrame * len(frames))()
    for i, f in enumerate(frames):
        arr[i] = f.c
    return arr


def frames_array(frames):
    arr = (SrzFrame * len(frames))()
    for i, f in enumerate(frames):
        arr[i] = f.c
    return arr
