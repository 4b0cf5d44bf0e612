"""srz — Python binding (ctypes) of the C ABI in include/srz.h, the MI355X raster + fragment-shade stage.

The compute path is ONLY libsrz.so (hand-written gfx950 kernels).  There is no CPU fallback: if the
library is missing or no gfx950 device is present, every call raises.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from .abi import Frame  # noqa: F401

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("SRZ_LIB_PATH", os.path.join(_PKG, "libsrz.so"))  # (override: A/B of dev builds)
_lib = None

EXPORTS = ["srz_abi_version", "srz_create", "srz_destroy", "srz_last_error", "srz_set_shard", "srz_set_option", "srz_texture_upload",
           "srz_draw", "srz_draw_scene", "srz_mesh_upload", "srz_mesh_update", "srz_sceneset_create", "srz_frameset_create", "srz_frameset_destroy", "srz_frameset_local_rows",
           "srz_frameset_out_bytes", "srz_frameset_render", "srz_frameset_resolve8", "srz_frameset_stats", "srz_frameset_algorithmic_bytes",
           "srz_kernel_time_ms", "srz_kernel_time_samples", "srz_set_kernel_timing", "srz_sync", "srz_debug_counters", "srz_verify_fastmath", "srz_verify_fastdiv", "srz_verify_fastpow", "srz_verify_fastlen", "srz_host_register", "srz_host_unregister", "srz_frameset_debug_counters", "srz_draw_batch",
           "srz_comm_unique_id", "srz_comm_create", "srz_comm_destroy", "srz_frameset_exchange_bytes", "srz_frameset_allgather",
           "srz_frameset_deinterleave", "srz_frameset_allgather_inplace", "srz_frameset_gathered_row_offset",
           "srz_frameset_read_gathered_frame", "srz_frameset_sparse_capacity", "srz_frameset_sparse_pack", "srz_frameset_sparse_unpack",
           "srz_frameset_allgather_sparse", "srz_frameset_render_visibility", "srz_frameset_peel_visibility", "srz_frameset_shade_visibility",
           "srz_frameset_update_shading", "srz_frameset_shade_kinds", "srz_frameset_gbuffer_bytes", "srz_frameset_gbuffer",
           "srz_frameset_motion_bytes", "srz_frameset_motion", "srz_frameset_interpolate_bytes", "srz_frameset_interpolate",
           "srz_frameset_interpolate_grad", "srz_frameset_position_grad", "srz_frameset_antialias", "srz_frameset_antialias_grad",
           "srz_frameset_positions", "srz_sceneset_vertex_grad",
           "srz_mesh_normals", "srz_mesh_normals_grad", "srz_sceneset_corner_attr", "srz_sceneset_corner_attr_grad",
           "srz_frameset_texture", "srz_frameset_texture_grad",
           "srz_texture_mip_levels", "srz_texture_mip_bytes", "srz_texture_mip_build", "srz_texture_mip_fold",
           "srz_frameset_interpolate_deriv", "srz_frameset_texture_mip", "srz_frameset_texture_mip_grad",
           "srz_frameset_texture_cube", "srz_frameset_texture_cube_grad",
           "srz_frameset_background", "srz_frameset_background_work_bytes", "srz_frameset_background_grad",
           "srz_cube_mip_levels", "srz_cube_mip_bytes", "srz_cube_mip_build", "srz_cube_mip_fold",
           "srz_frameset_texture_cube_mip", "srz_frameset_texture_cube_mip_grad", "srz_frameset_cube_level",
           "srz_cube_prefilter_work_bytes", "srz_cube_prefilter", "srz_cube_prefilter_grad",
           "srz_cube_sh_work_bytes", "srz_cube_sh", "srz_cube_sh_grad",
           "srz_frameset_sh", "srz_frameset_sh_work_bytes", "srz_frameset_sh_grad",
           "srz_frameset_light", "srz_frameset_light_work_bytes", "srz_frameset_light_grad",
           "srz_frameset_microfacet", "srz_frameset_microfacet_work_bytes", "srz_frameset_microfacet_grad",
           "srz_frameset_reflect", "srz_frameset_reflect_grad", "srz_brdf_table", "srz_frameset_ibl", "srz_frameset_ibl_grad",
           "srz_frameset_shadow", "srz_frameset_shadow_grad",
           "srz_mesh_tangents", "srz_mesh_tangents_grad", "srz_frameset_normal_map", "srz_frameset_normal_map_grad",
           "srz_mesh_laplacian", "srz_mesh_laplacian_grad",
           "srz_mesh_edges", "srz_mesh_edges_grad",
           "srz_frameset_composite", "srz_frameset_composite_grad",
           "srz_frameset_texture_set", "srz_frameset_texture_set_grad",
           "srz_frameset_perspective", "srz_frameset_perspective_grad", "srz_frameset_interpolate_deriv_persp",
           "srz_target_create", "srz_target_destroy", "srz_target_clear", "srz_target_draw", "srz_target_read", "srz_target_read_bgr8"]


class SrzError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"srz error {code}: {msg}")
        self.code = code


def lib():
    """Load libsrz.so (fails loudly if it was not built: run `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found — the HIP extension is not built and there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        # a binding and a library that disagree on the ABI (a stale build, SRZ_LIB_PATH pointing at another checkout) must not
        # get as far as a call: argument MEANINGS change between versions (v3: the stream sentinel), not only signatures
        L.srz_abi_version.restype = C.c_int
        got = L.srz_abi_version()
        if got != abi.SRZ_ABI_VERSION:
            raise ImportError(f"{LIB_PATH} reports SRZ_ABI_VERSION {got}, this binding is written against {abi.SRZ_ABI_VERSION}: "
                              "rebuild the library (python -c 'import __graft_entry__ as g; g.build()') or fix SRZ_LIB_PATH")
        fp, vp = C.POINTER(C.c_float), C.c_void_p
        L.srz_create.argtypes = [C.POINTER(vp), C.c_int]
        L.srz_destroy.argtypes = [vp]
        L.srz_destroy.restype = None
        L.srz_last_error.argtypes = [vp]
        L.srz_last_error.restype = C.c_char_p
        L.srz_set_shard.argtypes = [vp, C.c_int, C.c_int]
        L.srz_set_option.argtypes = [vp, C.c_int, C.c_int]
        L.srz_texture_upload.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int]
        L.srz_draw.argtypes = [vp, C.c_int, C.POINTER(abi.SrzFrame), fp, fp, fp, fp, C.POINTER(abi.SrzStats)]
        L.srz_draw_batch.argtypes = [vp, C.c_int, C.POINTER(abi.SrzFrame), C.c_int, C.POINTER(fp), C.POINTER(abi.SrzStats)]
        L.srz_frameset_create.argtypes = [vp, C.POINTER(abi.SrzFrame), C.c_int, C.POINTER(vp)]
        L.srz_sceneset_create.argtypes = [vp, C.POINTER(abi.SrzSceneFrame), C.c_int, C.POINTER(vp)]
        L.srz_mesh_upload.argtypes = [vp, C.c_int, vp, C.c_uint32, vp, C.c_uint32]
        L.srz_mesh_update.argtypes = [vp, C.c_int, vp, C.c_uint32, vp]
        L.srz_draw_scene.argtypes = [vp, C.c_int, C.POINTER(abi.SrzSceneFrame), fp, fp, fp, fp, C.POINTER(abi.SrzStats)]
        L.srz_frameset_destroy.argtypes = [vp, vp]
        L.srz_frameset_destroy.restype = None
        L.srz_frameset_local_rows.argtypes = [vp, vp]
        L.srz_frameset_out_bytes.argtypes = [vp, vp]
        L.srz_frameset_out_bytes.restype = C.c_size_t
        L.srz_frameset_render.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp]
        L.srz_frameset_render_visibility.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp]
        L.srz_frameset_peel_visibility.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_uint32, vp]
        L.srz_frameset_shade_visibility.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_uint32, vp]
        L.srz_frameset_gbuffer_bytes.argtypes = [vp, vp, C.c_uint32]
        L.srz_frameset_gbuffer_bytes.restype = C.c_size_t
        L.srz_frameset_gbuffer.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp]
        L.srz_frameset_motion_bytes.argtypes = [vp, vp, C.c_uint32]
        L.srz_frameset_motion_bytes.restype = C.c_size_t
        L.srz_frameset_motion.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_uint32, C.c_int, C.c_uint32, vp]
        L.srz_frameset_interpolate_bytes.argtypes = [vp, vp, C.c_uint32]
        L.srz_frameset_interpolate_bytes.restype = C.c_size_t
        L.srz_frameset_interpolate.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t, C.c_uint32, vp]
        L.srz_frameset_interpolate_grad.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp]
        L.srz_frameset_position_grad.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp]
        L.srz_frameset_positions.argtypes = [vp, vp, C.c_uint32, vp, C.c_size_t, vp]
        L.srz_sceneset_vertex_grad.argtypes = [vp, vp, C.c_int, vp, C.c_uint32, vp, vp, C.c_uint32, vp]
        L.srz_mesh_normals.argtypes = [vp, C.c_int, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp]
        L.srz_mesh_normals_grad.argtypes = [vp, C.c_int, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp]
        L.srz_sceneset_corner_attr.argtypes = [vp, vp, C.c_int, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp]
        L.srz_sceneset_corner_attr_grad.argtypes = [vp, vp, C.c_int, vp, C.c_uint32, vp, C.c_uint32, vp]
        L.srz_frameset_antialias.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, C.c_size_t, C.c_uint32, vp]
        L.srz_frameset_antialias_grad.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp]
        L.srz_frameset_texture.argtypes = abi.TEXTURE_ARGTYPES
        L.srz_frameset_texture_grad.argtypes = abi.TEXTURE_GRAD_ARGTYPES
        L.srz_texture_mip_levels.argtypes = abi.MIP_LEVELS_ARGTYPES
        L.srz_texture_mip_levels.restype = C.c_uint32
        L.srz_texture_mip_bytes.argtypes = abi.MIP_BYTES_ARGTYPES
        L.srz_texture_mip_bytes.restype = C.c_size_t
        L.srz_texture_mip_build.argtypes = abi.MIP_BUILD_ARGTYPES
        L.srz_texture_mip_fold.argtypes = abi.MIP_FOLD_ARGTYPES
        L.srz_frameset_interpolate_deriv.argtypes = abi.INTERPOLATE_DERIV_ARGTYPES
        L.srz_frameset_texture_mip.argtypes = abi.TEXTURE_MIP_ARGTYPES
        L.srz_frameset_texture_mip_grad.argtypes = abi.TEXTURE_MIP_GRAD_ARGTYPES
        L.srz_frameset_texture_cube.argtypes = abi.TEXTURE_CUBE_ARGTYPES
        L.srz_frameset_texture_cube_grad.argtypes = abi.TEXTURE_CUBE_GRAD_ARGTYPES
        L.srz_frameset_background.argtypes = abi.BACKGROUND_ARGTYPES
        L.srz_frameset_background_work_bytes.argtypes = abi.BACKGROUND_WORK_BYTES_ARGTYPES
        L.srz_frameset_background_work_bytes.restype = C.c_size_t
        L.srz_frameset_background_grad.argtypes = abi.BACKGROUND_GRAD_ARGTYPES
        L.srz_cube_mip_levels.argtypes = abi.CUBE_MIP_LEVELS_ARGTYPES
        L.srz_cube_mip_levels.restype = C.c_uint32
        L.srz_cube_mip_bytes.argtypes = abi.CUBE_MIP_BYTES_ARGTYPES
        L.srz_cube_mip_bytes.restype = C.c_size_t
        L.srz_cube_mip_build.argtypes = abi.CUBE_MIP_BUILD_ARGTYPES
        L.srz_cube_mip_fold.argtypes = abi.CUBE_MIP_FOLD_ARGTYPES
        L.srz_frameset_texture_cube_mip.argtypes = abi.TEXTURE_CUBE_MIP_ARGTYPES
        L.srz_frameset_texture_cube_mip_grad.argtypes = abi.TEXTURE_CUBE_MIP_GRAD_ARGTYPES
        L.srz_frameset_cube_level.argtypes = abi.CUBE_LEVEL_ARGTYPES
        L.srz_cube_prefilter_work_bytes.argtypes = abi.CUBE_PREFILTER_WORK_BYTES_ARGTYPES
        L.srz_cube_prefilter_work_bytes.restype = C.c_size_t
        L.srz_cube_prefilter.argtypes = abi.CUBE_PREFILTER_ARGTYPES
        L.srz_cube_prefilter_grad.argtypes = abi.CUBE_PREFILTER_GRAD_ARGTYPES
        L.srz_cube_sh_work_bytes.argtypes = abi.CUBE_SH_WORK_BYTES_ARGTYPES
        L.srz_cube_sh_work_bytes.restype = C.c_size_t
        L.srz_cube_sh.argtypes = abi.CUBE_SH_ARGTYPES
        L.srz_cube_sh_grad.argtypes = abi.CUBE_SH_GRAD_ARGTYPES
        L.srz_frameset_sh.argtypes = abi.SH_ARGTYPES
        L.srz_frameset_sh_work_bytes.argtypes = abi.SH_WORK_BYTES_ARGTYPES
        L.srz_frameset_sh_work_bytes.restype = C.c_size_t
        L.srz_frameset_sh_grad.argtypes = abi.SH_GRAD_ARGTYPES
        L.srz_frameset_light.argtypes = abi.LIGHT_ARGTYPES
        L.srz_frameset_light_work_bytes.argtypes = abi.LIGHT_WORK_BYTES_ARGTYPES
        L.srz_frameset_light_work_bytes.restype = C.c_size_t
        L.srz_frameset_light_grad.argtypes = abi.LIGHT_GRAD_ARGTYPES
        L.srz_frameset_microfacet.argtypes = abi.MICROFACET_ARGTYPES
        L.srz_frameset_microfacet_work_bytes.argtypes = abi.MICROFACET_WORK_BYTES_ARGTYPES
        L.srz_frameset_microfacet_work_bytes.restype = C.c_size_t
        L.srz_frameset_microfacet_grad.argtypes = abi.MICROFACET_GRAD_ARGTYPES
        L.srz_frameset_reflect.argtypes = abi.REFLECT_ARGTYPES
        L.srz_frameset_reflect_grad.argtypes = abi.REFLECT_GRAD_ARGTYPES
        L.srz_brdf_table.argtypes = abi.BRDF_TABLE_ARGTYPES
        L.srz_frameset_ibl.argtypes = abi.IBL_ARGTYPES
        L.srz_frameset_ibl_grad.argtypes = abi.IBL_GRAD_ARGTYPES
        L.srz_mesh_tangents.argtypes = abi.MESH_TANGENTS_ARGTYPES
        L.srz_mesh_tangents_grad.argtypes = abi.MESH_TANGENTS_GRAD_ARGTYPES
        L.srz_mesh_laplacian.argtypes = L.srz_mesh_laplacian_grad.argtypes = abi.MESH_LAPLACIAN_ARGTYPES
        L.srz_mesh_edges.argtypes = abi.MESH_EDGES_ARGTYPES
        L.srz_mesh_edges_grad.argtypes = abi.MESH_EDGES_GRAD_ARGTYPES
        L.srz_frameset_normal_map.argtypes = abi.NORMAL_MAP_ARGTYPES
        L.srz_frameset_normal_map_grad.argtypes = abi.NORMAL_MAP_GRAD_ARGTYPES
        L.srz_frameset_composite.argtypes = abi.COMPOSITE_ARGTYPES
        L.srz_frameset_composite_grad.argtypes = abi.COMPOSITE_GRAD_ARGTYPES
        L.srz_frameset_texture_set.argtypes = abi.TEXTURE_SET_ARGTYPES
        L.srz_frameset_texture_set_grad.argtypes = abi.TEXTURE_SET_GRAD_ARGTYPES
        L.srz_frameset_shadow.argtypes = abi.SHADOW_ARGTYPES
        L.srz_frameset_shadow_grad.argtypes = abi.SHADOW_GRAD_ARGTYPES
        L.srz_frameset_perspective.argtypes = abi.PERSPECTIVE_ARGTYPES
        L.srz_frameset_perspective_grad.argtypes = abi.PERSPECTIVE_GRAD_ARGTYPES
        L.srz_frameset_interpolate_deriv_persp.argtypes = abi.INTERPOLATE_DERIV_PERSP_ARGTYPES
        L.srz_frameset_update_shading.argtypes = [vp, vp, C.POINTER(abi.SrzFrame), C.c_int]
        L.srz_sceneset_update.argtypes = [vp, vp, C.POINTER(abi.SrzSceneFrame), C.c_int]
        L.srz_frameset_resolve8.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
        L.srz_frameset_stats.argtypes = [vp, vp, C.POINTER(abi.SrzStats)]
        L.srz_frameset_algorithmic_bytes.argtypes = [vp, vp]
        L.srz_frameset_algorithmic_bytes.restype = C.c_uint64
        L.srz_kernel_time_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.srz_set_kernel_timing.argtypes = [vp, C.c_int]
        L.srz_kernel_time_samples.argtypes = [vp, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.srz_sync.argtypes = [vp]
        L.srz_debug_counters.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
        L.srz_verify_fastmath.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.srz_verify_fastdiv.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.srz_verify_fastpow.argtypes = [vp, C.c_float, C.POINTER(C.c_uint64)]
        L.srz_verify_fastlen.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.srz_host_register.argtypes = [vp, C.c_void_p, C.c_size_t]
        L.srz_host_unregister.argtypes = [vp, C.c_void_p]
        L.srz_frameset_debug_counters.argtypes = [vp, vp, C.POINTER(C.c_uint32)]
        L.srz_frameset_shade_kinds.argtypes = [vp, vp, C.POINTER(C.c_uint32)]
        L.srz_comm_unique_id.argtypes = [vp]
        L.srz_comm_create.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
        L.srz_comm_destroy.argtypes = [vp, vp]
        L.srz_comm_destroy.restype = None
        L.srz_frameset_exchange_bytes.argtypes = [vp, vp, C.c_int]
        L.srz_frameset_exchange_bytes.restype = C.c_size_t
        L.srz_frameset_allgather.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp]
        L.srz_frameset_deinterleave.argtypes = [vp, vp, vp, vp, C.c_int, vp]
        L.srz_frameset_allgather_inplace.argtypes = [vp, vp, vp, vp, C.c_int, vp]
        L.srz_frameset_gathered_row_offset.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.srz_frameset_gathered_row_offset.restype = C.c_size_t
        L.srz_frameset_read_gathered_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp]
        L.srz_frameset_sparse_capacity.argtypes = [vp, vp, C.c_int]
        L.srz_frameset_sparse_capacity.restype = C.c_size_t
        L.srz_frameset_sparse_pack.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_int, vp]
        L.srz_frameset_sparse_unpack.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_int, vp]
        L.srz_frameset_allgather_sparse.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_int, vp]
        L.srz_target_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
        L.srz_target_destroy.argtypes = [vp, vp]
        L.srz_target_destroy.restype = None
        L.srz_target_clear.argtypes = [vp, vp, C.c_int, C.c_int]
        L.srz_target_draw.argtypes = [vp, vp, C.c_int, vp, C.POINTER(abi.SrzStats)]
        L.srz_target_read.argtypes = [vp, vp, fp, fp, fp, fp]
        L.srz_target_read_bgr8.argtypes = [vp, vp, vp]
        _lib = L
    return _lib


def _stream(stream):
    """hipStream_t argument of the C ABI: None → NULL = the ctx's own non-blocking stream; 0 (HIP's null stream, e.g. torch's
    default stream) → SRZ_STREAM_NULL, because work on the ctx's stream is NOT ordered against the null stream."""
    if stream is None:
        return None
    return C.c_void_p(-1 if stream == 0 else stream)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def mip_levels(tex_w, tex_h):
    """the levels of the mip pyramid of a tex_w x tex_h texture, level 0 included: halving goes on while every extent is even or 1
    (include/srz.h); 0 for an extent of 0 or above abi.TEX_MAX_SIZE.  No GPU involved."""
    return int(lib().srz_texture_mip_levels(tex_w, tex_h))


def mip_bytes(tex_w, tex_h, n_ch, tex_frames, n_levels):
    """bytes of the levels 1 .. n_levels - 1, level-major, each [tex_frames][h_l][w_l][n_ch] float32; 0 for n_levels <= 1 or an
    argument out of range.  No GPU involved."""
    return int(lib().srz_texture_mip_bytes(tex_w, tex_h, n_ch, tex_frames, n_levels))


def cube_mip_levels(n):
    """the levels of the mip pyramid of a cube with n x n faces, level 0 included: mip_levels(n, n).  No GPU involved."""
    return int(lib().srz_cube_mip_levels(n))


def cube_mip_bytes(n, n_ch, tex_frames, n_levels):
    """bytes of the levels 1 .. n_levels - 1 of a cube's pyramid, level-major, each [tex_frames][6][n_l][n_l][n_ch] float32; 0 for
    n_levels <= 1 or an argument out of range (6 * tex_frames above 65536 among them).  No GPU involved."""
    return int(lib().srz_cube_mip_bytes(n, n_ch, tex_frames, n_levels))


class FrameSet:
    """Frames resident in HBM (srz_frameset_*)."""

    def __init__(self, ctx, frames):
        self.ctx, self.frames = ctx, list(frames)
        self.h = C.c_void_p()
        if isinstance(self.frames[0], abi.SceneFrame):  # meshes + matrices: vertex stage runs on the device
            arr = abi.scene_frames_array(self.frames)
            ctx._check(lib().srz_sceneset_create(ctx.h, arr, len(self.frames), C.byref(self.h)))
        else:
            arr = abi.frames_array(self.frames)
            ctx._check(lib().srz_frameset_create(ctx.h, arr, len(self.frames), C.byref(self.h)))
        self.n_frames = len(self.frames)
        self.width, self.height = self.frames[0].width, self.frames[0].height
        self.local_rows = lib().srz_frameset_local_rows(ctx.h, self.h)
        self.out_bytes = lib().srz_frameset_out_bytes(ctx.h, self.h)

    @property
    def out_shape(self):
        return (self.n_frames, 4, self.local_rows, self.width)

    def render(self, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """d_out_ptr: integer device address (e.g. torch_tensor.data_ptr()). Asynchronous."""
        self.ctx._check(lib().srz_frameset_render(self.ctx.h, self.h, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def render_visibility(self, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """the visibility buffer instead of the colour: planes z, id = triangle index in the frame + 1 | S class << 31 (0 = nobody),
        alpha, beta (include/srz.h; srz.visibility.decode takes it apart).  Same buffer and arguments as render().  Asynchronous."""
        self.ctx._check(lib().srz_frameset_render_visibility(self.ctx.h, self.h, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def peel_visibility(self, d_prev_ptr, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """depth peeling: the layer behind the visibility buffer at d_prev_ptr (layer k of this set, from render_visibility or from this
        call) into d_out_ptr, same layout — per pixel the first fragment strictly after d_prev's in the renders' visibility order, or
        nobody (include/srz.h states the rule).  Every pixel's four words are written; the buffers may not overlap.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_peel_visibility(self.ctx.h, self.h, C.c_void_p(d_prev_ptr), C.c_void_p(d_out_ptr), out_bytes,
                                                           flags, _stream(stream)))

    def shade_visibility(self, d_vis_ptr, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """the colour of a visibility buffer of this set (render_visibility) with the set's current shading data: equal bit for bit to
        render() of the same frames.  d_out_ptr may equal d_vis_ptr (in place); a partial overlap is an error.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_shade_visibility(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_out_ptr), out_bytes,
                                                            flags, _stream(stream)))

    def gbuffer_bytes(self, what=abi.GB_ALL):
        """bytes of the G-buffer of the groups in `what` (abi.GB_*); 0 for what == 0 or an unknown bit"""
        return int(lib().srz_frameset_gbuffer_bytes(self.ctx.h, self.h, what))

    def gbuffer_shape(self, what=abi.GB_ALL):
        """[frame][plane][local_rows][width] of 4-byte words, the planes of srz.visibility.gbuffer_planes(what)"""
        from .visibility import gbuffer_planes
        return (self.n_frames, len(gbuffer_planes(what)), self.local_rows, self.width)

    def gbuffer(self, d_vis_ptr, d_out_ptr, out_bytes, what=abi.GB_ALL, flags=abi.FUSED_CLEAR, stream=None):
        """the attribute planes of a visibility buffer of this set (render_visibility): what the built-in shaders are handed for every
        pixel's owner, bit for bit — normal, uv, batch + 1, albedo (include/srz.h; srz.visibility.gbuffer_decode takes it apart).
        d_out_ptr may not overlap d_vis_ptr; pixels nobody owns are zeros with FUSED_CLEAR, else left untouched.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_gbuffer(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_out_ptr), out_bytes, what, flags,
                                                   _stream(stream)))

    def motion_bytes(self, what=abi.MV_ALL):
        """bytes of the motion buffer of the groups in `what` (abi.MV_*); 0 for what == 0 or an unknown bit"""
        return int(lib().srz_frameset_motion_bytes(self.ctx.h, self.h, what))

    def motion_shape(self, what=abi.MV_ALL):
        """[frame][plane][local_rows][width] of 4-byte words, the planes of srz.visibility.motion_planes(what)"""
        from .visibility import motion_planes
        return (self.n_frames, len(motion_planes(what)), self.local_rows, self.width)

    def motion(self, d_vis_ptr, d_out_ptr, out_bytes, what=abi.MV_ALL, delta=1, flags=abi.FUSED_CLEAR, stream=None):
        """where the surface point under each pixel of frame f of a visibility buffer of this set (render_visibility) lies in frame
        f + delta, triangle t there standing for triangle t here: flow dx, dy; the depth there; the raw id and z words of frame
        f + delta at the nearest sample (include/srz.h; srz.visibility.motion_decode takes it apart).  d_out_ptr may not overlap
        d_vis_ptr; pixels nobody owns, and every pixel of a frame without a target frame, are zeros with FUSED_CLEAR, else left
        untouched.  MV_TARGET needs an unsharded context.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_motion(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_out_ptr), out_bytes, what, delta,
                                                  flags, _stream(stream)))

    def interpolate_bytes(self, n_ch):
        """bytes of [frame][n_ch][local_rows][width] float32; 0 for n_ch == 0 or above abi.ATTR_MAX_CH"""
        return int(lib().srz_frameset_interpolate_bytes(self.ctx.h, self.h, n_ch))

    def interpolate_shape(self, n_ch):
        """[frame][channel][local_rows][width] float32"""
        return (self.n_frames, n_ch, self.local_rows, self.width)

    def interpolate(self, d_vis_ptr, d_attr_ptr, n_ch, attr_frames, attr_tris, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """the caller's per-vertex attributes [attr_frames][attr_tris][3][n_ch] float32 (attr_frames: 1 or the frame count) under each
        pixel's barycentrics of a visibility buffer of this set, each channel interpolated as the owner's class interpolates uv
        (include/srz.h); pixels nobody owns are zeros with FUSED_CLEAR, else left untouched.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_interpolate(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_attr_ptr), n_ch, attr_frames,
                                                       attr_tris, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def interpolate_grad(self, d_vis_ptr, d_gout_ptr, d_attr_ptr, n_ch, attr_frames, attr_tris, d_gattr_ptr, d_gbary_ptr, flags=abi.FUSED_CLEAR,
                         stream=None):
        """the backward of interpolate: d_gout [frame][n_ch][local_rows][width] → ADDED into d_gattr (the attributes' shape; the order
        of the adds is unspecified: not bit-reproducible) and / or written to d_gbary [frame][2][local_rows][width] (the gradient with
        respect to alpha and beta; needs d_attr_ptr).  Either output pointer may be None / 0, not both.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_interpolate_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_gout_ptr),
                                                            C.c_void_p(d_attr_ptr or None), n_ch, attr_frames, attr_tris,
                                                            C.c_void_p(d_gattr_ptr or None), C.c_void_p(d_gbary_ptr or None), flags,
                                                            _stream(stream)))

    def position_grad(self, d_vis_ptr, d_gbary_ptr, d_gz_ptr, pos_tris, d_gpos_ptr, d_gpix_ptr, flags=abi.FUSED_CLEAR, stream=None):
        """the step behind interpolate_grad's d_gbary: d_gbary [frame][2][local_rows][width] (dalpha, dbeta) and / or d_gz
        [frame][1][local_rows][width] (the gradient of depth plane 0) → ADDED into d_gpos [n_frames][pos_tris][9] (ax ay z0 bx by z1 cx
        cy z2 per triangle; the order of the adds is unspecified: not bit-reproducible) and / or written to d_gpix
        [frame][2][local_rows][width] (the gradient with respect to the pixel's sample point).  Owners are held fixed; the positions
        are the set's own.  Either input and either output may be None / 0, not both.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_position_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_gbary_ptr or None),
                                                         C.c_void_p(d_gz_ptr or None), pos_tris, C.c_void_p(d_gpos_ptr or None),
                                                         C.c_void_p(d_gpix_ptr or None), flags, _stream(stream)))

    def positions(self, pos_tris, d_pos_ptr, pos_bytes, stream=None):
        """the set's own screen positions, as the rasteriser reads them: d_pos [n_frames][pos_tris][9] float32 (ax ay z0 bx by z1 cx cy
        z2 per triangle, the visibility buffer's triangle index; +0 behind a frame's last triangle), pos_tris at least every frame's
        triangle count.  A sceneset runs its vertex stage first.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_positions(self.ctx.h, self.h, pos_tris, C.c_void_p(d_pos_ptr), pos_bytes, _stream(stream)))

    def vertex_grad(self, mesh_id, d_gpos_ptr, pos_tris, d_gverts_ptr, d_gdraw_ptr, draw_stride, stream=None):
        """the backward of a sceneset's vertex stage for mesh slot mesh_id: d_gpos [n_frames][pos_tris][9] (position_grad's and
        antialias_grad's) → ADDED into d_gverts [n_frames][n_verts][3] (a gather: deterministic; elements no draw contributes to are
        left untouched) and / or d_gdraw [n_frames][draw_stride][18] (per draw of the slot: ndc_mvp's 16 gradients in its own order,
        zscale, zoffset; a sum in an unspecified order: not bit-reproducible).  Either output pointer may be None / 0, not both
        (include/srz.h states the rule).  Asynchronous."""
        self.ctx._check(lib().srz_sceneset_vertex_grad(self.ctx.h, self.h, mesh_id, C.c_void_p(d_gpos_ptr), pos_tris,
                                                       C.c_void_p(d_gverts_ptr or None), C.c_void_p(d_gdraw_ptr or None), draw_stride,
                                                       _stream(stream)))

    def corner_attr(self, mesh_id, d_attr_ptr, n_ch, attr_frames, d_out_ptr, pos_tris, stream=None):
        """per-vertex attributes of mesh slot mesh_id, d_attr [attr_frames][n_verts][n_ch] float32 (attr_frames 1 or the frame count),
        laid out as the set's triangle stream: corner k of every face of every draw of the slot in d_out [n_frames][pos_tris][3][n_ch]
        — interpolate's layout with attr_frames = n_frames.  Everything else in d_out is left untouched: one call per slot into one
        buffer.  A sceneset only.  Asynchronous."""
        self.ctx._check(lib().srz_sceneset_corner_attr(self.ctx.h, self.h, mesh_id, C.c_void_p(d_attr_ptr), n_ch, attr_frames,
                                                       C.c_void_p(d_out_ptr), pos_tris, _stream(stream)))

    def corner_attr_grad(self, mesh_id, d_gout_ptr, n_ch, d_gattr_ptr, pos_tris, stream=None):
        """the backward of corner_attr: d_gout [n_frames][pos_tris][3][n_ch] → d_gattr [n_frames][n_verts][n_ch], every element
        written: one running sum over the frame's draws of the slot in draw order and the vertex's corners in list order (a gather:
        deterministic; zeros for a frame that does not draw the slot).  Asynchronous."""
        self.ctx._check(lib().srz_sceneset_corner_attr_grad(self.ctx.h, self.h, mesh_id, C.c_void_p(d_gout_ptr), n_ch, C.c_void_p(d_gattr_ptr),
                                                            pos_tris, _stream(stream)))

    def antialias(self, d_vis_ptr, d_in_ptr, n_ch, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """the planes d_in [frame][n_ch][local_rows][width] float32 blended across the silhouettes of a visibility buffer of this set:
        where two 4-neighbours have different owners, the nearer owner's edge is intersected with the segment between the two
        sample points and the pixel it does not reach the middle of takes that share of the other's value (include/srz.h states the
        rule).  Every pixel of d_out is written, deterministic; d_out may overlap neither input.  Needs an unsharded context.
        Asynchronous."""
        self.ctx._check(lib().srz_frameset_antialias(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_in_ptr), n_ch, C.c_void_p(d_out_ptr),
                                                     out_bytes, flags, _stream(stream)))

    def antialias_grad(self, d_vis_ptr, d_in_ptr, d_gout_ptr, n_ch, d_gin_ptr, pos_tris, d_gpos_ptr, flags=abi.FUSED_CLEAR, stream=None):
        """the backward of antialias: d_gout and the forward's d_in, both [frame][n_ch][local_rows][width] → written to d_gin (the
        planes' shape, deterministic) and / or ADDED into d_gpos [n_frames][pos_tris][9] (ax ay z0 bx by z1 cx cy z2 per triangle: the
        silhouette term; the order of the adds is unspecified: not bit-reproducible; the z slots receive nothing).  Either output
        pointer may be None / 0, not both.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_antialias_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_in_ptr), C.c_void_p(d_gout_ptr),
                                                          n_ch, C.c_void_p(d_gin_ptr or None), pos_tris, C.c_void_p(d_gpos_ptr or None), flags,
                                                          _stream(stream)))

    def texture(self, d_vis_ptr, d_uv_ptr, d_tex_ptr, tex_w, tex_h, n_ch, tex_frames, mode, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR,
                stream=None):
        """the caller's float32 texture [tex_frames][tex_h][tex_w][n_ch] (tex_frames: 1 or the frame count) sampled bilinearly at the
        planes d_uv [frame][2][local_rows][width] (interpolate's of a two-channel attribute, or gbuffer(UV)) under a visibility
        buffer of this set → d_out [frame][n_ch][local_rows][width]; mode: abi.TEX_CLAMP or abi.TEX_WRAP (include/srz.h states the
        rule).  Pixels nobody owns are zeros with FUSED_CLEAR, else left untouched; an owner whose u or v is not finite gets zeros.
        Asynchronous."""
        self.ctx._check(lib().srz_frameset_texture(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_uv_ptr), C.c_void_p(d_tex_ptr), tex_w,
                                                   tex_h, n_ch, tex_frames, mode, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def texture_grad(self, d_vis_ptr, d_uv_ptr, d_gout_ptr, d_tex_ptr, tex_w, tex_h, n_ch, tex_frames, mode, d_gtex_ptr, d_guv_ptr,
                     flags=abi.FUSED_CLEAR, stream=None):
        """the backward of texture: d_gout [frame][n_ch][local_rows][width] → ADDED into d_gtex (the texture's shape; the order of the
        adds is unspecified: not bit-reproducible) and / or written to d_guv [frame][2][local_rows][width] (the gradient with respect
        to u and v, deterministic; needs d_tex_ptr; the layout interpolate_grad takes as d_gout at n_ch = 2).  Either output pointer
        may be None / 0, not both.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_texture_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_uv_ptr), C.c_void_p(d_gout_ptr),
                                                        C.c_void_p(d_tex_ptr or None), tex_w, tex_h, n_ch, tex_frames, mode,
                                                        C.c_void_p(d_gtex_ptr or None), C.c_void_p(d_guv_ptr or None), flags, _stream(stream)))

    def interpolate_deriv(self, d_vis_ptr, d_attr_ptr, n_ch, attr_frames, attr_tris, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """the screen-space derivatives of the attributes interpolate takes (n_ch <= abi.ATTR_MAX_CH // 2), from the set's own
        positions: d_out [frame][2 * n_ch][local_rows][width], interpolate_bytes(2 * n_ch) bytes, plane 2 ch d/dx and plane 2 ch + 1
        d/dy of channel ch per one-pixel step, constants of each pixel's owner (include/srz.h).  Nobody's pixels as interpolate.
        Asynchronous."""
        self.ctx._check(lib().srz_frameset_interpolate_deriv(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_attr_ptr), n_ch, attr_frames,
                                                             attr_tris, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def texture_mip(self, d_vis_ptr, d_uv_ptr, d_uvd_ptr, d_tex_ptr, tex_w, tex_h, n_ch, tex_frames, mode, d_mip_ptr, n_levels, d_out_ptr,
                    out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """texture() with a mip pyramid: the trilinear lookup over the n_levels levels of d_tex (level 0) and d_mip (Context.mip_build's
        levels 1 ..), the level of each pixel chosen from the derivative planes d_uvd [frame][4][local_rows][width] — ux, uy, vx, vy,
        interpolate_deriv's of the two-channel uv attribute (include/srz.h states the rule).  n_levels == 1: texture()'s output, d_uvd
        and d_mip may be None.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_texture_mip(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_uv_ptr), C.c_void_p(d_uvd_ptr or None),
                                                       C.c_void_p(d_tex_ptr), tex_w, tex_h, n_ch, tex_frames, mode, C.c_void_p(d_mip_ptr or None),
                                                       n_levels, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def texture_mip_grad(self, d_vis_ptr, d_uv_ptr, d_uvd_ptr, d_gout_ptr, d_tex_ptr, d_mip_ptr, tex_w, tex_h, n_ch, tex_frames, mode, n_levels,
                         d_gtex_ptr, d_gmip_ptr, d_guv_ptr, flags=abi.FUSED_CLEAR, stream=None):
        """the backward of texture_mip, the level held fixed: d_gout → ADDED into d_gtex (level 0) and d_gmip (the pyramid's layout; the
        two come together when n_levels > 1; float atomics: not bit-reproducible; Context.mip_fold then folds d_gmip into d_gtex) and /
        or written to d_guv [frame][2][local_rows][width] (deterministic; needs d_tex_ptr and d_mip_ptr).  Asynchronous."""
        self.ctx._check(lib().srz_frameset_texture_mip_grad(
            self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_uv_ptr), C.c_void_p(d_uvd_ptr or None), C.c_void_p(d_gout_ptr),
            C.c_void_p(d_tex_ptr or None), C.c_void_p(d_mip_ptr or None), tex_w, tex_h, n_ch, tex_frames, mode, n_levels,
            C.c_void_p(d_gtex_ptr or None), C.c_void_p(d_gmip_ptr or None), C.c_void_p(d_guv_ptr or None), flags, _stream(stream)))

    def texture_cube(self, d_vis_ptr, d_dir_ptr, d_tex_ptr, n, n_ch, tex_frames, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """the caller's float32 cube map [tex_frames][6][n][n][n_ch] (faces +X -X +Y -Y +Z -Z; tex_frames: 1 or the frame count) looked
        up bilinearly and seamlessly by the direction planes d_dir [frame][3][local_rows][width] (interpolate's of a three-channel
        attribute; any length) under a visibility buffer of this set → d_out [frame][n_ch][local_rows][width] (include/srz.h states
        the rule).  Pixels nobody owns are zeros with FUSED_CLEAR, else left untouched; an owner whose direction is not finite or
        zero gets zeros.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_texture_cube(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_dir_ptr), C.c_void_p(d_tex_ptr),
                                                        n, n_ch, tex_frames, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def texture_cube_grad(self, d_vis_ptr, d_dir_ptr, d_gout_ptr, d_tex_ptr, n, n_ch, tex_frames, d_gtex_ptr, d_gdir_ptr, flags=abi.FUSED_CLEAR,
                          stream=None):
        """the backward of texture_cube: d_gout [frame][n_ch][local_rows][width] → ADDED into d_gtex (the cube's shape; the order of
        the adds is unspecified: not bit-reproducible) and / or written to d_gdir [frame][3][local_rows][width] (the gradient with
        respect to the direction, deterministic; needs d_tex_ptr; the layout interpolate_grad takes as d_gout at n_ch = 3).  Either
        output pointer may be None / 0, not both.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_texture_cube_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_dir_ptr),
                                                             C.c_void_p(d_gout_ptr), C.c_void_p(d_tex_ptr or None), n, n_ch, tex_frames,
                                                             C.c_void_p(d_gtex_ptr or None), C.c_void_p(d_gdir_ptr or None), flags,
                                                             _stream(stream)))

    def background(self, d_vis_ptr, d_ray_ptr, ray_frames, d_tex_ptr, n, n_ch, tex_frames, where, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR,
                   stream=None):
        """the environment behind a visibility buffer of this set: at the pixels nobody owns (where = abi.BG_NOBODY) or at every pixel
        (abi.BG_ALL: d_vis_ptr may be None / 0 and is not read) the pixel's view ray r0 + x rx + y ry — the block d_ray
        [ray_frames][9]: r0[3] rx[3] ry[3]; ray_frames: 1 or the frame count — looked up in texture_cube's cube by texture_cube's
        rule → d_out [frame][n_ch][local_rows][width] (include/srz.h states the rule).  Owned pixels (BG_NOBODY) are zeros with
        FUSED_CLEAR, else left untouched; a pixel of the pass whose ray is not finite or zero gets zeros.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_background(self.ctx.h, self.h, C.c_void_p(d_vis_ptr or None), C.c_void_p(d_ray_ptr), ray_frames,
                                                      C.c_void_p(d_tex_ptr), n, n_ch, tex_frames, where, C.c_void_p(d_out_ptr), out_bytes, flags,
                                                      _stream(stream)))

    def background_work_bytes(self):
        """bytes of the scratch buffer background_grad needs for d_gray"""
        return int(lib().srz_frameset_background_work_bytes(self.ctx.h, self.h))

    def background_grad(self, d_vis_ptr, d_ray_ptr, ray_frames, d_gout_ptr, d_tex_ptr, n, n_ch, tex_frames, where, d_gtex_ptr, d_gray_ptr,
                        d_work_ptr, work_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """the backward of background: d_gout [frame][n_ch][local_rows][width] → ADDED into d_gtex (the cube's shape; the order of the
        adds is unspecified: not bit-reproducible) and / or WRITTEN to d_gray [ray_frames][9] (the gradient of the ray block, summed
        in a fixed tree: bit-reproducible; needs d_tex_ptr and d_work of background_work_bytes() bytes).  Either output pointer may be
        None / 0, not both.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_background_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr or None), C.c_void_p(d_ray_ptr), ray_frames,
                                                           C.c_void_p(d_gout_ptr), C.c_void_p(d_tex_ptr or None), n, n_ch, tex_frames, where,
                                                           C.c_void_p(d_gtex_ptr or None), C.c_void_p(d_gray_ptr or None),
                                                           C.c_void_p(d_work_ptr or None), work_bytes, flags, _stream(stream)))

    def texture_cube_mip(self, d_vis_ptr, d_dir_ptr, d_lam_ptr, d_tex_ptr, n, n_ch, tex_frames, d_mip_ptr, n_levels, d_out_ptr, out_bytes,
                         flags=abi.FUSED_CLEAR, stream=None):
        """texture_cube() over a mip pyramid of the cube: the lookup blended between the two levels around the per-pixel level of
        detail d_lam [frame][1][local_rows][width] (the caller's: a roughness, or cube_level's footprint level), over the n_levels
        levels of d_tex (level 0) and d_mip (Context.cube_mip_build's pyramid, or the caller's own in that layout) → d_out
        [frame][n_ch][local_rows][width] (include/srz.h states the rule).  n_levels == 1 is texture_cube itself (d_lam_ptr and
        d_mip_ptr may be None).  Asynchronous."""
        self.ctx._check(lib().srz_frameset_texture_cube_mip(
            self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_dir_ptr), C.c_void_p(d_lam_ptr or None), C.c_void_p(d_tex_ptr), n, n_ch,
            tex_frames, C.c_void_p(d_mip_ptr or None), n_levels, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def texture_cube_mip_grad(self, d_vis_ptr, d_dir_ptr, d_lam_ptr, d_gout_ptr, d_tex_ptr, d_mip_ptr, n, n_ch, tex_frames, n_levels,
                              d_gtex_ptr, d_gmip_ptr, d_gdir_ptr, d_glam_ptr, flags=abi.FUSED_CLEAR, stream=None):
        """the backward of texture_cube_mip: d_gout → ADDED into d_gtex (level 0) and d_gmip (the pyramid's layout; the two come
        together when n_levels > 1; float atomics: not bit-reproducible; Context.cube_mip_fold then folds d_gmip into d_gtex for a
        box-built pyramid) and / or written to d_gdir [frame][3][local_rows][width] and d_glam [frame][1][local_rows][width] (the
        gradients with respect to the direction and to the level, deterministic; they need d_tex_ptr and, at n_levels > 1,
        d_mip_ptr).  Output pointers may be None / 0, not all.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_texture_cube_mip_grad(
            self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_dir_ptr), C.c_void_p(d_lam_ptr or None), C.c_void_p(d_gout_ptr),
            C.c_void_p(d_tex_ptr or None), C.c_void_p(d_mip_ptr or None), n, n_ch, tex_frames, n_levels, C.c_void_p(d_gtex_ptr or None),
            C.c_void_p(d_gmip_ptr or None), C.c_void_p(d_gdir_ptr or None), C.c_void_p(d_glam_ptr or None), flags, _stream(stream)))

    def cube_level(self, d_vis_ptr, d_dir_ptr, d_dird_ptr, n, n_levels, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """the level of detail of a cube lookup from its screen-space footprint: the direction planes d_dir and their derivative planes
        d_dird [frame][6][local_rows][width] (interpolate_deriv's at n_ch = 3) for a cube of n x n faces with n_levels levels → the
        plane d_out [frame][1][local_rows][width] texture_cube_mip takes as d_lam (include/srz.h states the rule).  Asynchronous."""
        self.ctx._check(lib().srz_frameset_cube_level(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_dir_ptr), C.c_void_p(d_dird_ptr),
                                                      n, n_levels, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def shadow(self, d_vis_ptr, d_sc_ptr, d_map_ptr, map_w, map_h, map_frames, bias, width, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR,
               stream=None):
        """percentage-closer filtering of the caller's float32 depth map [map_frames][map_h][map_w] (map_frames: 1 or the frame count;
        whole, never band-sharded) at the coordinate planes d_sc [frame][3][local_rows][width] — sx, sy in map texels with the texel
        centres on the integers, sd in the map's depth units: interpolate's of a three-channel attribute — under a visibility buffer
        of this (the camera's) set → d_out [frame][1][local_rows][width], 1 lit .. 0 shadowed (include/srz.h states the rule).
        bias, width: finite floats, width >= 0; 0 is the hard test, above it a linear ramp of that width in depth.  Pixels nobody owns
        are zeros with FUSED_CLEAR, else left untouched; an owner whose coordinates are not finite gets 1.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_shadow(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_sc_ptr), C.c_void_p(d_map_ptr), map_w,
                                                  map_h, map_frames, bias, width, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def shadow_grad(self, d_vis_ptr, d_sc_ptr, d_gout_ptr, d_map_ptr, map_w, map_h, map_frames, bias, width, d_gmap_ptr, d_gsc_ptr,
                    flags=abi.FUSED_CLEAR, stream=None):
        """the backward of shadow: d_gout [frame][1][local_rows][width] → ADDED into d_gmap (the map's shape; only corners on the ramp
        add, none with width == 0; the order of the adds is unspecified: not bit-reproducible) and / or written to d_gsc
        [frame][3][local_rows][width] (the gradient with respect to sx, sy, sd, deterministic; the layout interpolate_grad takes as
        d_gout at n_ch = 3).  Either output pointer may be None / 0, not both.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_shadow_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_sc_ptr), C.c_void_p(d_gout_ptr),
                                                       C.c_void_p(d_map_ptr), map_w, map_h, map_frames, bias, width,
                                                       C.c_void_p(d_gmap_ptr or None), C.c_void_p(d_gsc_ptr or None), flags, _stream(stream)))

    def perspective(self, d_vis_ptr, d_q_ptr, q_frames, q_tris, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """a visibility buffer of this set with its screen-linear alpha, beta rewritten into the PERSPECTIVE-CORRECT alpha', beta', from
        d_q [q_frames][q_tris][3] float32, the reciprocal clip w of every triangle's corners (q_frames: 1 or the frame count;
        corner_attr's layout at one channel) → d_out, a buffer of the same four-plane layout, every word written (z, the ids and
        nobody's pixels copied; a pixel whose q or denominator is not a positive normal float keeps alpha, beta: include/srz.h states
        the rule).  interpolate, interpolate_grad, gbuffer and shade_visibility take d_out and are then perspective-correct;
        position_grad, motion, antialias, peel_visibility and interpolate_deriv keep taking the ORIGINAL buffer.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_perspective(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_q_ptr), q_frames, q_tris,
                                                       C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def perspective_grad(self, d_vis_ptr, d_q_ptr, q_frames, q_tris, d_gbary_p_ptr, d_gbary_ptr, d_gq_ptr, flags=abi.FUSED_CLEAR, stream=None):
        """the backward of perspective: d_gbary_p [frame][2][local_rows][width], the gradient with respect to alpha', beta'
        (interpolate_grad's d_gbary on the perspective buffer), with the ORIGINAL buffer d_vis and the same d_q → written to d_gbary
        (the gradient with respect to the screen-linear alpha, beta: what position_grad takes with the ORIGINAL buffer;
        deterministic) and / or ADDED into d_gq (d_q's shape; the order of the adds is unspecified: not bit-reproducible).  Either
        output pointer may be None / 0, not both.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_perspective_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_q_ptr), q_frames, q_tris,
                                                            C.c_void_p(d_gbary_p_ptr), C.c_void_p(d_gbary_ptr or None),
                                                            C.c_void_p(d_gq_ptr or None), flags, _stream(stream)))

    def interpolate_deriv_persp(self, d_vis_ptr, d_q_ptr, q_frames, q_tris, d_attr_ptr, n_ch, attr_frames, attr_tris, d_out_ptr, out_bytes,
                                flags=abi.FUSED_CLEAR, stream=None):
        """interpolate_deriv under the perspective-correct interpolation: the per-pixel screen-space derivatives of the attributes, from
        the ORIGINAL buffer d_vis, d_q as perspective takes it and the set's own positions → d_out
        [frame][2 * n_ch][local_rows][width] (include/srz.h states the rule; where it does not apply, interpolate_deriv's words).
        Asynchronous."""
        self.ctx._check(lib().srz_frameset_interpolate_deriv_persp(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_q_ptr), q_frames,
                                                                   q_tris, C.c_void_p(d_attr_ptr), n_ch, attr_frames, attr_tris,
                                                                   C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def light(self, d_vis_ptr, d_nrm_ptr, d_pos_ptr, d_kd_ptr, d_par_ptr, n_lights, par_frames, p, d_out_ptr, out_bytes,
              flags=abi.FUSED_CLEAR, stream=None):
        """Blinn-Phong under n_lights point lights for the caller's planes d_nrm, d_pos, d_kd (None / 0: albedo ones), each
        [frame][3][local_rows][width], and the parameter block d_par [par_frames][abi.light_par(n_lights)] (eye ka ks, then per light
        pos intensity; par_frames: 1 or the frame count) with the integer exponent p in 1 .. 256 → d_out [frame][3][local_rows][width],
        unclamped (include/srz.h states the rule).  Pixels nobody owns are zeros with FUSED_CLEAR, else left untouched; an owner whose
        normal has no finite positive length gets zeros.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_light(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_nrm_ptr), C.c_void_p(d_pos_ptr),
                                                 C.c_void_p(d_kd_ptr or None), C.c_void_p(d_par_ptr), n_lights, par_frames, p,
                                                 C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def light_work_bytes(self, n_lights):
        """bytes of the scratch buffer light_grad needs for d_gpar; 0 for n_lights == 0 or above abi.LIGHT_MAX"""
        return int(lib().srz_frameset_light_work_bytes(self.ctx.h, self.h, n_lights))

    def light_grad(self, d_vis_ptr, d_nrm_ptr, d_pos_ptr, d_kd_ptr, d_par_ptr, n_lights, par_frames, p, d_gout_ptr, d_gnrm_ptr, d_gpos_ptr,
                   d_gkd_ptr, d_gpar_ptr, d_work_ptr, work_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """the backward of light: d_gout [frame][3][local_rows][width] → written to d_gnrm, d_gpos, d_gkd (the planes' shape,
        deterministic) and / or d_gpar (d_par's shape: WRITTEN, reduced in a fixed tree, bit-reproducible for a shard layout; needs
        d_work of light_work_bytes(n_lights) bytes).  Every output pointer may be None / 0, not all; d_gkd needs d_kd.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_light_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_nrm_ptr), C.c_void_p(d_pos_ptr),
                                                      C.c_void_p(d_kd_ptr or None), C.c_void_p(d_par_ptr), n_lights, par_frames, p,
                                                      C.c_void_p(d_gout_ptr), C.c_void_p(d_gnrm_ptr or None), C.c_void_p(d_gpos_ptr or None),
                                                      C.c_void_p(d_gkd_ptr or None), C.c_void_p(d_gpar_ptr or None),
                                                      C.c_void_p(d_work_ptr or None), work_bytes, flags, _stream(stream)))

    def sh(self, d_vis_ptr, d_nrm_ptr, d_sh_ptr, n_ch, sh_frames, kind, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """nine order-2 spherical-harmonic coefficients per channel d_sh [sh_frames][9][n_ch] (sh_frames: 1 or the frame count; 1 <=
        n_ch <= abi.SH_MAX_CH) evaluated at the caller's normal planes d_nrm [frame][3][local_rows][width] → d_out
        [frame][n_ch][local_rows][width], unclamped: the irradiance over pi (kind abi.SH_IRRADIANCE, ibl's `irr`) or the function
        itself (abi.SH_RADIANCE) (include/srz.h states the rule).  Pixels nobody owns are zeros with FUSED_CLEAR, else left untouched;
        an owner whose normal has no finite positive length gets zeros.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_sh(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_nrm_ptr), C.c_void_p(d_sh_ptr), n_ch,
                                              sh_frames, kind, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def sh_work_bytes(self, n_ch):
        """bytes of the scratch buffer sh_grad needs for d_gsh; 0 for n_ch == 0 or above abi.SH_MAX_CH"""
        return int(lib().srz_frameset_sh_work_bytes(self.ctx.h, self.h, n_ch))

    def sh_grad(self, d_vis_ptr, d_nrm_ptr, d_sh_ptr, n_ch, sh_frames, kind, d_gout_ptr, d_gnrm_ptr, d_gsh_ptr, d_work_ptr, work_bytes,
                flags=abi.FUSED_CLEAR, stream=None):
        """the backward of sh: d_gout [frame][n_ch][local_rows][width] → written to d_gnrm (three planes, deterministic) and / or d_gsh
        (d_sh's shape: WRITTEN, reduced in a fixed tree, bit-reproducible for a shard layout; needs d_work of sh_work_bytes(n_ch)
        bytes).  Each output pointer may be None / 0, not both.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_sh_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_nrm_ptr), C.c_void_p(d_sh_ptr), n_ch,
                                                   sh_frames, kind, C.c_void_p(d_gout_ptr), C.c_void_p(d_gnrm_ptr or None),
                                                   C.c_void_p(d_gsh_ptr or None), C.c_void_p(d_work_ptr or None), work_bytes, flags,
                                                   _stream(stream)))

    def microfacet(self, d_vis_ptr, d_nrm_ptr, d_pos_ptr, d_base_ptr, d_mat_ptr, d_par_ptr, n_lights, par_frames, d_out_ptr, out_bytes,
                   flags=abi.FUSED_CLEAR, stream=None):
        """Cook-Torrance (GGX, Schlick-Smith, Schlick Fresnel; metallic-roughness) under n_lights point lights for the caller's planes
        d_nrm, d_pos, d_base (None / 0: base colour ones), each [frame][3][local_rows][width], the material d_mat
        [frame][2][local_rows][width] (roughness, metallic) and the parameter block d_par [par_frames][abi.microfacet_par(n_lights)]
        (eye amb, then per light pos intensity; par_frames: 1 or the frame count) → d_out [frame][3][local_rows][width], unclamped
        (include/srz.h states the rule).  Pixels nobody owns are zeros with FUSED_CLEAR, else left untouched; an owner whose normal has
        no finite positive length gets zeros.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_microfacet(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_nrm_ptr), C.c_void_p(d_pos_ptr),
                                                      C.c_void_p(d_base_ptr or None), C.c_void_p(d_mat_ptr), C.c_void_p(d_par_ptr), n_lights,
                                                      par_frames, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def microfacet_work_bytes(self, n_lights):
        """bytes of the scratch buffer microfacet_grad needs for d_gpar; 0 for n_lights == 0 or above abi.LIGHT_MAX"""
        return int(lib().srz_frameset_microfacet_work_bytes(self.ctx.h, self.h, n_lights))

    def microfacet_grad(self, d_vis_ptr, d_nrm_ptr, d_pos_ptr, d_base_ptr, d_mat_ptr, d_par_ptr, n_lights, par_frames, d_gout_ptr, d_gnrm_ptr,
                        d_gpos_ptr, d_gbase_ptr, d_gmat_ptr, d_gpar_ptr, d_work_ptr, work_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """the backward of microfacet: d_gout [frame][3][local_rows][width] → written to d_gnrm, d_gpos, d_gbase (three planes), d_gmat
        (two planes: roughness, metallic; 0 where a clamp holds), all deterministic, and / or d_gpar (d_par's shape: WRITTEN, reduced
        in a fixed tree, bit-reproducible for a shard layout; needs d_work of microfacet_work_bytes(n_lights) bytes).  Every output
        pointer may be None / 0, not all; d_gbase needs d_base.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_microfacet_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_nrm_ptr),
                                                           C.c_void_p(d_pos_ptr), C.c_void_p(d_base_ptr or None), C.c_void_p(d_mat_ptr),
                                                           C.c_void_p(d_par_ptr), n_lights, par_frames, C.c_void_p(d_gout_ptr),
                                                           C.c_void_p(d_gnrm_ptr or None), C.c_void_p(d_gpos_ptr or None),
                                                           C.c_void_p(d_gbase_ptr or None), C.c_void_p(d_gmat_ptr or None),
                                                           C.c_void_p(d_gpar_ptr or None), C.c_void_p(d_work_ptr or None), work_bytes, flags,
                                                           _stream(stream)))

    def reflect(self, d_vis_ptr, d_nrm_ptr, d_pos_ptr, d_eye_ptr, par_frames, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """the reflection of the view direction about the normal, and n.v: the caller's planes d_nrm, d_pos
        [frame][3][local_rows][width] and the eye d_eye [par_frames][3] on the device (par_frames: 1 or the frame count) → d_out
        [frame][4][local_rows][width]: R = 2 (N.Vd) N - Vd, then the RAW N.Vd (include/srz.h states the rule).  An owner without a
        lit normal or a view gets four zeros: texture_cube's "unsampled".  Asynchronous."""
        self.ctx._check(lib().srz_frameset_reflect(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_nrm_ptr), C.c_void_p(d_pos_ptr),
                                                   C.c_void_p(d_eye_ptr), par_frames, C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def reflect_grad(self, d_vis_ptr, d_nrm_ptr, d_pos_ptr, d_eye_ptr, par_frames, d_gout_ptr, d_gnrm_ptr, d_gpos_ptr, flags=abi.FUSED_CLEAR,
                     stream=None):
        """the backward of reflect: d_gout [frame][4][local_rows][width] → written to d_gnrm and / or d_gpos (three planes; one may be
        None / 0), per pixel, deterministic.  The eye's gradient is minus the sum of a frame's d_gpos.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_reflect_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_nrm_ptr), C.c_void_p(d_pos_ptr),
                                                        C.c_void_p(d_eye_ptr), par_frames, C.c_void_p(d_gout_ptr), C.c_void_p(d_gnrm_ptr or None),
                                                        C.c_void_p(d_gpos_ptr or None), flags, _stream(stream)))

    def ibl(self, d_vis_ptr, d_base_ptr, d_mat_ptr, d_nv_ptr, d_irr_ptr, d_spec_ptr, d_tab_ptr, n, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR,
            stream=None):
        """the split-sum combine: d_base (None / 0: ones), d_irr, d_spec [frame][3][local_rows][width], d_mat [frame][2][..] (roughness,
        metallic), d_nv [frame][1][..] and Context.brdf_table's d_tab [n][n][2] → d_out [frame][3][..] = cdif irr + spec (F0 A + B),
        unclamped (include/srz.h states the rule).  Asynchronous."""
        self.ctx._check(lib().srz_frameset_ibl(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_base_ptr or None), C.c_void_p(d_mat_ptr),
                                               C.c_void_p(d_nv_ptr), C.c_void_p(d_irr_ptr), C.c_void_p(d_spec_ptr), C.c_void_p(d_tab_ptr), n,
                                               C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def ibl_grad(self, d_vis_ptr, d_base_ptr, d_mat_ptr, d_nv_ptr, d_irr_ptr, d_spec_ptr, d_tab_ptr, n, d_gout_ptr, d_gbase_ptr, d_gmat_ptr,
                 d_gnv_ptr, d_girr_ptr, d_gspec_ptr, d_gtab_ptr, flags=abi.FUSED_CLEAR, stream=None):
        """the backward of ibl: d_gout [frame][3][local_rows][width] → written to d_gbase, d_girr, d_gspec (three planes), d_gmat (two),
        d_gnv (one), all per pixel and deterministic, and / or ADDED INTO d_gtab [n][n][2] (float adds: within texture_grad's bound).
        Every output pointer may be None / 0, not all; d_gbase needs d_base.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_ibl_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_base_ptr or None),
                                                    C.c_void_p(d_mat_ptr), C.c_void_p(d_nv_ptr), C.c_void_p(d_irr_ptr), C.c_void_p(d_spec_ptr),
                                                    C.c_void_p(d_tab_ptr), n, C.c_void_p(d_gout_ptr), C.c_void_p(d_gbase_ptr or None),
                                                    C.c_void_p(d_gmat_ptr or None), C.c_void_p(d_gnv_ptr or None),
                                                    C.c_void_p(d_girr_ptr or None), C.c_void_p(d_gspec_ptr or None),
                                                    C.c_void_p(d_gtab_ptr or None), flags, _stream(stream)))

    def normal_map(self, d_vis_ptr, d_nrm_ptr, d_tan_ptr, d_m_ptr, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """tangent-space normal mapping of the caller's planes: d_nrm [frame][3][local_rows][width] (the interpolated normal), d_tan
        [frame][4][...] (the interpolated tangent and handedness of Context.mesh_tangents) and d_m [frame][3][...] (the tangent-space
        normal as the caller decoded it) → d_out [frame][3][...], the unit shading normal light and texture_cube take (include/srz.h
        states the rule).  Pixels nobody owns are zeros with FUSED_CLEAR, else left untouched; an owner whose normal has no finite
        positive length gets zeros, one without a tangent frame the unperturbed unit normal.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_normal_map(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_nrm_ptr), C.c_void_p(d_tan_ptr),
                                                      C.c_void_p(d_m_ptr), C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def normal_map_grad(self, d_vis_ptr, d_nrm_ptr, d_tan_ptr, d_m_ptr, d_gout_ptr, d_gnrm_ptr, d_gtan_ptr, d_gm_ptr, flags=abi.FUSED_CLEAR,
                        stream=None):
        """the backward of normal_map: d_gout [frame][3][local_rows][width] → written to d_gnrm, d_gm (three planes) and d_gtan (four
        planes, the w plane +0), per pixel, deterministic.  Every output pointer may be None / 0, not all.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_normal_map_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_nrm_ptr),
                                                           C.c_void_p(d_tan_ptr), C.c_void_p(d_m_ptr), C.c_void_p(d_gout_ptr),
                                                           C.c_void_p(d_gnrm_ptr or None), C.c_void_p(d_gtan_ptr or None),
                                                           C.c_void_p(d_gm_ptr or None), flags, _stream(stream)))

    def composite(self, layers, n_ch, d_bg_ptr, want_through, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR, stream=None):
        """depth layers composited front to back in one pass: layers is a sequence, nearest first, of (d_vis_ptr, d_color_ptr,
        d_alpha_ptr or None, opacity) — a visibility buffer of this set, its colours [frame][n_ch][local_rows][width] and its alpha
        plane [frame][1][...] or, with None, the scalar opacity; d_bg_ptr (None / 0: nothing) is [frame][n_ch][...] behind everything
        → d_out [frame][n_ch + want_through][...], the last plane the transmittance if asked for (include/srz.h states the rule).  A
        layer that does not cover a pixel is skipped; every pixel is written.  Asynchronous."""
        arr = abi.composite_layers_array(list(layers))
        self.ctx._check(lib().srz_frameset_composite(self.ctx.h, self.h, arr, len(layers), n_ch, C.c_void_p(d_bg_ptr or None), int(want_through),
                                                     C.c_void_p(d_out_ptr), out_bytes, flags, _stream(stream)))

    def composite_grad(self, layers, n_ch, d_bg_ptr, want_through, d_gout_ptr, d_gcolor_ptrs, d_galpha_ptrs, d_gbg_ptr, flags=abi.FUSED_CLEAR,
                       stream=None):
        """the backward of composite: d_gout [frame][n_ch + want_through][local_rows][width] → written to d_gcolor_ptrs[k] (layer k's
        colour shape), d_galpha_ptrs[k] (one plane, also for a scalar opacity) and d_gbg_ptr (d_bg's shape); the two sequences are None
        or one entry per layer, every entry and d_gbg_ptr may be None / 0, not all.  +0 where the layer does not cover the pixel; per
        pixel, deterministic.  Asynchronous."""
        layers = list(layers)
        arr = abi.composite_layers_array(layers)

        def ptrs(seq):
            if seq is None:
                return None
            seq = list(seq)
            if len(seq) != len(layers):
                raise ValueError(f"composite_grad: {len(seq)} gradient pointers for {len(layers)} layers")
            return (C.c_void_p * max(1, len(seq)))(*[p or None for p in seq])
        self.ctx._check(lib().srz_frameset_composite_grad(self.ctx.h, self.h, arr, len(layers), n_ch, C.c_void_p(d_bg_ptr or None),
                                                          int(want_through), C.c_void_p(d_gout_ptr), ptrs(d_gcolor_ptrs), ptrs(d_galpha_ptrs),
                                                          C.c_void_p(d_gbg_ptr or None), flags, _stream(stream)))

    def texture_set(self, d_vis_ptr, d_uv_ptr, slots, d_batch_slot_ptr, n_batch_slot, n_ch, d_out_ptr, out_bytes, flags=abi.FUSED_CLEAR,
                    stream=None):
        """texture() with the texture of each pixel picked by its owner's batch: slots is a sequence of 1 .. abi.TEXSET_MAX tuples
        (d_tex_ptr, d_gtex_ptr (unused here: None), tex_w, tex_h, tex_frames, mode), each a texture [tex_frames][tex_h][tex_w][n_ch] as
        texture() takes it; d_batch_slot_ptr is DEVICE memory of n_batch_slot bytes, batch (a sceneset: draw) → slot, one map for
        every frame.  A pixel whose batch lies beyond the map or whose byte names no slot (abi.TEXSET_NONE) gets zeros, like one
        whose uv is not finite → d_out [frame][n_ch][local_rows][width] (include/srz.h states the rule).  Asynchronous."""
        slots = list(slots)
        arr = abi.texset_slots_array(slots)
        self.ctx._check(lib().srz_frameset_texture_set(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_uv_ptr), arr, len(slots),
                                                       C.c_void_p(d_batch_slot_ptr), n_batch_slot, n_ch, C.c_void_p(d_out_ptr), out_bytes,
                                                       flags, _stream(stream)))

    def texture_set_grad(self, d_vis_ptr, d_uv_ptr, d_gout_ptr, slots, d_batch_slot_ptr, n_batch_slot, n_ch, d_guv_ptr, flags=abi.FUSED_CLEAR,
                         stream=None):
        """the backward of texture_set: d_gout [frame][n_ch][local_rows][width] → ADDED into every slot's d_gtex_ptr that is not None
        (that slot's texture shape; float atomics: not bit-reproducible) and / or written to d_guv [frame][2][local_rows][width]
        (deterministic; needs every slot's d_tex_ptr).  d_guv_ptr may be None / 0 if some slot asks for its gradient.  Asynchronous."""
        slots = list(slots)
        arr = abi.texset_slots_array(slots)
        self.ctx._check(lib().srz_frameset_texture_set_grad(self.ctx.h, self.h, C.c_void_p(d_vis_ptr), C.c_void_p(d_uv_ptr),
                                                            C.c_void_p(d_gout_ptr), arr, len(slots), C.c_void_p(d_batch_slot_ptr),
                                                            n_batch_slot, n_ch, C.c_void_p(d_guv_ptr or None), flags, _stream(stream)))

    def update_shading(self, frames):
        """new eye, ka, ks, p, kh, kn, lights, flags and batch shaders / textures for a set made from abi.Frame's, triangles untouched
        (same frame count, size, light counts, batch counts and triangles per batch).  Ordered on the context's own stream."""
        frames = list(frames)
        arr = abi.frames_array(frames)
        self.ctx._check(lib().srz_frameset_update_shading(self.ctx.h, self.h, arr, len(frames)))
        self.frames = frames

    def resolve8(self, d_planes_ptr, d_bgr8_ptr, bgr8_bytes, stream=None):
        """display()'s 8-bit resolve on the device: planes (render output) → [frame][rows][W][3] uint8."""
        self.ctx._check(lib().srz_frameset_resolve8(self.ctx.h, self.h, C.c_void_p(d_planes_ptr), C.c_void_p(d_bgr8_ptr), bgr8_bytes,
                                                    _stream(stream)))

    def debug_counters(self):
        """(tests) what the last render left: {slow_tiles, redo_tiles, pool_sub_cap, pool_demand, clear_wgs, clear_tuned}; waits for the device"""
        out = (C.c_uint32 * 6)()
        self.ctx._check(lib().srz_frameset_debug_counters(self.ctx.h, self.h, out))
        return dict(zip(("slow_tiles", "redo_tiles", "pool_sub_cap", "pool_demand", "clear_wgs", "clear_tuned"), (int(x) for x in out)))

    def shade_kinds(self):
        """(tests) (mask, any_generic): bit k of mask = some frame is shaded by FAST build kind k at the next render / shade,
        any_generic = some frame takes the generic build (srz_frameset_shade_kinds); launches nothing"""
        out = (C.c_uint32 * 2)()
        self.ctx._check(lib().srz_frameset_shade_kinds(self.ctx.h, self.h, out))
        return int(out[0]), bool(out[1])

    def exchange_bytes(self, what=abi.EXCHANGE_PLANES):
        return int(lib().srz_frameset_exchange_bytes(self.ctx.h, self.h, what))

    def allgather(self, comm, d_shard_ptr, d_gathered_ptr, d_full_ptr, what=abi.EXCHANGE_PLANES, stream=None):
        """RCCL all-gather of this rank's shard + de-interleave into row-major frames (srz_frameset_allgather)."""
        self.ctx._check(lib().srz_frameset_allgather(self.ctx.h, comm.h, self.h, C.c_void_p(d_shard_ptr), C.c_void_p(d_gathered_ptr),
                                                     C.c_void_p(d_full_ptr), what, _stream(stream)))

    def allgather_inplace(self, comm, d_gathered_ptr, what=abi.EXCHANGE_PLANES, stream=None):
        """the exchange without a second pass: this rank's shard was rendered at d_gathered + rank * exchange_bytes; ONE in-place
        RCCL all-gather fills in the others.  Layout: [rank][frame][plane][bands_per_rank*32][row] (gathered_row_offset)"""
        self.ctx._check(lib().srz_frameset_allgather_inplace(self.ctx.h, comm.h, self.h, C.c_void_p(d_gathered_ptr), what, _stream(stream)))

    def gathered_row_offset(self, frame, plane, row, what=abi.EXCHANGE_PLANES):
        """byte offset of row `row` of (frame, plane) in a rank-major gathered buffer; IndexError for a frame / plane / row /
        exchange kind the set does not have (the C call returns (size_t)-1 there: never add THAT to a device pointer)"""
        off = int(lib().srz_frameset_gathered_row_offset(self.ctx.h, self.h, what, frame, plane, row))
        if off == 2 ** 64 - 1:
            raise IndexError(f"gathered_row_offset: frame {frame} / plane {plane} / row {row} / kind {what} out of range")
        return off

    def read_gathered_frame(self, d_gathered_ptr, frame, what=abi.EXCHANGE_PLANES, stream=None):
        """one frame of a gathered buffer as row-major host planes ([4,H,W] float32, or [H,W,3] uint8), de-interleaved by the
        device→host copies"""
        out = np.empty((4, self.height, self.width), np.float32) if what == abi.EXCHANGE_PLANES else np.empty((self.height, self.width, 3), np.uint8)
        self.ctx._check(lib().srz_frameset_read_gathered_frame(self.ctx.h, self.h, C.c_void_p(d_gathered_ptr), what, frame,
                                                                out.ctypes.data_as(C.c_void_p), _stream(stream)))
        return out

    def deinterleave(self, d_gathered_ptr, d_full_ptr, what=abi.EXCHANGE_PLANES, stream=None):
        self.ctx._check(lib().srz_frameset_deinterleave(self.ctx.h, self.h, C.c_void_p(d_gathered_ptr), C.c_void_p(d_full_ptr), what,
                                                        _stream(stream)))

    def sparse_capacity(self, what=abi.EXCHANGE_PLANES):
        """bytes of this rank's largest tile-sparse message (every tile touched): the size of the message buffer"""
        return int(lib().srz_frameset_sparse_capacity(self.ctx.h, self.h, what))

    def sparse_pack(self, d_shard_ptr, d_msg_ptr, msg_bytes, what=abi.EXCHANGE_PLANES, stream=None):
        """this rank's tile-sparse message from its shard (format: include/srz.h); enqueue it after the render, before the set's
        next render.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_sparse_pack(self.ctx.h, self.h, C.c_void_p(d_shard_ptr), C.c_void_p(d_msg_ptr), msg_bytes, what,
                                                       _stream(stream)))

    def sparse_unpack(self, d_recv_ptr, msg_stride, d_gathered_ptr, what=abi.EXCHANGE_PLANES, stream=None):
        """every other rank's shard of a rank-major gathered buffer from its message at d_recv + rank * msg_stride.  Asynchronous."""
        self.ctx._check(lib().srz_frameset_sparse_unpack(self.ctx.h, self.h, C.c_void_p(d_recv_ptr), msg_stride, C.c_void_p(d_gathered_ptr),
                                                         what, _stream(stream)))

    def allgather_sparse(self, comm, d_msg_ptr, d_recv_ptr, recv_bytes, d_gathered_ptr, what=abi.EXCHANGE_PLANES, stream=None):
        """the tile-sparse exchange over RCCL (sizes all-gather, one host synchronisation, padded all-gather of the messages,
        unpack): the same result as allgather_inplace.  SrzError SRZ_E_NOMEM on EVERY rank when some rank's recv_bytes is short."""
        self.ctx._check(lib().srz_frameset_allgather_sparse(self.ctx.h, comm.h, self.h, C.c_void_p(d_msg_ptr), C.c_void_p(d_recv_ptr), recv_bytes,
                                                            C.c_void_p(d_gathered_ptr), what, _stream(stream)))

    def stats(self):
        st = abi.SrzStats()
        self.ctx._check(lib().srz_frameset_stats(self.ctx.h, self.h, C.byref(st)))
        return st.as_dict()

    def algorithmic_bytes(self):
        return int(lib().srz_frameset_algorithmic_bytes(self.ctx.h, self.h))

    def close(self):
        if self.h:
            lib().srz_frameset_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Target:
    """A framebuffer resident in HBM (srz_target_*): z and three colour planes that stay on the device between draws.  It starts
    cleared (z = +inf, colour 0).  A thin handle: what the planes hold, and when a clear takes place, is the library's business."""

    def __init__(self, ctx, width, height):
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        self.h = C.c_void_p()
        ctx._check(lib().srz_target_create(ctx.h, self.width, self.height, C.byref(self.h)))

    def clear(self, color=True, depth=True):
        """RenderingPipeline::clear(Buffers): colour planes to 0 and / or z to +inf"""
        self.ctx._check(lib().srz_target_clear(self.ctx.h, self.h, 1 if color else 0, 1 if depth else 0))

    def draw(self, frameset, primitive=abi.PRIMITIVE_TRIANGLES, want_stats=False):
        """frame 0 of a 1-frame set of the target's size (FrameSet of abi.Frame's or abi.SceneFrame's), drawn onto what the target
        holds; asynchronous on the context's own stream unless want_stats.  -> the counters' dict, or None"""
        st = abi.SrzStats()
        self.ctx._check(lib().srz_target_draw(self.ctx.h, self.h, primitive, frameset.h, C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def read(self, planes=(True, True, True, True)):
        """(z, c0, c1, c2) as [height, width] float32 arrays.  An entry of `planes` that is False skips that plane (NULL is passed, None
        comes back); an entry that is a float32 array of the target's shape is read into."""
        out = []
        for p in planes:
            if isinstance(p, np.ndarray):
                assert p.dtype == np.float32 and p.shape == (self.height, self.width) and p.flags.c_contiguous
                out.append(p)
            else:
                out.append(np.empty((self.height, self.width), np.float32) if p else None)
        self.ctx._check(lib().srz_target_read(self.ctx.h, self.h, *[None if a is None else _fp(a) for a in out]))
        return tuple(out)

    def read_bgr8(self):
        """display()'s 8-bit resolve of the colour planes: [height, width, 3] uint8"""
        out = np.empty((self.height, self.width, 3), np.uint8)
        self.ctx._check(lib().srz_target_read_bgr8(self.ctx.h, self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        if self.h:
            lib().srz_target_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """RCCL communicator of the band exchange (srz_comm_*): rank 0 makes the id, the host program distributes it."""

    def __init__(self, ctx, id128, rank, world):
        self.ctx, self.h = ctx, C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(id128))
        ctx._check(lib().srz_comm_create(ctx.h, buf, rank, world, C.byref(self.h)))
        self.rank, self.world = rank, world

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        rc = lib().srz_comm_unique_id(buf)
        if rc != 0:
            raise SrzError(rc, lib().srz_last_error(None).decode())
        return bytes(buf)

    def close(self):
        if self.h:
            lib().srz_comm_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


class Context:
    """One ctx per process / GPU (srz_create)."""

    def __init__(self, device_id=0, rank=0, world=1):
        self.h = C.c_void_p()
        self.mesh_sizes = {}  # slot -> (vertices, faces) of the mesh uploaded last
        rc = lib().srz_create(C.byref(self.h), device_id)
        if rc != 0:
            raise SrzError(rc, lib().srz_last_error(None).decode())
        if world != 1:
            self.set_shard(rank, world)

    def _check(self, rc):
        if rc != 0:
            raise SrzError(rc, lib().srz_last_error(self.h).decode())

    def set_shard(self, rank, world):
        self._check(lib().srz_set_shard(self.h, rank, world))

    def set_option(self, option, value):
        """per-ctx switches for framesets created afterwards (abi.OPT_POOL_LAZY)"""
        self._check(lib().srz_set_option(self.h, option, int(value)))

    def texture_upload(self, tex_id, bgr):
        a = np.ascontiguousarray(bgr, dtype=np.uint8)
        h, w, c = a.shape
        assert c == 3
        self._check(lib().srz_texture_upload(self.h, tex_id, a.ctypes.data, w, h, w * 3))

    def mip_build(self, d_tex_ptr, tex_w, tex_h, n_ch, tex_frames, n_levels, d_mip_ptr, mip_bytes, stream=None):
        """the levels 1 .. n_levels - 1 of the float32 texture [tex_frames][tex_h][tex_w][n_ch] at d_tex_ptr → d_mip_ptr (srz.mip_bytes
        bytes, level-major), each level the box filter of the level above it, deterministic (include/srz.h).  n_levels == 1 launches
        nothing.  Asynchronous."""
        self._check(lib().srz_texture_mip_build(self.h, C.c_void_p(d_tex_ptr), tex_w, tex_h, n_ch, tex_frames, n_levels, C.c_void_p(d_mip_ptr),
                                                mip_bytes, _stream(stream)))

    def mip_fold(self, d_gmip_ptr, mip_bytes, tex_w, tex_h, n_ch, tex_frames, n_levels, d_gtex_ptr, stream=None):
        """the backward of mip_build: the gradient pyramid at d_gmip_ptr folded into the level-0 gradient at d_gtex_ptr (added into, one
        fma per element; a gather, deterministic).  Asynchronous."""
        self._check(lib().srz_texture_mip_fold(self.h, C.c_void_p(d_gmip_ptr), mip_bytes, tex_w, tex_h, n_ch, tex_frames, n_levels,
                                               C.c_void_p(d_gtex_ptr), _stream(stream)))

    def cube_mip_build(self, d_tex_ptr, n, n_ch, tex_frames, n_levels, d_mip_ptr, mip_bytes, stream=None):
        """the levels 1 .. n_levels - 1 of the float32 cube [tex_frames][6][n][n][n_ch] at d_tex_ptr → d_mip_ptr (srz.cube_mip_bytes
        bytes, level-major), every face box-filtered on its own: mip_build on the cube as 6 * tex_frames textures.  Asynchronous."""
        self._check(lib().srz_cube_mip_build(self.h, C.c_void_p(d_tex_ptr), n, n_ch, tex_frames, n_levels, C.c_void_p(d_mip_ptr), mip_bytes,
                                             _stream(stream)))

    def cube_mip_fold(self, d_gmip_ptr, mip_bytes, n, n_ch, tex_frames, n_levels, d_gtex_ptr, stream=None):
        """the backward of cube_mip_build: the gradient pyramid at d_gmip_ptr folded into the level-0 gradient at d_gtex_ptr (mip_fold
        on the cube as 6 * tex_frames textures; deterministic).  Asynchronous."""
        self._check(lib().srz_cube_mip_fold(self.h, C.c_void_p(d_gmip_ptr), mip_bytes, n, n_ch, tex_frames, n_levels, C.c_void_p(d_gtex_ptr),
                                            _stream(stream)))

    def cube_prefilter_work_bytes(self, n_src, n_dst, n_ch, tex_frames):
        """bytes of the scratch cube_prefilter and cube_prefilter_grad take for these sizes (0: a size out of range)"""
        return int(lib().srz_cube_prefilter_work_bytes(n_src, n_dst, n_ch, tex_frames))

    def cube_prefilter(self, d_src_ptr, n_src, d_dst_ptr, n_dst, n_ch, tex_frames, kind, roughness, cmin, d_den_ptr, d_work_ptr, work_bytes,
                       stream=None):
        """the float32 cube [tex_frames][6][n_src][n_src][n_ch] at d_src_ptr convolved with the cosine lobe (abi.PREFILTER_COSINE) or
        the GGX lobe at `roughness` (abi.PREFILTER_GGX) over the pairs with a cosine above cmin → the cube of n_dst x n_dst faces at
        d_dst_ptr and (d_den_ptr not None / 0) the normaliser [6][n_dst][n_dst]; d_work_ptr: cube_prefilter_work_bytes bytes of
        scratch.  Deterministic, no atomics (include/srz.h states the rule).  Asynchronous."""
        self._check(lib().srz_cube_prefilter(self.h, C.c_void_p(d_src_ptr), n_src, C.c_void_p(d_dst_ptr), n_dst, n_ch, tex_frames, kind, roughness,
                                             cmin, C.c_void_p(d_den_ptr), C.c_void_p(d_work_ptr), work_bytes, _stream(stream)))

    def cube_prefilter_grad(self, d_gdst_ptr, d_den_ptr, n_src, n_dst, n_ch, tex_frames, kind, roughness, cmin, d_gsrc_ptr, d_work_ptr, work_bytes,
                            stream=None):
        """the backward of cube_prefilter, its exact transpose as a gather: d_gdst_ptr and the normaliser the forward wrote →
        d_gsrc_ptr (written, not added into), deterministic.  Asynchronous."""
        self._check(lib().srz_cube_prefilter_grad(self.h, C.c_void_p(d_gdst_ptr), C.c_void_p(d_den_ptr), n_src, n_dst, n_ch, tex_frames, kind,
                                                  roughness, cmin, C.c_void_p(d_gsrc_ptr), C.c_void_p(d_work_ptr), work_bytes, _stream(stream)))

    def cube_sh_work_bytes(self, n, n_ch, tex_frames):
        """bytes of the scratch cube_sh and cube_sh_grad take for these sizes (0: a size out of range)"""
        return int(lib().srz_cube_sh_work_bytes(n, n_ch, tex_frames))

    def cube_sh(self, d_src_ptr, n, n_ch, tex_frames, d_sh_ptr, d_den_ptr, d_work_ptr, work_bytes, stream=None):
        """the float32 cube [tex_frames][6][n][n][n_ch] at d_src_ptr projected to its nine order-2 spherical-harmonic coefficients per
        channel → d_sh_ptr [tex_frames][9][n_ch] and (d_den_ptr not None / 0) the normaliser, one float; d_work_ptr: cube_sh_work_bytes
        bytes of scratch; 1 <= n_ch <= abi.SH_MAX_CH.  One O(n²) pass summed in a fixed tree: deterministic, no atomics (include/srz.h
        states the rule).  Asynchronous."""
        self._check(lib().srz_cube_sh(self.h, C.c_void_p(d_src_ptr), n, n_ch, tex_frames, C.c_void_p(d_sh_ptr), C.c_void_p(d_den_ptr or None),
                                      C.c_void_p(d_work_ptr), work_bytes, _stream(stream)))

    def cube_sh_grad(self, d_gsh_ptr, d_den_ptr, n, n_ch, tex_frames, d_gsrc_ptr, d_work_ptr, work_bytes, stream=None):
        """the backward of cube_sh, a gather per source texel: d_gsh_ptr [tex_frames][9][n_ch] and the normaliser the forward wrote →
        d_gsrc_ptr, the cube's shape (written, not added into), deterministic.  Asynchronous."""
        self._check(lib().srz_cube_sh_grad(self.h, C.c_void_p(d_gsh_ptr), C.c_void_p(d_den_ptr), n, n_ch, tex_frames, C.c_void_p(d_gsrc_ptr),
                                           C.c_void_p(d_work_ptr), work_bytes, _stream(stream)))

    def brdf_table(self, d_tab_ptr, tab_bytes, n, m, stream=None):
        """the split-sum table of FrameSet.microfacet's own specular lobe → d_tab [n][n][2] float32 (A, B; F0 A + B is the lobe's
        directional albedo), rows nv = i / (n - 1), columns roughness 1/16 + 15/16 j / (n - 1); m rings of 2 m samples, in a fixed
        order (include/srz.h states the quadrature): deterministic.  2 <= n <= abi.BRDF_TABLE_MAX, 1 <= m <= 256.  Asynchronous."""
        self._check(lib().srz_brdf_table(self.h, C.c_void_p(d_tab_ptr), tab_bytes, n, m, _stream(stream)))

    def mesh_upload(self, mesh_id, verts8, faces):
        """verts8: (nV,8) float32 [pos3 nrm3 uv2]; faces: (nF,3) uint32."""
        v = np.ascontiguousarray(verts8, dtype=np.float32)
        f = np.ascontiguousarray(faces, dtype=np.uint32)
        self._check(lib().srz_mesh_upload(self.h, mesh_id, v.ctypes.data, len(v), f.ctypes.data, len(f)))
        self.mesh_sizes[mesh_id] = (len(v), len(f))

    def mesh_update(self, mesh_id, d_verts_ptr, n_verts, stream=None):
        """new vertices for a slot that holds a mesh, in place: d_verts_ptr is a DEVICE address of n_verts (the slot's count) 32-byte
        records [pos3 nrm3 uv2] — one asynchronous device-to-device copy.  Faces, addresses and the upload counter stay: every
        sceneset that draws the slot stays valid and transforms the new vertices from its next vertex stage on."""
        self._check(lib().srz_mesh_update(self.h, mesh_id, C.c_void_p(d_verts_ptr), n_verts, _stream(stream)))

    def mesh_normals(self, mesh_id, d_pos_ptr, pos_stride, n_sets, d_nrm_ptr, nrm_stride, stream=None):
        """area-weighted vertex normals of slot mesh_id's faces for n_sets position sets on the device: vertex v of set s at float
        (s * n_verts + v) * stride of d_pos / d_nrm (strides >= 3).  d_pos_ptr None / 0: the slot's own vertices, d_nrm_ptr None / 0:
        the slot's own nrm fields (n_sets 1 either way); both: the slot refreshed in place.  A gather, deterministic (include/srz.h
        states the rule).  Asynchronous."""
        self._check(lib().srz_mesh_normals(self.h, mesh_id, C.c_void_p(d_pos_ptr or None), pos_stride, n_sets, C.c_void_p(d_nrm_ptr or None),
                                           nrm_stride, _stream(stream)))

    def mesh_normals_grad(self, mesh_id, d_pos_ptr, pos_stride, n_sets, d_gnrm_ptr, gnrm_stride, d_work_ptr, d_gpos_ptr, stream=None):
        """the backward of mesh_normals: d_gnrm (laid out like the normals, gnrm_stride >= 3) → d_gpos [n_sets][n_verts][3], every
        element written; d_work: a workspace of d_gpos's size.  Two gathers, deterministic.  Asynchronous."""
        self._check(lib().srz_mesh_normals_grad(self.h, mesh_id, C.c_void_p(d_pos_ptr or None), pos_stride, n_sets, C.c_void_p(d_gnrm_ptr or None),
                                                gnrm_stride, C.c_void_p(d_work_ptr or None), C.c_void_p(d_gpos_ptr or None), _stream(stream)))

    def mesh_tangents(self, mesh_id, d_pos_ptr, pos_stride, n_sets, d_uv_ptr, uv_stride, d_tan_ptr, tan_stride, stream=None):
        """uv-area-weighted vertex tangents (x, y, z) and handedness w = +-1 of slot mesh_id's faces for n_sets position sets and ONE
        uv set on the device: vertex v of set s at float (s * n_verts + v) * stride of d_pos (>= 3) / d_tan (>= 4), uv of v at float
        v * uv_stride (>= 2).  d_pos_ptr None / 0: the slot's own positions (n_sets 1), d_uv_ptr None / 0: the slot's own uv.  A
        gather, deterministic (include/srz.h states the rule).  Asynchronous."""
        self._check(lib().srz_mesh_tangents(self.h, mesh_id, C.c_void_p(d_pos_ptr or None), pos_stride, n_sets, C.c_void_p(d_uv_ptr or None),
                                            uv_stride, C.c_void_p(d_tan_ptr or None), tan_stride, _stream(stream)))

    def mesh_tangents_grad(self, mesh_id, d_pos_ptr, pos_stride, n_sets, d_uv_ptr, uv_stride, d_gtan_ptr, gtan_stride, d_work_ptr, d_gpos_ptr,
                           stream=None):
        """the backward of mesh_tangents to the positions: d_gtan (laid out like the tangents, gtan_stride >= 4, its w never read) →
        d_gpos [n_sets][n_verts][3], every element written; d_work: a workspace of d_gpos's size.  Two gathers, deterministic."""
        self._check(lib().srz_mesh_tangents_grad(self.h, mesh_id, C.c_void_p(d_pos_ptr or None), pos_stride, n_sets, C.c_void_p(d_uv_ptr or None),
                                                 uv_stride, C.c_void_p(d_gtan_ptr or None), gtan_stride, C.c_void_p(d_work_ptr or None),
                                                 C.c_void_p(d_gpos_ptr or None), _stream(stream)))

    def mesh_laplacian(self, mesh_id, d_x_ptr, x_stride, n_ch, n_sets, kind, d_wpos_ptr, wpos_stride, d_out_ptr, out_stride, stream=None):
        """the mesh Laplacian (kind: abi.LAP_UMBRELLA / LAP_GRAPH / LAP_COTAN) of slot mesh_id's connectivity over n_sets per-vertex
        fields of n_ch (1 .. 64) channels on the device: vertex v of set s at float (s * n_verts + v) * stride of d_x / d_out (strides
        >= n_ch).  d_x_ptr None / 0: the slot's own positions (n_ch 3, n_sets 1).  d_wpos_ptr: ONE position set (wpos_stride >= 3)
        COTAN makes its weights from, None / 0: the slot's own.  A gather, deterministic (include/srz.h states the rule).
        Asynchronous."""
        self._check(lib().srz_mesh_laplacian(self.h, mesh_id, C.c_void_p(d_x_ptr or None), x_stride, n_ch, n_sets, kind,
                                             C.c_void_p(d_wpos_ptr or None), wpos_stride, C.c_void_p(d_out_ptr or None), out_stride, _stream(stream)))

    def mesh_laplacian_grad(self, mesh_id, d_gout_ptr, gout_stride, n_ch, n_sets, kind, d_wpos_ptr, wpos_stride, d_gx_ptr, gx_stride,
                            stream=None):
        """the backward of mesh_laplacian, its exact transpose: d_gout (laid out like the output) → d_gx (laid out like x), every
        element written.  GRAPH and COTAN are symmetric: the forward's kernel and bits over d_gout.  A gather, deterministic, no
        workspace.  Asynchronous."""
        self._check(lib().srz_mesh_laplacian_grad(self.h, mesh_id, C.c_void_p(d_gout_ptr or None), gout_stride, n_ch, n_sets, kind,
                                                  C.c_void_p(d_wpos_ptr or None), wpos_stride, C.c_void_p(d_gx_ptr or None), gx_stride,
                                                  _stream(stream)))

    def mesh_edges(self, mesh_id, d_pos_ptr, pos_stride, n_sets, kind, d_out_ptr, out_stride, stream=None):
        """the per-(face, edge) terms (kind: abi.EDGE_COUNT / EDGE_LENGTH / EDGE_DIHEDRAL) of slot mesh_id over n_sets position sets
        on the device: for set s and face f three floats at float (s * n_faces + f) * out_stride of d_out (out_stride >= 3), edge j
        opposite corner j.  d_pos_ptr None / 0: the slot's own positions (n_sets 1).  COUNT: the number of faces on the edge
        (n_sets 1); LENGTH: the edge's length; DIHEDRAL: the sum over the faces across the edge of 1 - cos of the unit normals.  The
        adjacency is found from the slot's corner lists; a gather, deterministic (include/srz.h states the rules).  Asynchronous."""
        self._check(lib().srz_mesh_edges(self.h, mesh_id, C.c_void_p(d_pos_ptr or None), pos_stride, n_sets, kind, C.c_void_p(d_out_ptr or None),
                                         out_stride, _stream(stream)))

    def mesh_edges_grad(self, mesh_id, d_pos_ptr, pos_stride, n_sets, kind, d_gout_ptr, gout_stride, d_work_ptr, d_gpos_ptr, stream=None):
        """the backward of mesh_edges (LENGTH or DIHEDRAL; COUNT has none) to the positions: d_gout (laid out like the output) →
        d_gpos [n_sets][n_verts][3], every element written.  d_work: DIHEDRAL's workspace [n_sets][n_faces][3]; LENGTH takes None /
        0.  Gathers without atomics, deterministic.  Asynchronous."""
        self._check(lib().srz_mesh_edges_grad(self.h, mesh_id, C.c_void_p(d_pos_ptr or None), pos_stride, n_sets, kind,
                                              C.c_void_p(d_gout_ptr or None), gout_stride, C.c_void_p(d_work_ptr or None),
                                              C.c_void_p(d_gpos_ptr or None), _stream(stream)))

    def draw(self, frame, planes=None, primitive=abi.PRIMITIVE_TRIANGLES, want_stats=False):
        """TraditionalRasterizer::draw for one scene; planes (z,c0,c1,c2) are modified in place."""
        if planes is None:
            h, w = frame.height, frame.width
            planes = (np.full((h, w), np.inf, np.float32), np.zeros((h, w), np.float32), np.zeros((h, w), np.float32),
                      np.zeros((h, w), np.float32))
        z, c0, c1, c2 = planes
        st = abi.SrzStats()
        fn = lib().srz_draw_scene if isinstance(frame, abi.SceneFrame) else lib().srz_draw
        self._check(fn(self.h, primitive, C.byref(frame.c), _fp(z), _fp(c0), _fp(c1), _fp(c2),
                       C.byref(st) if want_stats else None))
        return planes, (st.as_dict() if want_stats else None)

    def draw_batch(self, frames, planes=None, primitive=abi.PRIMITIVE_TRIANGLES, want_stats=False):
        """srz_draw_batch: planes = float32 array [n, 4, H, W] (z, c0, c1, c2 per frame), modified in place."""
        n, h, w = len(frames), frames[0].height, frames[0].width
        if planes is None:
            planes = np.zeros((n, 4, h, w), np.float32)
            planes[:, 0] = np.inf
        assert planes.dtype == np.float32 and planes.shape == (n, 4, h, w) and planes.flags.c_contiguous
        ptrs = (lib().srz_draw_batch.argtypes[4]._type_ * n)(*[_fp(planes[i]) for i in range(n)])
        st = abi.SrzStats()
        self._check(lib().srz_draw_batch(self.h, primitive, abi.frames_array(frames), n, ptrs, C.byref(st) if want_stats else None))
        return planes, (st.as_dict() if want_stats else None)

    def host_register(self, array):
        """page-lock a numpy array's memory: srz_draw / srz_draw_batch then move planes inside it by DMA (srz_host_register)"""
        self._check(lib().srz_host_register(self.h, array.ctypes.data, array.nbytes))

    def host_unregister(self, array):
        self._check(lib().srz_host_unregister(self.h, array.ctypes.data))

    def frameset(self, frames):
        return FrameSet(self, frames)

    def target(self, width, height):
        return Target(self, width, height)

    def set_kernel_timing(self, on):
        """False/0: off; 1: whole launch set only (2 events per render); True/2: per-kernel groups as well (4 events)"""
        self._check(lib().srz_set_kernel_timing(self.h, 2 if on is True else int(on)))

    def kernel_time_ms(self, reset=True):
        ms, n = (C.c_double * 4)(), C.c_int()
        self._check(lib().srz_kernel_time_ms(self.h, 1 if reset else 0, ms, C.byref(n)))
        return {"bin_ms": ms[0], "raster_ms": ms[1], "shade_ms": ms[2], "total_ms": ms[3], "launches": n.value}

    def kernel_time_samples(self, cap=65536):
        """(per-render launch-set ms since the last reset, span ms from the first start to the last end); read it BEFORE
        kernel_time_ms(reset=True)"""
        out, n, span = (C.c_float * cap)(), C.c_int(), C.c_double()
        self._check(lib().srz_kernel_time_samples(self.h, out, cap, C.byref(n), C.byref(span)))
        return [float(out[i]) for i in range(n.value)], span.value

    def verify_fastmath(self):
        out = (C.c_uint64 * 4)()
        self._check(lib().srz_verify_fastmath(self.h, out))
        return [int(x) for x in out]

    def verify_fastdiv(self):
        out = (C.c_uint64 * 3)()
        self._check(lib().srz_verify_fastdiv(self.h, out))
        return [int(x) for x in out]

    def verify_fastpow(self, p):
        out = (C.c_uint64 * 4)()
        self._check(lib().srz_verify_fastpow(self.h, float(p), out))
        return [int(x) for x in out]

    def verify_fastlen(self):
        out = (C.c_uint64 * 5)()
        self._check(lib().srz_verify_fastlen(self.h, out))
        return [int(x) for x in out]

    def debug_counters(self):
        out = (C.c_uint64 * 32)()
        n = lib().srz_debug_counters(self.h, out, 32)
        return [int(out[i]) for i in range(n)]

    def sync(self):
        self._check(lib().srz_sync(self.h))

    def close(self):
        if self.h:
            lib().srz_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
