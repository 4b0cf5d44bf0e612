/*
 * srz.h — C ABI of the MI355X-native triangle rasterization + fragment-shading stage.
 *
 * This is the drop-in boundary for ONE path of Liupeter01/Software-Rasterizer:
 *     virtual void RenderingPipeline::draw(Primitive) = 0        (include/base/Render.hpp:84)
 *     void TraditionalRasterizer::draw(Primitive)                (src/Rasterizer.cpp:183-240)
 * The reference has no FFI; the seam is that C++ virtual.  Everything `draw` pulls from the
 * scene (post-MVP triangle stream, lights, eye, shader type, texture, Blinn-Phong constants)
 * is passed here as plain pointers and sizes; everything it writes (z-buffer + 3 planar float
 * colour planes, include/base/Render.hpp:250-257) comes back through plain pointers.
 *
 * Conventions (all entry points):
 *   - return 0 on success, negative SRZ_E_* on error; text via srz_last_error().
 *   - no exception crosses this boundary; the C++ host shim (software-rasterizer_amd/host)
 *     rethrows as std::runtime_error for draw() to keep the reference's convention
 *     (src/Rasterizer.cpp:185-189).
 *   - the caller owns every host pointer; the library copies in/out and keeps only device state.
 *   - one ctx per host thread, one GPU per ctx, one process per GPU (multi-GPU = one ctx per rank,
 *     bands of 32 rows dealt round-robin (each round of N rotated by five ranks) with srz_set_shard, reassembled by an RCCL all-gather).
 *   - there is NO CPU fallback: every compute entry point fails with SRZ_E_NODEVICE when no
 *     gfx950 device is usable.
 */
#ifndef SRZ_H_
#define SRZ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an entry point is added, a struct changes or an argument changes its meaning; every binding compares it
 * with srz_abi_version() when it loads the library and refuses a mismatch (srz/__init__.py: ImportError; libsrz_host.so:
 * std::runtime_error from the TraditionalRasterizer constructor).
 *   1  round 1
 *   2  srz_draw_batch, scenesets, targets
 *   3  `stream` arguments: NULL = the ctx's own stream, SRZ_STREAM_NULL = HIP's null stream (was: NULL = null stream);
 *      srz_comm_*, srz_frameset_allgather / _deinterleave / _exchange_bytes, srz_kernel_time_samples
 *   4  srz_frameset_allgather_inplace, srz_frameset_gathered_row_offset, srz_frameset_read_gathered_frame
 *   5  srz_set_option, srz_verify_fastpow; srz_frameset_gathered_row_offset returns (size_t)-1 for an unknown `what` too
 *   6  SRZ_OPT_APPROX_SHADE (the tolerance mode of the shaders); srz_frameset_resolve8 / _deinterleave / the bgr8 exchange take any width;
 *      the tile-list pool is sized by srz_frameset_create / srz_sceneset_create, the first srz_frameset_render no longer blocks
 *   7  srz_host_register / srz_host_unregister, SRZ_NO_Z_READBACK, srz_verify_fastlen, srz_frameset_debug_counters; srz_draw_batch reads one piece of the batch
 *      back while the next one renders
 *      (additive, same version: no existing signature, struct or meaning changed) the tile-sparse exchange srz_frameset_sparse_capacity /
 *      _sparse_pack / _sparse_unpack, srz_frameset_allgather_sparse
 *      (additive, same version) the visibility buffer srz_frameset_render_visibility
 *      (additive, same version) shading a visibility buffer srz_frameset_shade_visibility, new shading data for a frameset
 *      srz_frameset_update_shading
 *      (additive, same version) the diagnostic srz_frameset_shade_kinds
 *      (additive, same version) the G-buffer of a visibility buffer srz_frameset_gbuffer / srz_frameset_gbuffer_bytes, SRZ_GB_*
 *      (additive, same version) the motion pass between frames of a set srz_frameset_motion / srz_frameset_motion_bytes, SRZ_MV_*
 *      (additive, same version) caller attributes over a visibility buffer, with gradients srz_frameset_interpolate /
 *      srz_frameset_interpolate_bytes / srz_frameset_interpolate_grad, SRZ_ATTR_MAX_CH
 *      (additive, same version) position gradients of a visibility buffer srz_frameset_position_grad
 *      (additive, same version) silhouette antialiasing of a visibility buffer srz_frameset_antialias / srz_frameset_antialias_grad
 *      (additive, same version) caller textures over a visibility buffer, with gradients srz_frameset_texture /
 *      srz_frameset_texture_grad, SRZ_TEX_CLAMP, SRZ_TEX_WRAP, SRZ_TEX_MAX_SIZE
 *      (additive, same version) mipmapped texture sampling over a visibility buffer, with gradients srz_texture_mip_levels /
 *      srz_texture_mip_bytes / srz_texture_mip_build / srz_texture_mip_fold / srz_frameset_interpolate_deriv /
 *      srz_frameset_texture_mip / srz_frameset_texture_mip_grad, SRZ_TEX_MAX_LEVELS
 *      (additive, same version) depth peeling: the layer behind a visibility buffer srz_frameset_peel_visibility
 *      (additive, same version) vertex normals and per-vertex attributes on the device, with gradients srz_mesh_normals /
 *      srz_mesh_normals_grad / srz_sceneset_corner_attr / srz_sceneset_corner_attr_grad
 *      (additive, same version) cube-map lookup by direction over a visibility buffer, with gradients srz_frameset_texture_cube /
 *      srz_frameset_texture_cube_grad
 *      (additive, same version) Blinn-Phong lighting pass over a visibility buffer, with gradients srz_frameset_light /
 *      srz_frameset_light_grad / srz_frameset_light_work_bytes
 *      (additive, same version) shadow-map lookup over a visibility buffer, with gradients srz_frameset_shadow /
 *      srz_frameset_shadow_grad
 *      (additive, same version) mipmapped cube-map lookup by direction and level, with gradients srz_cube_mip_levels /
 *      srz_cube_mip_bytes / srz_cube_mip_build / srz_cube_mip_fold / srz_frameset_texture_cube_mip /
 *      srz_frameset_texture_cube_mip_grad / srz_frameset_cube_level
 *      (additive, same version) tangent-space normal mapping over a visibility buffer, with gradients srz_mesh_tangents /
 *      srz_mesh_tangents_grad / srz_frameset_normal_map / srz_frameset_normal_map_grad
 *      (additive, same version) Cook-Torrance GGX shading pass over a visibility buffer, with gradients srz_frameset_microfacet /
 *      srz_frameset_microfacet_grad / srz_frameset_microfacet_work_bytes, SRZ_MICROFACET_PAR
 *      (additive, same version) a cube prefiltered on the device with a cosine or a GGX lobe, with gradients srz_cube_prefilter /
 *      srz_cube_prefilter_grad / srz_cube_prefilter_work_bytes, SRZ_PREFILTER_COSINE, SRZ_PREFILTER_GGX
 *      (additive, same version) image-based lighting over a visibility buffer, with gradients srz_frameset_reflect /
 *      srz_frameset_reflect_grad / srz_brdf_table / srz_frameset_ibl / srz_frameset_ibl_grad, SRZ_BRDF_TABLE_MAX
 *      (additive, same version) the environment behind a visibility buffer, by view ray, with gradients srz_frameset_background /
 *      srz_frameset_background_work_bytes / srz_frameset_background_grad, SRZ_BG_NOBODY, SRZ_BG_ALL
 *      (additive, same version) compositing depth layers front to back, with gradients srz_frameset_composite /
 *      srz_frameset_composite_grad, srz_composite_layer, SRZ_COMPOSITE_MAX
 *      (additive, same version) texture sets: each pixel's caller texture picked by its owner's batch, with gradients
 *      srz_frameset_texture_set / srz_frameset_texture_set_grad, srz_texset_slot, SRZ_TEXSET_MAX, SRZ_TEXSET_NONE
 *      (additive, same version) SH9 lighting: a cube projected to nine spherical-harmonic coefficients per channel, and those
 *      evaluated at each pixel's normal, with gradients srz_cube_sh / srz_cube_sh_grad / srz_cube_sh_work_bytes / srz_frameset_sh /
 *      srz_frameset_sh_grad / srz_frameset_sh_work_bytes, SRZ_SH_MAX_CH, SRZ_SH_IRRADIANCE, SRZ_SH_RADIANCE
 *      (additive, same version) the mesh Laplacian over a slot's connectivity: umbrella, graph and cotangent, with gradients
 *      srz_mesh_laplacian / srz_mesh_laplacian_grad, SRZ_LAP_UMBRELLA, SRZ_LAP_GRAPH, SRZ_LAP_COTAN
 *      (additive, same version) the mesh edge terms over a slot's connectivity: edge count, edge length and normal consistency, with
 *      gradients srz_mesh_edges / srz_mesh_edges_grad, SRZ_EDGE_COUNT, SRZ_EDGE_LENGTH, SRZ_EDGE_DIHEDRAL
 */
#define SRZ_ABI_VERSION 7

/* error codes */
#define SRZ_OK 0
#define SRZ_E_INVALID (-1)  /* bad argument (null pointer, bad size, unknown shader, ...) */
#define SRZ_E_NODEVICE (-2) /* no usable HIP device / HIP runtime error */
#define SRZ_E_NOMEM (-3)    /* host or device allocation failed */
#define SRZ_E_TEXTURE (-4)  /* a TEXTURE/BUMP/DISPLACEMENT batch names a tex_id that was not uploaded */
#define SRZ_E_PRIMITIVE (-5) /* primitive type not supported (src/Rasterizer.cpp:185-189) */

/* = SoftRasterizer::SHADERS_TYPE (include/shader/Shader.hpp:32-38) */
#define SRZ_SHADER_NORMAL 0
#define SRZ_SHADER_TEXTURE 1
#define SRZ_SHADER_PHONG 2
#define SRZ_SHADER_DISPLACEMENT 3
#define SRZ_SHADER_BUMP 4

/* = SoftRasterizer::Primitive (include/base/Render.hpp:74) */
#define SRZ_PRIMITIVE_LINES 0
#define SRZ_PRIMITIVE_TRIANGLES 1

/* frame flags */
#define SRZ_EXACT_SPLIT 0u /* default: reproduce the reference's AVX-columns / scalar-tail split per (triangle,pixel) */
#define SRZ_UNIFIED 1u     /* every pixel uses the 8-wide ("AVX") semantics; NOT reference-exact, for A/B only */
#define SRZ_FUSED_CLEAR 2u /* treat z/colour as just cleared (clear(Color|Depth), src/Render.cpp:46-55): write-only framebuffer */
#define SRZ_NO_Z_READBACK 8u /* srz_draw / srz_draw_scene / srz_draw_batch only: the depth plane is not copied back to the host (the caller
                              * reads colour only: a quarter of the PCIe bytes less).  The caller's z buffer is then stale: use it
                              * with SRZ_FUSED_CLEAR frames, i.e. where the next draw does not start from it */
#define SRZ_ORDERED_RASTER 4u /* rasterise every tile with the reference's ordered triangle walk (src/Rasterizer.cpp:199-236)
                               * instead of the order-independent depth keys; same result bit for bit, slower; for A/B only */

/* Post-MVP triangle = payload of SoftRasterizer::Triangle that draw() consumes
 * (m_vertex/m_normal/m_texCoords, include/object/Triangle.hpp:88-93).  Screen-space x,y in pixels,
 * z remapped to [near,far] (src/Scene.cpp:937-947).  bbox, cull and binning are recomputed on device. */
typedef struct srz_tri {
  float pos[3][3];
  float nrm[3][3];
  float uv[3][2];
} srz_tri; /* 96 B */

/* = light_struct {position,intensity} (include/light/Light.hpp:8-45) */
typedef struct srz_light {
  float pos[3];
  float intensity[3];
} srz_light; /* 24 B */

/* One mesh's triangles with the shader bound to that mesh = one ObjTuple of
 * Scene::loadTriangleStream (include/scene/Scene.hpp:30-31). Batches are drawn in array order,
 * triangles in array order (src/Rasterizer.cpp:199-200). */
typedef struct srz_batch {
  int32_t shader;  /* SRZ_SHADER_* */
  int32_t tex_id;  /* texture slot (srz_texture_upload); ignored by NORMAL / PHONG */
  uint32_t n_tris;
  uint32_t _pad;
  const srz_tri *tris; /* host pointer, n_tris entries */
} srz_batch;

/* Everything one draw() of one scene pulls (src/Rasterizer.cpp:191-196) */
typedef struct srz_frame {
  int32_t width, height; /* RenderingPipeline::m_width/m_height */
  float eye[3];          /* Scene::loadEyeVec() (camera POSITION) */
  float ka[3], ks[3];    /* Shader::ka / ks statics (src/Shader.cpp:7-8) */
  float p;               /* Shader::p (src/Shader.cpp:10) */
  float kh, kn;          /* Shader::kh / kn (src/Shader.cpp:11-12), BUMP / DISPLACEMENT only */
  uint32_t n_lights;
  uint32_t n_batches;
  const srz_light *lights;
  const srz_batch *batches;
  uint32_t flags; /* SRZ_EXACT_SPLIT | SRZ_UNIFIED | SRZ_FUSED_CLEAR | SRZ_ORDERED_RASTER */
  uint32_t _pad;
} srz_frame;

/* Per-call counters (summed over the frames of the call). */
typedef struct srz_stats {
  uint64_t n_tris;      /* triangles submitted */
  uint64_t n_culled;    /* rejected by the backface test (src/Rasterizer.cpp:203-205) */
  uint64_t pixel_tests; /* sum of bbox areas of the surviving triangles */
  uint64_t fragments;   /* (triangle,pixel) pairs that pass the coverage test */
  uint64_t shaded;      /* of those, pairs that also pass the z-test in submission order (the reference's ordered walk;
                         * a call that asks for stats runs the ordered rasteriser once more on a scratch copy) */
  uint64_t visible;     /* pixels whose final owner is a triangle of this call */
  uint64_t visible_textured; /* of those, pixels whose owner's shader fetches the texture (B_tex of the roofline) */
} srz_stats;

/* ---- device vertex stage (= Scene::loadTriangleStream, src/Scene.cpp:903-964, run on the GPU) ------------------
 * Instead of post-MVP triangles the caller hands over meshes (uploaded once) and, per frame, one srz_mesh_draw per mesh:
 * the two matrices loadTriangleStream builds (:922-923) and the depth remap (:279-280).  Matrices are column-major
 * (glm layout, m[col*4+row]). */
typedef struct srz_vertex { /* = SoftRasterizer::Vertex {position, normal, texCoord} (include/object/Object.hpp:17-31) */
  float pos[3];
  float nrm[3];
  float uv[2];
} srz_vertex; /* 32 B */

typedef struct srz_mesh_draw {
  int32_t mesh_id;     /* srz_mesh_upload slot */
  int32_t shader;      /* SRZ_SHADER_* of the Shader bound to the mesh */
  int32_t tex_id;      /* texture slot, ignored by NORMAL / PHONG */
  int32_t _pad;
  float ndc_mvp[16];   /* m_ndcToScreenMatrix * m_projection * m_view * modelMatrix */
  float normal_m[16];  /* transpose(inverse(modelMatrix)) */
} srz_mesh_draw;

typedef struct srz_scene_frame {
  int32_t width, height;
  float eye[3], ka[3], ks[3];
  float p, kh, kn;
  float zscale, zoffset; /* (far-near)/2, (far+near)/2 */
  uint32_t n_lights, n_draws;
  const srz_light *lights;
  const srz_mesh_draw *draws; /* in mesh registration order = batch order */
  uint32_t flags, _pad;
} srz_scene_frame;

typedef struct srz_ctx srz_ctx;
typedef struct srz_frameset srz_frameset;

/* ---- lifetime ------------------------------------------------------------------------- */
int srz_abi_version(void);
/* device_id: HIP ordinal. Replaces the TraditionalRasterizer(w,h) construction of device state. */
int srz_create(srz_ctx **out, int device_id);
void srz_destroy(srz_ctx *ctx);
const char *srz_last_error(const srz_ctx *ctx); /* ctx may be NULL: last error of srz_create */

/* Per-ctx switches (value 0 / 1), applied to framesets created AFTERWARDS:
 *   SRZ_OPT_POOL_LAZY  1 = creating a set does NOT size its tile-list pool by a binning pass of its own (see srz_frameset_render:
 *                      bands whose lists do not fit take the ordered rasteriser until a later render has grown the pool).
 *                      Default 0, or 1 when the environment variable SRZ_POOL_LAZY is set — read ONCE, in srz_create. */
#define SRZ_OPT_POOL_LAZY 1
/*   SRZ_OPT_APPROX_SHADE  1 = TOLERANCE MODE of the fragment shaders (default 0 = exact: bit-identical to the CPU oracle).  The
 *                      reference's x86 path shades with approximate instructions — _mm256_rcp_ps (include/shader/Shader.hpp:131,
 *                      src/Tools.cpp:19, include/loader/TextureLoader.hpp:99, src/Rasterizer.cpp:111) and SVML _mm256_pow_ps
 *                      (include/shader/Shader.hpp:195); this switch gives the colour arithmetic the same class on gfx950 (v_rcp_f32 /
 *                      v_rsq_f32 / v_sqrt_f32 at 1 ulp, x^p = exp2(p log2 x)).  Depth, coverage and ownership stay bit-exact (the
 *                      rasteriser does not change); colours: 8-wide ("V") columns within 0.5 of the exact value on the 0..255 scale,
 *                      scalar-tail ("S") columns equal except where the value in front of the floor lies within 1e-3 of an integer
 *                      (tests/test_gpu_approx.py).  Frames with 1..4 lights and no BUMP / DISPLACEMENT batch take it; others stay exact. */
#define SRZ_OPT_APPROX_SHADE 2
int srz_set_option(srz_ctx *ctx, int option, int value);

/* Multi-GPU: this ctx owns the 32-row bands b of rank(b) == rank, at local band b / world.  THE BAND MAP:
 *     rank(b) = (b + band_rot(world) * (b / world)) % world,   band_rot(world) = 5, or 1 when 5 % world == 0
 * (integer division): every group of `world` consecutive bands hands one band to every rank, rotated by band_rot ranks per group.
 * Default (0,1) = whole frame. Affects srz_frameset_* only. */
int srz_set_shard(srz_ctx *ctx, int rank, int world);

/* ---- texture = TextureLoader's cv::Mat (BGR u8, row-major, top row first;
 *      src/TextureLoader.cpp:3-12).  row_stride in bytes. Slots 0..63. ------------------- */
int srz_texture_upload(srz_ctx *ctx, int tex_id, const uint8_t *bgr, int w, int h, int row_stride);

/* ---- mesh = Mesh::vertices + Mesh::faces (include/object/Mesh.hpp:52-57), slots 0..255; faces = 3 indices each ----
 * n_faces may be 0 (a draw of such a mesh draws nothing).  Uploading to a slot that holds a mesh waits for the ctx's own stream and
 * FREES the old buffers.  A sceneset keeps the addresses of the buffers its draws named when it was created, so once a slot it draws
 * is uploaded anew the set must be destroyed, or at least never rendered, shaded or passed to srz_frameset_stats again (every such
 * call runs the vertex stage over the freed buffers): srz_sceneset_update refuses it with SRZ_E_INVALID whatever the new mesh's
 * size, which is the one thing left to do with it besides srz_frameset_destroy.  Renders of the set still running on a stream of the
 * caller's must have finished before the upload.  srz_draw_scene handles all of this itself: it rebuilds its set.
 * The upload also builds, on the host by a counting sort, the slot's CORNER LISTS for srz_sceneset_vertex_grad's gather —
 * corner_off[n_verts + 1] and corners[3 * n_faces]: vertex v is named by the corners corners[corner_off[v] .. corner_off[v + 1]), each
 * 3 * face + k, in increasing order — and uploads them beside the faces; they are freed with the slot. */
int srz_mesh_upload(srz_ctx *ctx, int mesh_id, const srz_vertex *verts, uint32_t n_verts, const uint32_t *faces,
                    uint32_t n_faces);
/* NEW VERTICES for a slot that holds a mesh, IN PLACE, FROM DEVICE MEMORY: d_verts is a device pointer to n_verts 32-byte srz_vertex
 * records (a [n_verts][8] float32 array: the caller updates normals and uv as they see fit), 4-byte aligned; n_verts must equal the
 * slot's count.  ONE asynchronous device-to-device copy into the slot's existing vertex buffer on `stream` (NULL: the ctx's own
 * stream, SRZ_STREAM_NULL: HIP's null stream).  The face list, the corner lists, the buffers' addresses and the slot's upload
 * counter do not change: every sceneset that draws the slot stays valid — srz_sceneset_update goes on accepting it — and transforms
 * the new vertices from its next vertex stage on (the next render, srz_frameset_positions or pass that runs the stage).  Ordering
 * against renders and passes on other streams is the caller's, as for srz_sceneset_update; the tile-list pool follows the new demand
 * as it does after a matrix update.  SRZ_E_INVALID, nothing copied, for: a null ctx; a mesh_id outside 0..255 or a slot that holds no
 * mesh; a null or misaligned d_verts; n_verts other than the slot's count. */
int srz_mesh_update(srz_ctx *ctx, int mesh_id, const srz_vertex *d_verts, uint32_t n_verts, void *stream);
/* VERTEX NORMALS of a slot's faces FROM POSITIONS, ON THE DEVICE: area-weighted (the sum of the cross products of the faces that name
 * the vertex, normalised), for n_sets position sets over the slot's face list in one pass.  d_pos: n_sets sets of n_verts vertices,
 * vertex v of set s at float (s * n_verts + v) * pos_stride, pos_stride >= 3; d_nrm laid out the same way with nrm_stride.  A null
 * d_pos selects the slot's own vertices (stride 8; n_sets must be 1), a null d_nrm the slot's own nrm fields (stride 8; n_sets must
 * be 1): both null REFRESHES THE SLOT IN PLACE — what srz_mesh_update leaves to the caller, one call after it on the same stream.  A
 * caller's [V][8] record array works as d_pos = base, d_nrm = base + 3, both strides 8.
 * THE RULE, in float32, nothing fused, in this order.  cross(u, w) = (u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x);
 * dot3(a, b) = (a.x b.x + a.y b.y) + a.z b.z.  Per set and vertex v, with p the set's positions and list(v) the slot's corner list of
 * v, in list order (srz_mesh_upload):
 *   S = (+0, +0, +0);  for corner c in list(v):  (i0, i1, i2) = faces[c / 3];  N = cross(p[i1] - p[i0], p[i2] - p[i0]);  S = S + N
 *   len2 = dot3(S, S)
 *   len2 > 0 && len2 <= FLT_MAX:  r = 1.0f / sqrtf(len2);  n = S * r            (v is NORMALISED)
 *   otherwise:                    n = (+0, +0, +0)     (no face names v, degenerate faces only, a NaN, an overflow, an underflow)
 * N is taken in the face's OWN vertex order whichever corner asks: a face contributes the same bits to its three vertices.  The pass
 * is a GATHER — the one thread that owns (s, v) stores its three floats once — with no atomics: DETERMINISTIC, bit for bit.  The
 * other floats of a strided record are not touched.  THIS IS NOT THE LOADER'S RULE for files without normals (the last face that
 * names a vertex wins there, src/ObjLoader.cpp:166-186): a mesh loaded from such a file and refreshed changes its normals.
 * Asynchronous on `stream` (NULL: the ctx's own stream, SRZ_STREAM_NULL: HIP's null stream); order it against srz_mesh_update,
 * renders and passes as a render is ordered.  No input value makes the pass read or write outside its buffers.
 * SRZ_E_INVALID, nothing written and nothing launched, for: a null ctx; a mesh_id outside 0..255 or a slot that holds no mesh; n_sets
 * of 0 or above 65535; a stride below 3 (of a non-null buffer); a null d_pos or d_nrm with n_sets != 1; a pointer that is not 4-byte
 * aligned; normals whose span (first to last float reached) overlaps the positions' span — except the record form d_nrm == d_pos + 3
 * with equal strides >= 6, the slot's own layout. */
int srz_mesh_normals(srz_ctx *ctx, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, float *d_nrm,
                     uint32_t nrm_stride, void *stream);
/* THE BACKWARD of srz_mesh_normals.  d_pos, pos_stride, n_sets as above (the positions of the forward call; null: the slot's own);
 * d_gnrm: the gradient with respect to the normals, laid out like d_nrm with gnrm_stride >= 3; d_gpos: [n_sets][n_verts][3] float32,
 * the gradient with respect to the positions, EVERY element written; d_work: a workspace of the same size whose contents afterwards
 * are unspecified.  THE RULE, in float32, nothing fused, two phases (the second starts when the first has ended), both gathers:
 *   PHASE 1, per set and vertex v:  S, r, n as above;  g = d_gnrm[s][v]
 *     v normalised:  d = dot3(n, g);  gS[v] = (g - n * d) * r        (componentwise: (g.x - n.x * d) * r, ...)
 *     otherwise:     gS[v] = (+0, +0, +0)
 *   PHASE 2, per set and vertex v:  acc = (+0, +0, +0);  for corner c in list(v), in list order:
 *     (i0, i1, i2) = faces[c / 3];  a, b, c' = p[i0], p[i1], p[i2];  k = c % 3;  G = (gS[i0] + gS[i1]) + gS[i2]
 *     k == 0:  acc = acc + cross(b - c', G);   k == 1:  acc = acc + cross(c' - a, G);   k == 2:  acc = acc + cross(G, b - a)
 *     d_gpos[s][v] = acc
 * No atomics: DETERMINISTIC, bit for bit.  A vertex that was not normalised passes no gradient on (the forward is constant there).
 * Non-finite values propagate as IEEE has them.  Asynchronous on `stream`.
 * SRZ_E_INVALID, nothing written and nothing launched, for what srz_mesh_normals refuses of ctx, mesh_id, n_sets, d_pos and
 * pos_stride, and for: a null d_gnrm, d_work or d_gpos; gnrm_stride below 3; a pointer that is not 4-byte aligned; d_work or d_gpos
 * overlapping the positions' or d_gnrm's span, or each other. */
int srz_mesh_normals_grad(srz_ctx *ctx, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, const float *d_gnrm,
                          uint32_t gnrm_stride, float *d_work, float *d_gpos, void *stream);
/* VERTEX TANGENTS AND HANDEDNESS of a slot's faces FROM POSITIONS AND UV, ON THE DEVICE: srz_mesh_normals' sibling, for tangent-space
 * normal mapping (srz_frameset_normal_map).  d_pos, pos_stride, n_sets: as srz_mesh_normals (null: the slot's own positions, n_sets
 * must be 1).  d_uv: ONE uv set of n_verts entries shared by every position set, vertex v at float v * uv_stride, uv_stride >= 2; null
 * selects the slot's own uv (floats 6..7 of its records, stride 8).  d_tan: per set and vertex, at float (s * n_verts + v) * tan_stride,
 * tan_stride >= 4, FOUR floats: the unit tangent (x, y, z) and the handedness w = +-1 — a 4-channel attribute for
 * srz_sceneset_corner_attr.  There is no in-place record form: a vertex record has no tangent field, d_tan must not be null.
 * THE RULE, in float32, nothing fused, in this order, dot3 and the list order as srz_mesh_normals has them.  Per set and vertex v, with
 * p the set's positions:
 *   S = (+0, +0, +0);  D = +0;  for corner c in list(v):  (i0, i1, i2) = faces[c / 3]
 *     e1 = p[i1] - p[i0];  e2 = p[i2] - p[i0]
 *     du1 = uv[i1].u - uv[i0].u;  dv1 = uv[i1].v - uv[i0].v;  du2 = uv[i2].u - uv[i0].u;  dv2 = uv[i2].v - uv[i0].v
 *     det = du1 * dv2 - du2 * dv1
 *     Tf  = e1 * dv2 - e2 * dv1        (componentwise; = det * dP/du: a face weighs in by its uv area)
 *     s   = det < 0 ? -1 : +1
 *     S = S + s * Tf;   D = D + det
 *   len2 = dot3(S, S)
 *   len2 > 0 && len2 <= FLT_MAX:  r = 1.0f / sqrtf(len2);  t = S * r          (v is NORMALISED)
 *   otherwise:                    t = (+0, +0, +0)        (no face names v, all uv equal, a NaN, an overflow, an underflow)
 *   w = D < 0 ? -1 : +1
 * The face's terms are taken in the face's OWN vertex order whichever corner asks.  So t points along +u whether or not the uv are
 * mirrored, and with a normal N that follows the winding (srz_mesh_normals') w * cross(N, t) points along +v.  A gather, no atomics:
 * DETERMINISTIC, bit for bit.  The other floats of a strided record are not touched.  Asynchronous on `stream`.  No input value makes
 * the pass read or write outside its buffers.
 * SRZ_E_INVALID, nothing written and nothing launched, for what srz_mesh_normals refuses of ctx, mesh_id, n_sets, d_pos and pos_stride,
 * and for: uv_stride below 2 (of a non-null d_uv); a null d_tan; tan_stride below 4; a pointer that is not 4-byte aligned; tangents
 * whose span overlaps the positions' or the uv's span. */
int srz_mesh_tangents(srz_ctx *ctx, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, const float *d_uv,
                      uint32_t uv_stride, float *d_tan, uint32_t tan_stride, void *stream);
/* THE BACKWARD of srz_mesh_tangents, TO THE POSITIONS ONLY: uv, s and w are held fixed.  d_gtan: the gradient with respect to the
 * tangents, laid out like d_tan with gtan_stride >= 4; its w float is NEVER READ.  d_gpos: [n_sets][n_verts][3], EVERY element
 * written; d_work: a workspace of the same size whose contents afterwards are unspecified.  Two phases, both gathers:
 *   PHASE 1, per set and vertex v:  S, r, t as above;  g = d_gtan[s][v].xyz
 *     v normalised:  d = dot3(t, g);  gS[v] = (g - t * d) * r;     otherwise:  gS[v] = (+0, +0, +0)
 *   PHASE 2, per set and vertex v:  acc = (+0, +0, +0);  for corner c in list(v), in list order:
 *     (i0, i1, i2) = faces[c / 3];  dv1, dv2, s as above;  k = c % 3;  G = (gS[i0] + gS[i1]) + gS[i2]
 *     k == 0:  co = s * (dv1 - dv2);   k == 1:  co = s * dv2;   k == 2:  co = -(s * dv1);     acc = acc + G * co
 *     d_gpos[s][v] = acc
 * No atomics: DETERMINISTIC, bit for bit.  Non-finite values propagate as IEEE has them.  Asynchronous on `stream`.
 * SRZ_E_INVALID, nothing written and nothing launched, for what srz_mesh_tangents refuses of ctx, mesh_id, n_sets, d_pos, pos_stride,
 * d_uv and uv_stride, and for: a null d_gtan, d_work or d_gpos; gtan_stride below 4; a pointer that is not 4-byte aligned; d_work or
 * d_gpos overlapping the positions', the uv's or d_gtan's span, or each other. */
int srz_mesh_tangents_grad(srz_ctx *ctx, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, const float *d_uv,
                           uint32_t uv_stride, const float *d_gtan, uint32_t gtan_stride, float *d_work, float *d_gpos, void *stream);
/* THE MESH LAPLACIAN over a slot's connectivity, ON THE DEVICE: one linear operator in three kinds over per-vertex fields of 1 to 64
 * channels — the regulariser of the mesh side (a penalty on positions or on a learned attribute, or the operator of a solve
 * (I + lambda L) u = b).  d_x: n_sets fields of n_verts vertices, vertex v of set s at float (s * n_verts + v) * x_stride, n_ch floats
 * read there, x_stride >= n_ch; d_out laid out the same way with out_stride >= n_ch, n_ch floats written per vertex, the other floats
 * of a strided record are not touched.  n_ch is 1 .. 64, n_sets 1 .. 65535.  A null d_x selects the slot's own positions (stride 8;
 * n_ch must be 3 and n_sets 1).  d_wpos: ONE position set shared by the sets, vertex v at float v * wpos_stride, wpos_stride >= 3;
 * only COTAN reads it, and there null selects the slot's own positions.  d_out is never null. */
#define SRZ_LAP_UMBRELLA 0   /* x[v] - mean of the neighbours: not symmetric */
#define SRZ_LAP_GRAPH    1   /* n x[v] - sum of the neighbours: symmetric, positive semidefinite */
#define SRZ_LAP_COTAN    2   /* cotangent weights from a position set held fixed: symmetric */
/* THE RULE, in float32, nothing fused, in this order; dot3 and cross are srz_mesh_normals'.  The channels j are independent and
 * follow the same order of operations.  Per set and vertex v: list(v) is the slot's corner list of v, in list order
 * (srz_mesh_upload); per corner c:  f = c / 3;  k = c % 3;  (i0, i1, i2) = faces[f];  a = i[(k + 1) % 3];  b = i[(k + 2) % 3];
 * n_v = (float)(2 * |list(v)|).
 *   UMBRELLA:  S = +0;  for c in list(v):  S = S + (x[a] + x[b]);   n_v > 0:  out[v] = x[v] - S / n_v;   otherwise out[v] = +0
 *     (a neighbour counts once per face it shares with v: twice across an interior edge, once on a boundary edge; on a closed
 *     manifold mesh this is the uniform Laplacian)
 *   GRAPH:     S as above;   out[v] = n_v * x[v] - S
 *   COTAN:     with p = wpos, in the face's OWN vertex order whichever corner asks:
 *                N = cross(p[i1] - p[i0], p[i2] - p[i0]);  d2 = dot3(N, N);  ok = d2 > 0 && d2 <= FLT_MAX;  ia = 1.0f / sqrtf(d2)
 *                cot_m = dot3(p[i_(m+1)] - p[i_m], p[i_(m+2)] - p[i_m]) * ia        (m = 0, 1, 2, indices mod 3)
 *              acc = +0;  for c in list(v) whose face is ok:  acc = acc + (cot_b * (x[v] - x[a]) + cot_a * (x[v] - x[b]))
 *                (cot_a, cot_b: the face's cotangents at a and at b);   out[v] = 0.5f * acc
 *              A face that is not ok is SKIPPED, never multiplied by zero: a non-finite x behind it reaches nothing.  The weight of
 *              edge (v, a) in face f is the same word from v's side and from a's side: the matrix is symmetric in the bits.
 * A GATHER — the one thread that owns (s, v) and a chunk of channels stores its floats once — with plain stores and no atomics:
 * DETERMINISTIC, bit for bit.  Non-finite values propagate as IEEE has them, to the vertex itself and to its neighbours only.  No
 * input value makes the pass read or write outside its buffers.  Asynchronous on `stream` (NULL: the ctx's own stream,
 * SRZ_STREAM_NULL: HIP's null stream), as the other mesh passes are.
 * SRZ_E_INVALID, nothing written and nothing launched, for: everything srz_mesh_normals refuses of ctx, mesh_id and n_sets; n_ch of 0
 * or above 64; a stride of a non-null buffer below n_ch, or a wpos_stride below 3 (of a non-null d_wpos, whichever kind); an unknown
 * kind; a null d_x with n_ch != 3 or n_sets != 1; a null d_out; a pointer that is not 4-byte aligned; an output whose span (first to
 * last float reached) overlaps the input's span, or overlaps wpos' span when COTAN reads it.  There is NO in-place record form: the
 * pass reads its neighbours' inputs, so running it in place is a race. */
int srz_mesh_laplacian(srz_ctx *ctx, int mesh_id, const float *d_x, uint32_t x_stride, uint32_t n_ch, uint32_t n_sets, int kind,
                       const float *d_wpos, uint32_t wpos_stride, float *d_out, uint32_t out_stride, void *stream);
/* THE BACKWARD of srz_mesh_laplacian: THE EXACT TRANSPOSE, also a gather; it needs neither x nor a workspace.  d_gout: the gradient
 * with respect to the output, laid out like d_out with gout_stride >= n_ch; d_gx: the gradient with respect to x, laid out the same
 * way with gx_stride >= n_ch, EVERY element (n_ch floats per vertex) written.  kind, d_wpos, wpos_stride: the forward call's.
 *   GRAPH, COTAN:  the matrix is symmetric: srz_mesh_laplacian_grad IS the forward rule applied to gout — the same kernel, the same
 *     bits as srz_mesh_laplacian over the same data.
 *   UMBRELLA:  T = +0;  for c in list(v):  T = T + (gout[a] / n_a + gout[b] / n_b);   gx[v] = (n_v > 0 ? gout[v] : +0) - T
 *     (n_u = (float)(2 * |list(u)|), read from the corner lists; a vertex that a face names has n_u >= 2)
 * Plain stores, no atomics: DETERMINISTIC, bit for bit.  Non-finite values propagate as IEEE has them, to the vertex itself and to
 * its neighbours only.  No input value makes the pass read or write outside its buffers.  Asynchronous on `stream`.
 * SRZ_E_INVALID, nothing written and nothing launched, for what srz_mesh_laplacian refuses (d_gout in d_x's place, d_gx in d_out's)
 * and for a null d_gout: the backward has no null form. */
int srz_mesh_laplacian_grad(srz_ctx *ctx, int mesh_id, const float *d_gout, uint32_t gout_stride, uint32_t n_ch, uint32_t n_sets, int kind,
                            const float *d_wpos, uint32_t wpos_stride, float *d_gx, uint32_t gx_stride, void *stream);
/* THE MESH EDGE TERMS over a slot's connectivity, ON THE DEVICE: per (face, edge) the number of faces on the edge, the edge's length,
 * and the normal consistency (1 - cos of the dihedral angle) with the faces across it — the two regularisers a fitting loop uses
 * beside a Laplacian.  The slot holds no edge table: the adjacency is found from the corner lists (srz_mesh_upload).
 * d_pos, pos_stride, n_sets: as srz_mesh_normals (a null d_pos selects the slot's own positions, stride 8, n_sets must be 1).
 * d_out: a per-(face, edge) field, for set s and face f THREE floats at float (s * n_faces + f) * out_stride, out_stride >= 3; the
 * other floats of a strided record are not touched.  EDGE j of a face (i0, i1, i2) lies opposite corner j: it joins
 * a_j = i[(j + 1) % 3] and b_j = i[(j + 2) % 3]. */
#define SRZ_EDGE_COUNT    0   /* the number of faces on the edge: 1 boundary, 2 manifold, more non-manifold */
#define SRZ_EDGE_LENGTH   1   /* |p[b_j] - p[a_j]| */
#define SRZ_EDGE_DIHEDRAL 2   /* the sum over the faces across the edge of 1 - dot3(unit normal of f, unit normal of g) */
/* THE NEIGHBOURS OF (f, j), which every kind uses: a list of ENTRIES (g, j'), g a face and j' one of its edges.
 *   w = whichever of a_j, b_j has the SHORTER corner list, a_j on a tie;  o = the other of the two
 *   for corner c in list(w), in list order:  g = c / 3;  k = c % 3;  (g0, g1, g2) = faces[g]
 *     g == f:                  no entry
 *     g[(k + 1) % 3] == o:     the entry (g, (k + 2) % 3)      (o is at g's next corner; the edge opposite the remaining corner)
 *     else g[(k + 2) % 3] == o:  the entry (g, (k + 1) % 3)    (o is at g's previous corner)
 *     otherwise:               no entry
 * ONE entry per corner, never two.  A face that names a vertex twice follows this rule as written.  Between two faces of three
 * distinct vertices each the relation is mutual: (g, j') is an entry of (f, j) exactly when (f, j) is an entry of (g, j').
 * THE RULES, in float32, nothing fused, in this order; dot3 and cross are srz_mesh_normals'.  p: the set's positions.
 *   COUNT:     out[f][j] = (float)(1 + the number of entries).  Positions are not read; n_sets must be 1.
 *   LENGTH:    d = p[b_j] - p[a_j];  out[f][j] = sqrtf(dot3(d, d))
 *   DIHEDRAL:  THE UNIT NORMAL of a face (i0, i1, i2), in the face's OWN vertex order whichever side asks:
 *                N = cross(p[i1] - p[i0], p[i2] - p[i0]);  d2 = dot3(N, N);  ok = d2 > 0 && d2 <= FLT_MAX;  r = 1.0f / sqrtf(d2);
 *                n = N * r      (componentwise)
 *              f not ok:  out[f][j] = +0.  Otherwise  acc = +0;  for the entries (g, j') in entry order whose g is ok:
 *                acc = acc + (1.0f - dot3(n_f, n_g));   out[f][j] = acc
 *              A face that is not ok is SKIPPED, never multiplied by zero.  The term of the pair (f, g) is the same word from both
 *              sides: dot3's products commute and its adds keep their order.
 * A GATHER — the one thread that owns (s, f) stores its three floats once — with plain stores and no atomics: DETERMINISTIC, bit for
 * bit.  Non-finite positions propagate as IEEE has them, to the faces that name the vertex and to their edge neighbours only.  No
 * input value makes the pass read or write outside its buffers.  Asynchronous on `stream` (NULL: the ctx's own stream,
 * SRZ_STREAM_NULL: HIP's null stream), as the other mesh passes are.  A slot with no faces is not an error: nothing is launched.
 * SRZ_E_INVALID, nothing written and nothing launched, for: everything srz_mesh_normals refuses of ctx, mesh_id, n_sets, d_pos and
 * pos_stride; an unknown kind; COUNT with n_sets != 1; a null d_out; out_stride below 3; a pointer that is not 4-byte aligned; an
 * output span (first to last float reached) that overlaps the positions' span (under COUNT too). */
int srz_mesh_edges(srz_ctx *ctx, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, int kind, float *d_out,
                   uint32_t out_stride, void *stream);
/* THE BACKWARD of srz_mesh_edges to the positions.  d_gout: the gradient with respect to the output, laid out like d_out with
 * gout_stride >= 3; d_gpos: [n_sets][n_verts][3] packed, EVERY element written (zeros for a slot with no faces); d_work: DIHEDRAL's
 * workspace [n_sets][n_faces][3] packed, whose contents afterwards are unspecified — LENGTH does not use it, it may be null there.
 * COUNT has no backward: it is refused.  In float32, nothing fused, all gathers:
 *   LENGTH, one phase, per set and vertex v:  acc = (+0, +0, +0);  for corner c in list(v), in list order:  f = c / 3;  k = c % 3
 *     v is the b end of edge j1 = (k + 1) % 3 and the a end of edge j2 = (k + 2) % 3 of f.  For an edge j:  d_j = p[b_j] - p[a_j];
 *     len_j = sqrtf(dot3(d_j, d_j));  the edge is LIVE when len_j > 0 && len_j <= FLT_MAX;  u_j = d_j * (1.0f / len_j)
 *     j1 live:  acc = acc + gout[f][j1] * u_j1;    then j2 live:  acc = acc - gout[f][j2] * u_j2        (componentwise)
 *     An edge that is not live is SKIPPED.   d_gpos[s][v] = acc
 *   DIHEDRAL, two phases (the second starts when the first has ended), w = gout:
 *     PHASE 1, per set and face f:  f not ok:  gN[f] = (+0, +0, +0).  Otherwise  H = (+0, +0, +0);  for j = 0, 1, 2, for the entries
 *       (g, j') of (f, j) in entry order whose g is ok:  s = w[f][j] + w[g][j'];  H = H - n_g * s        (componentwise)
 *       t = dot3(n_f, H);  gN[f] = (H - n_f * t) * r_f        (componentwise: (H.x - n_f.x * t) * r_f, ...);  d_work[s][f] = gN[f]
 *     PHASE 2, per set and vertex v:  srz_mesh_normals_grad's phase 2 with G = gN of the corner's own face:  acc = (+0, +0, +0);
 *       for corner c in list(v), in list order:  (i0, i1, i2) = faces[c / 3];  a, b, c' = p[i0], p[i1], p[i2];  k = c % 3;  G = gN[c / 3]
 *       k == 0:  acc = acc + cross(b - c', G);   k == 1:  acc = acc + cross(c' - a, G);   k == 2:  acc = acc + cross(G, b - a)
 *       d_gpos[s][v] = acc
 * Plain stores, no atomics: DETERMINISTIC, bit for bit.  The gradient is that of the rule as stated wherever the neighbour relation
 * is mutual (it is between ok faces).  Non-finite values propagate as IEEE has them.  No input value makes the pass read or write
 * outside its buffers.  Asynchronous on `stream`.
 * SRZ_E_INVALID, nothing written and nothing launched, for what srz_mesh_edges refuses of ctx, mesh_id, n_sets, d_pos and pos_stride,
 * and for: a kind that is not LENGTH or DIHEDRAL; a null d_gout or d_gpos; a null d_work under DIHEDRAL; gout_stride below 3; a
 * pointer that is not 4-byte aligned; d_gpos or (DIHEDRAL) d_work overlapping the positions' or d_gout's span, or each other. */
int srz_mesh_edges_grad(srz_ctx *ctx, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, int kind,
                        const float *d_gout, uint32_t gout_stride, float *d_work, float *d_gpos, void *stream);

/* ---- draw = TraditionalRasterizer::draw(TRIANGLES) for one scene ----------------------
 * z/c0/c1/c2: W*H floats each, in/out (m_zBuffer, m_channels[0..2]); draw never clears unless
 * SRZ_FUSED_CLEAR.  primitive: LINES is accepted and rasterised as triangles exactly like the
 * reference (src/Rasterizer.cpp:185-189; rasterizeWireframe is never called); anything else →
 * SRZ_E_PRIMITIVE.  stats may be NULL. */
int srz_draw(srz_ctx *ctx, int primitive, const srz_frame *frame, float *z, float *c0, float *c1,
             float *c2, srz_stats *stats);

/* Batch form of srz_draw (host buffers): n frames of one size in one launch set.  planes[f] points to 4*W*H floats of
 * frame f laid out [z | c0 | c1 | c2], in/out like srz_draw's four pointers.  stats (optional) = sums over the batch.
 * The batch is rendered in pieces of ~128 MB of planes: piece k is read back on a second stream while piece k + 1 renders (and
 * uploads its in/out planes); planes registered with srz_host_register move by DMA.  SRZ_NO_Z_READBACK (per frame) skips the depth
 * plane's download.  For data that stays on the device use the frameset calls below. */
int srz_draw_batch(srz_ctx *ctx, int primitive, const srz_frame *frames, int n_frames, float *const *planes,
                   srz_stats *stats);

/* ---- throughput mode: frames resident in HBM ------------------------------------------
 * A frameset copies n frames (same width/height) to the device once.  srz_frameset_render
 * rasterises + shades all of them into ONE device buffer laid out
 *     [frame][plane: z,c0,c1,c2][local_rows][width]   (float32)
 * where local_rows = srz_frameset_local_rows() (= height for an unsharded ctx, else
 * bands_per_rank*32, zero-padded).  d_out is a DEVICE pointer (e.g. a torch tensor's data_ptr),
 * stream a hipStream_t (NULL = the ctx's own non-blocking stream; pass SRZ_STREAM_NULL for HIP's null stream:
 * work on the ctx's stream is NOT ordered against the null stream).  The call is asynchronous on that stream, the first render of
 * a set included: srz_frameset_create / srz_sceneset_create (synchronous anyway: they upload) run a binning pass of their own and
 * size the tile-list pool by its count of (triangle, tile) pairs, so a set is rendered by the fast path as a whole from its first
 * render on.  Afterwards the pool follows the previous renders'
 * demand (a sceneset's geometry may change with srz_sceneset_update); growth — rare — is the one place a render waits for the
 * device (hipDeviceSynchronize + hipMalloc), and the bands that did not fit take the ordered rasteriser in the render that found out.
 * srz_set_option(ctx, SRZ_OPT_POOL_LAZY, 1) before creating the set skips the creation-time pass (the pool then only follows the
 * renders' demand). */
#define SRZ_STREAM_NULL ((void *)(intptr_t)-1)
int srz_frameset_create(srz_ctx *ctx, const srz_frame *frames, int n_frames, srz_frameset **out);
/* Same, but the frames are given as meshes + matrices: every srz_frameset_render first runs the vertex stage on the
 * device (k_vertex) to produce the post-MVP stream, i.e. it times the reference's whole draw(). */
int srz_sceneset_create(srz_ctx *ctx, const srz_scene_frame *frames, int n_frames, srz_frameset **out);
/* draw() for one scene with the vertex stage on the device (host planes in/out, like srz_draw) */
int srz_draw_scene(srz_ctx *ctx, int primitive, const srz_scene_frame *frame, float *z, float *c0, float *c1, float *c2,
                   srz_stats *stats);
void srz_frameset_destroy(srz_ctx *ctx, srz_frameset *fs);
int srz_frameset_local_rows(const srz_ctx *ctx, const srz_frameset *fs);
size_t srz_frameset_out_bytes(const srz_ctx *ctx, const srz_frameset *fs);
int srz_frameset_render(srz_ctx *ctx, srz_frameset *fs, void *d_out, size_t out_bytes,
                        uint32_t flags, void *stream);
/* The VISIBILITY BUFFER instead of the shaded image: which triangle owns each pixel and where inside it the pixel lies.  Same
 * arguments, flag mask, stream semantics, buffer size (srz_frameset_out_bytes), local_rows and band sharding as srz_frameset_render;
 * framesets and scenesets alike.  The buffer is [frame][4 planes][local_rows][width], 4 bytes per word:
 *     plane 0  z      float32  the owner fragment's depth, bit-identical to plane 0 of srz_frameset_render   (nobody: +inf)
 *     plane 1  id     uint32   (triangle index + 1) | (S class ? 0x80000000 : 0)                                (nobody: 0)
 *     plane 2  alpha  float32  the owner's barycentric alpha, exactly as the shaders use it                     (nobody: 0)
 *     plane 3  beta   float32  the owner's beta, likewise                                                       (nobody: 0)
 * "nobody" = a pixel no triangle owns in a frame rendered with SRZ_FUSED_CLEAR (frame flags | render flags).
 * Triangle index: the position in the FRAME's own triangle stream — its batches in array order, culled triangles counted; for a
 * sceneset its draws in order, n_faces records each — not in the frameset-wide array.
 * alpha / beta (the oracle's values): V class (the 8-wide columns of the owner's bounding box) alpha = fmsub(PBx,PCy,PCx*PBy) * RN(1/area_v),
 * S class (the scalar tail) alpha = aPBC / s_area with the IEEE division; beta likewise.  gamma is not stored: 1 - (alpha + beta) for V,
 * (1 - alpha) - beta for S, as the shaders compute it (the class bit says which).  Exact in every mode: SRZ_OPT_APPROX_SHADE has no
 * effect here.  SRZ_UNIFIED (every pixel V class) and SRZ_ORDERED_RASTER mean what they mean for the colour render.
 * Without SRZ_FUSED_CLEAR the call changes exactly the pixels the colour render would change: a pixel whose incoming value survives
 * keeps all four of its words (two visibility renders can be layered).
 * The "nobody" words are the clear values of the exchange (z = +inf, three zero words), so a visibility buffer goes through
 * srz_frameset_allgather / _allgather_inplace / _deinterleave / _read_gathered_frame and the tile-sparse exchange unchanged, as
 * SRZ_EXCHANGE_PLANES.  No texture has to be uploaded; the render files no sample of the side clear's grid measurement. */
int srz_frameset_render_visibility(srz_ctx *ctx, srz_frameset *fs, void *d_out, size_t out_bytes, uint32_t flags, void *stream);
/* DEPTH PEELING: the layer BEHIND a visibility buffer.  d_prev: a visibility buffer of THIS set with its current geometry — layer k,
 * from srz_frameset_render_visibility or from this call; d_out receives layer k + 1 in the same layout, [frame][z, id, alpha, beta]
 * [local_rows][width], so every pass over a visibility buffer (shade, G-buffer, motion, interpolate, texture, antialias and their
 * gradients) works on every layer unchanged.  Size, 16-byte alignment (of both), stream semantics, local_rows and band sharding as
 * srz_frameset_render_visibility; asynchronous, no host synchronisation beyond what a render has (the tile-list pool's growth); a
 * sceneset runs its vertex stage first; no sample of the side clear's grid measurement.  Any overlap of the two buffers is
 * SRZ_E_INVALID.  Flags: the render's mask; SRZ_UNIFIED means what it means for a render, SRZ_ORDERED_RASTER is accepted and has no
 * effect, and all four words of EVERY pixel are written, as by a render with SRZ_FUSED_CLEAR (implied).
 * THE RULE, per pixel, with zp, idp the words of d_prev, wp = (idp & 0x7fffffff) - 1 and sp = idp >> 31:
 *   the pixel has ENDED if idp == 0, or wp >= the frame's triangle count, or zp is NaN: the output is nobody (+inf, 0, 0, 0).
 *   Otherwise take every FRAGMENT of the frame at that pixel as the renders compute it — coverage and class the reference's (V in the
 *   8-wide columns of the owner's bounding box, S in its scalar tail; with SRZ_UNIFIED every fragment is V), depth the class's own z
 *   expression: a fragment is (z, w = triangle index in the frame, s = class); one whose z is NaN is never taken.  The fragments of a
 *   pixel are ORDERED by z ascending (float comparison: +0 == -0); at equal z the S fragments come first, by w descending, then the V
 *   fragments, by w ascending — the renders' "last S at that depth, else first V" as a total order.  The output is the first
 *   fragment in that order STRICTLY AFTER (zp, wp, sp), or nobody if there is none: z, (w + 1) | s << 31, and alpha and beta exactly
 *   as the shaders use them (srz_frameset_render_visibility).
 * Consequences: for frames without NaN depths layer k + 1 is what the reference renders when, at every pixel, the owners of layers
 * 1..k are not drawn.  Peeling until a layer is all nobody visits every (triangle, pixel) pair of srz_stats.fragments exactly once.
 * A d_prev whose every pixel is (z = -inf, id = 1) gives layer 1: for frames of finite depths bit-identical to
 * srz_frameset_render_visibility on all four planes.  d_prev is only COMPARED, never used as an index: any words in it give defined
 * output and no out-of-range access. */
int srz_frameset_peel_visibility(srz_ctx *ctx, srz_frameset *fs, const void *d_prev, void *d_out, size_t out_bytes,
                                 uint32_t flags, void *stream);
/* The COLOUR of a visibility buffer: rasterise once (srz_frameset_render_visibility), shade many times — new lights, ka / ks / p, shader
 * types (srz_frameset_update_shading, srz_sceneset_update).  d_vis: a visibility buffer of THIS set on this ctx's shard; d_out: a buffer
 * in the layout of srz_frameset_render.  Size (srz_frameset_out_bytes, for each of the two), 16-byte alignment of both, the flag mask,
 * stream semantics, local_rows and band sharding as srz_frameset_render; asynchronous, no host synchronisation.  Per pixel of d_vis:
 *   id != 0 (and (id & 0x7fffffff) - 1 < the frame's triangle count): plane 0 = the visibility z, bit for bit; planes 1..3 = the colour
 *            the colour render gives owner (id & 0x7fffffff) - 1 of that frame at (x, y), from the stored alpha and beta (gamma =
 *            1 - (alpha + beta) for class V, (1 - alpha) - beta for class S: bit 31 of id) with the set's CURRENT shading data — eye, ka,
 *            ks, p, kh, kn, lights, each batch's shader and texture (which must be uploaded, as for srz_frameset_render);
 *   otherwise ("nobody"): with SRZ_FUSED_CLEAR (frame flags | flags) the clear values (+inf, 0, 0, 0); without it the four output
 *            words are left untouched.
 * So srz_frameset_shade_visibility(render_visibility(F), F) is bit-identical to srz_frameset_render(F) on all four planes, in every
 * shading build (the tolerance mode of SRZ_OPT_APPROX_SHADE included: against that set's own colour render) and for SRZ_UNIFIED and
 * SRZ_ORDERED_RASTER renders.  d_out == d_vis (in place) is allowed: the owned pixels' planes 1..3 are written, and with SRZ_FUSED_CLEAR
 * the four words of a pixel whose id is out of range get the clear values; id-0 words are left as they are (after a fused visibility
 * render they are the clear values already).  A partial overlap of the two buffers is SRZ_E_INVALID.  A sceneset
 * runs its vertex stage first, as a render does.  The call files no sample of the side clear's grid measurement. */
int srz_frameset_shade_visibility(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, void *d_out, size_t out_bytes,
                                  uint32_t flags, void *stream);
/* The G-BUFFER of a visibility buffer: per pixel, the attributes the built-in shaders are handed for its owner — bit for bit what
 * they consume — so that a shader of the caller's own (a lighting model in torch, a material mask, a denoiser's guide images) need not
 * restate the two interpolation rules, the two texel fetches and the batch → shader → texture lookup.  `what` names the groups: */
#define SRZ_GB_NORMAL 1u  /* 3 planes nx, ny, nz */
#define SRZ_GB_UV     2u  /* 2 planes u, v */
#define SRZ_GB_BATCH  4u  /* 1 plane uint32 */
#define SRZ_GB_ALBEDO 8u  /* 3 planes, in the order of the colour planes (plane 0 = texture blue) */
/* d_vis: a visibility buffer of THIS set on this ctx's shard (srz_frameset_out_bytes); d_out: [frame][plane][local_rows][width], 4-byte
 * words, the planes of the groups in `what` in the order above, without gaps: srz_frameset_gbuffer_bytes(what) bytes (0 for what == 0 or
 * an unknown bit).  Band sharding, local_rows, stream semantics, 16-byte alignment of both buffers and asynchrony (no host wait) as
 * srz_frameset_shade_visibility; a sceneset runs its vertex stage first.  d_out may not overlap d_vis (the layouts differ):
 * SRZ_E_INVALID, like what == 0, an unknown bit of `what`, a short out_bytes and any bit of `flags` but SRZ_FUSED_CLEAR.
 * The pass reads the id plane everywhere and alpha / beta where there is an owner; never z, and it needs no pixel coordinate.
 * Per pixel with an owner (id != 0 and (id & 0x7fffffff) - 1 < the frame's triangle count; class = bit 31 of id; gamma =
 * 1 - (alpha + beta) for V, (1 - alpha) - beta for S):
 *   NORMAL  the interpolated, normalised normal as the owner's class hands it to its shader.  V: fma interpolation, then
 *           NormalSIMD::normalized (a length that is not > 0: (0, 0, 0)); S: products and sums, then glm::normalize (zero length: NaN)
 *   UV      the raw interpolated u, v of the class (V: fma; S: products and sums), before any scaling or clamping
 *   BATCH   the owner's batch index within its frame (for a sceneset: its draw) + 1
 *   ALBEDO  the kd the owner's shader multiplies its lighting by, under the set's CURRENT shading data (srz_frameset_update_shading,
 *           srz_sceneset_update, texture uploads).  V class, TEXTURE batch: the texel at the round-half-even of the scaled coordinate
 *           clamped to [0, size - 1], times RN(1/255); S class, TEXTURE / BUMP / DISPLACEMENT batch: the texel at the truncated
 *           clamped-then-scaled coordinate divided by 255, black outside the texture (u or v == 1, a NaN coordinate); every other
 *           combination: (1, 1, 1).  Only when ALBEDO is asked for must the textures be uploaded (else SRZ_E_TEXTURE).
 * Always the exact arithmetic (correctly rounded reciprocal, root and division): SRZ_OPT_APPROX_SHADE has no effect.
 * Pixels nobody owns (id 0 or out of range): with SRZ_FUSED_CLEAR (frame flags | flags) every requested word is 0; without it the
 * words are left untouched. */
size_t srz_frameset_gbuffer_bytes(const srz_ctx *ctx, const srz_frameset *fs, uint32_t what);
int srz_frameset_gbuffer(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, void *d_out, size_t out_bytes, uint32_t what, uint32_t flags,
                         void *stream);
/* The MOTION PASS of a visibility buffer: where the surface point under each pixel of frame f lies in frame g = f + delta of the same
 * set — optical flow, the depth there, and who owns the nearest sample there (an occlusion test) — for sets whose frames are poses of
 * one mesh: triangle t of frame g is taken to be triangle t of frame f.  It completes the guide images a G-buffer is made for
 * (normal, albedo, depth, motion) without the caller restating the two interpolation rules and both forms of gamma.  `what` names
 * the groups: */
#define SRZ_MV_FLOW   1u /* 2 planes  dx, dy   float32 */
#define SRZ_MV_DEPTH  2u /* 1 plane   z'       float32 */
#define SRZ_MV_TARGET 4u /* 2 planes  tid uint32, tz float32 */
/* d_vis: a visibility buffer of THIS set on this ctx's shard; d_out: [frame][plane][local_rows][width], 4-byte words, the planes of the
 * groups in `what` in the order above, without gaps: srz_frameset_motion_bytes(what) bytes (0 for what == 0 or an unknown bit).  Size,
 * 16-byte alignment of both buffers, band sharding, stream semantics, asynchrony and the null-argument rules as srz_frameset_gbuffer; a
 * sceneset runs its vertex stage first.  No texture need be uploaded.
 * Per pixel (x, y) of frame f — y the FRAME's row, not the shard's local row — whose id names an owner t (id != 0 and
 * (id & 0x7fffffff) - 1 < frame f's triangle count; class = bit 31 of id; gamma = 1 - (alpha + beta) for V, (1 - alpha) - beta for S),
 * with a, b, c the three positions of triangle t in frame g's stream:
 *   the point in g   P' = (x', y', z'), each component interpolated exactly as the class interpolates z:
 *                    V: fma(alpha, a, fma(beta, b, gamma * c));  S: alpha * a + beta * b + gamma * c, left to right, nothing fused
 *   FLOW    dx = x' - (float)x, dy = y' - (float)y
 *   DEPTH   z'
 *   TARGET  tx = rintf(x'), ty = rintf(y') (round half even; a pixel's sample point is its integer corner, so this is the nearest
 *           sample).  Inside — tx >= 0 && tx <= W - 1 && ty >= 0 && ty <= H - 1, compared as floats before any conversion, so that a
 *           NaN or a huge coordinate is outside and never becomes an index —: tid and tz are the raw words of planes 1 and 0 of frame
 *           g in d_vis at (tx, ty).  Outside: tid = 0, tz = +inf.  (tid == the pixel's own id, or tz close to z', means the point is
 *           visible in g; anything else that it is occluded there or has left the image.)
 * The interpolation is LINEAR IN SCREEN SPACE, as everywhere in the reference, which has no perspective-correct interpolation
 * (srz_frameset_perspective, below, adds it for the attribute-side passes; this pass interpolates screen positions and keeps the
 * ORIGINAL buffer).
 * Always the exact arithmetic: SRZ_OPT_APPROX_SHADE has no effect.
 * Nobody: a pixel nobody owns (id 0 or out of range), and EVERY pixel of a frame whose g lies outside [0, n_frames).  With
 * SRZ_FUSED_CLEAR (frame flags | flags) every requested word of a nobody pixel is 0; without it those words are left untouched.
 * Two consequences: with delta == 0, DEPTH equals plane 0 of d_vis bit for bit at every owned pixel, and TARGET returns the pixel's own
 * id and z wherever |dx| and |dy| are below 0.5.
 * SRZ_E_INVALID, the output untouched, for: what == 0 or an unknown bit of `what`; a short out_bytes; a misaligned pointer; d_out
 * overlapping d_vis; any bit of `flags` but SRZ_FUSED_CLEAR; some pair (f, f + delta) inside the set whose frames differ in triangle
 * count (nothing is launched); SRZ_MV_TARGET on a ctx whose shard world is above 1 (the target row may belong to another rank — FLOW
 * and DEPTH work on any shard). */
size_t srz_frameset_motion_bytes(const srz_ctx *ctx, const srz_frameset *fs, uint32_t what);
int srz_frameset_motion(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, void *d_out, size_t out_bytes, uint32_t what, int delta,
                        uint32_t flags, void *stream);
/* CALLER ATTRIBUTES over a visibility buffer, and their gradients: per-vertex data of the caller's own (colours, object-space
 * positions, labels, skinning weights, tangents — whatever the 96-byte srz_tri does not carry) interpolated under each pixel's
 * alpha, beta, gamma exactly as the owner's class interpolates uv, and the backward of that interpolation: the front half of a
 * differentiable renderer.
 * d_vis: a visibility buffer of THIS set on this ctx's shard.  d_attr: [attr_frames][attr_tris][3 corners][n_ch] float32, 4-byte
 * aligned; attr_frames is 1 (every frame reads the same array: poses of one mesh) or the set's frame count; attr_tris is at least
 * every frame's triangle count.  Triangle index and corner order are the visibility buffer's and srz_tri's: the index is the position
 * in the frame's own stream, corners 0, 1, 2 go with alpha, beta, gamma.  d_out and d_gout: [frame][n_ch][local_rows][width] float32,
 * srz_frameset_interpolate_bytes(n_ch) bytes (0 for n_ch == 0 or n_ch > SRZ_ATTR_MAX_CH, or a null set).  Band sharding, local_rows,
 * stream semantics, asynchrony and the 16-byte alignment of the visibility buffer and every plane buffer (d_out, d_gout, d_gbary) as
 * srz_frameset_gbuffer.  The passes read no position, record or texture: a sceneset does not run its vertex stage, nothing else is
 * launched.  Owner and nobody as srz_frameset_gbuffer: (id & 0x7fffffff) - 1 < the frame's triangle count means an owner, bit 31 of
 * id is the class, gamma = 1 - (alpha + beta) for V and (1 - alpha) - beta for S.
 * FORWARD, bit for bit: with a, b, c the owner's three values of channel ch,
 *   V: fma(alpha, a, fma(beta, b, gamma * c));  S: alpha * a + beta * b + gamma * c, left to right, nothing fused.
 * Always the exact arithmetic: SRZ_OPT_APPROX_SHADE has no effect.  A nobody pixel gets 0 with SRZ_FUSED_CLEAR (frame flags | flags)
 * and is left untouched without it.
 * BACKWARD: at least one of d_gattr and d_gbary is non-null.
 *   d_gattr has d_attr's shape (d_attr itself may be null when only d_gattr is asked for).  For every owned pixel with weights
 *   w = (alpha, beta, gamma) and every channel ch the float32 product w[k] * gout[ch] is ADDED to gattr[fa][t][k][ch] (fa = 0 when
 *   attr_frames == 1): the caller zeroes the buffer, or accumulates over several calls.  THE ORDER OF THE ADDS IS UNSPECIFIED, each
 *   add rounds, so this buffer is NOT BIT-REPRODUCIBLE between launches — the one place in this ABI where that holds.  With n
 *   contributing pixels an element lies within n 2^-24 / (1 - n 2^-24) * sum |w[k] * gout[ch]| of the exact sum; an element with one
 *   contributing pixel is exact.  The adds are hardware float atomics: d_gattr must be ordinary (coarse-grained) device memory.  On
 *   a sharded ctx each rank produces the partial sums of its own bands.
 *   d_gbary: [frame][2][local_rows][width] float32, needs d_attr: dalpha = acc after acc = 0; for ch ascending: acc = fma(gout[ch],
 *   a - c, acc), dbeta the same with b - c, the differences rounded to float first.  Deterministic, bit for bit.  Nobody pixels as
 *   in the forward pass: 0 when fused, untouched otherwise.
 *   Words of d_gout at nobody pixels never reach a result: they may hold anything.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, d_vis, d_attr (forward; backward with d_gbary),
 * d_out, d_gout, or both of d_gattr and d_gbary; n_ch == 0 or above SRZ_ATTR_MAX_CH; attr_frames not 1 or the frame count; attr_tris
 * below some frame's triangle count; a misaligned pointer; a short out_bytes; any bit of `flags` but SRZ_FUSED_CLEAR; an output that
 * overlaps an input (d_out with d_vis or d_attr; d_gattr or d_gbary with d_vis, d_gout or d_attr) or the other output. */
#define SRZ_ATTR_MAX_CH 64u
size_t srz_frameset_interpolate_bytes(const srz_ctx *ctx, const srz_frameset *fs, uint32_t n_ch);
int srz_frameset_interpolate(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_attr, uint32_t n_ch, uint32_t attr_frames,
                             uint32_t attr_tris, void *d_out, size_t out_bytes, uint32_t flags, void *stream);
int srz_frameset_interpolate_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_gout, const float *d_attr, uint32_t n_ch,
                                  uint32_t attr_frames, uint32_t attr_tris, float *d_gattr, void *d_gbary, uint32_t flags, void *stream);
/* POSITION GRADIENTS of a visibility buffer: the step behind srz_frameset_interpolate_grad's d_gbary — from the loss gradient with
 * respect to each pixel's alpha and beta (and / or to its depth, plane 0) to the gradient with respect to the owners' SCREEN
 * POSITIONS, the nine floats ax ay z0 bx by z1 cx cy z2 of a triangle in the dense position stream's order, and to the pixel's own
 * sample point.  Owners are held fixed: this is the interior term of a differentiable rasteriser; the silhouette (coverage) term
 * is srz_frameset_antialias_grad's, below.  (Likewise the mip level lambda of srz_frameset_texture_mip is held fixed in its backward:
 * the derivative planes srz_frameset_interpolate_deriv writes select a level and take no gradient.)  The chain visibility -> interpolate -> loss -> interpolate_grad -> positions then runs on
 * the device.
 * d_vis: a visibility buffer of THIS set on this ctx's shard.  d_gbary: [frame][2][local_rows][width] float32, exactly the planes
 * srz_frameset_interpolate_grad writes (dalpha and dbeta already carry gamma's share).  d_gz: [frame][1][local_rows][width] float32,
 * the gradient with respect to depth plane 0.  At least one of the two is non-null.  d_gpos: [n_frames][pos_tris][9] float32, 4-byte
 * aligned, pos_tris at least every frame's triangle count, triangle index that of the visibility buffer; ADDED into: the caller
 * zeroes it, or accumulates over several calls.  d_gpix: [frame][2][local_rows][width] float32, the gradient with respect to the
 * pixel's sample point (x, then y); a nobody pixel gets 0 with SRZ_FUSED_CLEAR (frame flags | flags) and is left untouched without
 * it.  At least one of d_gpos and d_gpix is non-null.  The two-plane buffers hold srz_frameset_interpolate_bytes(2) bytes, d_gz
 * srz_frameset_interpolate_bytes(1).  Band sharding (each rank adds the partial sums of its own bands), local_rows, stream
 * semantics, asynchrony, the 16-byte alignment of the visibility buffer and every plane buffer, and owner and nobody
 * ((id & 0x7fffffff) - 1 < the frame's triangle count) as srz_frameset_interpolate_grad.  The owner's positions are the set's own,
 * obtained as srz_frameset_motion obtains them: a sceneset runs its vertex stage first.
 * Per owned pixel, in float32, nothing fused beyond what is written, with P the owner's nine floats and w = (alpha, beta, gamma),
 * gamma by the owner's class:
 *   area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);  r = 1.0f / area (the IEEE division, both classes)
 *   da = d_gbary ? dalpha : 0, db likewise;  with d_gz: da = fma(gz, z0 - z2, da), db = fma(gz, z1 - z2, db)
 *   gx = (da * (by - cy) + db * (cy - ay)) * r;  gy = (da * (cx - bx) + db * (ax - cx)) * r     -> d_gpix, deterministic, bit for bit
 *   for corner k: gpos[f][t][3k] += (-w[k]) * gx;  [3k + 1] += (-w[k]) * gy;  with d_gz also [3k + 2] += w[k] * gz
 * (d w_j / d V_k = -w_k grad w_j, grad alpha = (by - cy, cx - bx) / area, grad beta = (cy - ay, ax - cx) / area).  Without d_gz the z
 * slots receive no add.  THE ORDER OF THE ADDS IS UNSPECIFIED, each add rounds, so d_gpos is NOT BIT-REPRODUCIBLE between launches,
 * like d_gattr: with n contributing pixels an element lies within n 2^-24 / (1 - n 2^-24) * sum |term| of the exact sum of the
 * float32 terms; an element with one contributing pixel is exact.  The adds are hardware float atomics: d_gpos must be ordinary
 * (coarse-grained) device memory.  Non-finite values propagate as IEEE has them (a zero area gives inf or NaN); no input value
 * makes the pass read or write outside its buffers.  Words of d_gbary and d_gz at nobody pixels never reach a result.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set or d_vis; both of d_gbary and d_gz null, or both of
 * d_gpos and d_gpix; pos_tris below some frame's triangle count; a misaligned pointer; any bit of `flags` but SRZ_FUSED_CLEAR; an
 * output that overlaps an input (d_vis, d_gbary, d_gz) or the other output. */
int srz_frameset_position_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_gbary, const void *d_gz, uint32_t pos_tris,
                               float *d_gpos, void *d_gpix, uint32_t flags, void *stream);
/* SILHOUETTE ANTIALIASING of a visibility buffer, and its gradients: planes of the caller's (a shaded image, interpolated attributes,
 * a render's own four planes) blended across the outlines of the owners, analytically — no higher resolution is rendered — and the
 * backward of that blend, to the planes and to the SCREEN POSITIONS of the triangles whose edges form the outlines: the silhouette
 * (coverage) term of a differentiable rasteriser, the one srz_frameset_position_grad does not compute.
 * d_vis: a visibility buffer of THIS set on this ctx.  d_in, d_out, d_gout, d_gin: [frame][n_ch][local_rows][width] float32,
 * 1 <= n_ch <= SRZ_ATTR_MAX_CH, srz_frameset_interpolate_bytes(n_ch) bytes.  A render's own four-plane buffer is a valid n_ch = 4
 * input: the z plane is then blended too.  16-byte alignment of the visibility buffer and every plane buffer, stream semantics and
 * asynchrony as srz_frameset_interpolate.  Owner and nobody as there: (id & 0x7fffffff) - 1 < the frame's triangle count means an
 * owner, everything else is nobody; the class bit plays no part.  The positions are the set's own, obtained as
 * srz_frameset_position_grad obtains them: a sceneset runs its vertex stage first.  SRZ_FUSED_CLEAR is accepted and has no effect:
 * EVERY pixel of d_out / d_gin is written, and — unlike every other pass over a visibility buffer — the words of d_in at nobody's
 * pixels DO reach results: they are the background an outline blends with.
 * THE RULE, all of it float32, nothing fused except where fmaf is written, divisions the IEEE division.  A pixel's sample point is
 * its integer corner (x, y), as in the motion pass.  Every pair of 4-neighbours inside the image is evaluated, horizontal and
 * vertical; the evaluation depends on the unordered pair only, so both pixels of a pair see the same answer:
 *   1. a pair does nothing when both pixels are nobody, or both have an owner with the same triangle index.
 *   2. N, the nearer pixel, and F, the farther: a nobody is farther than any owner; between two owners N is the right or lower
 *      pixel iff its z (plane 0) is < the other's — ties and NaN give N = the left or upper pixel.
 *   3. s = +1 if F lies at the larger coordinate, else -1.  For each vertex v of N's triangle, u_v along the pair's axis (0 at N,
 *      1 at F) and n_v across it:  horizontal pair  u_v = s * (v.x - xN), n_v = v.y - yN;  vertical pair  u_v = s * (v.y - yN),
 *      n_v = v.x - xN.
 *   4. the edges (v0, v1) = (a, b), (b, c), (c, a) in this order; THE edge is the first with
 *        (n0 <= 0 && n1 > 0) || (n1 <= 0 && n0 > 0)                                    (it straddles the pair's line, half open)
 *        d = n0 - n1;  k = n0 / d;  t = u0 + k * (u1 - u0);  0 <= t && t <= 1          (it crosses between the two sample points)
 *      (a NaN fails both).  No such edge: the pair does nothing.
 *   5. F has an owner and both v0 and v1 occur among the three corners of F's triangle, compared as the three 32-bit words x, y, z:
 *      the two owners share this edge, an interior edge of a mesh, and the pair does nothing.  (The sets are triangle soups; a
 *      shared mesh vertex reaches both triangles with identical bits, in a frameset and from the vertex stage alike.)
 *   6. a = t - 0.5f.  a > 0: the target is F, the source N, w = a (N's triangle covers that share of F's footprint); a < 0: the
 *      target is N, the source F, w = -a; a == 0: nothing.
 * FORWARD, deterministic, bit for bit (a gather: no float atomics): for every pixel p and channel,
 *   acc = in[p];  for q in (x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1), in this order, where q lies inside the image:
 *   if pair(p, q) has target p: acc = fmaf(w, in[q] - in[p], acc);  out[p] = acc.
 * BACKWARD: d_gout, the same d_in and the same d_vis; at least one of d_gin and d_gpos is non-null.
 *   d_gin has the planes' shape, deterministic, bit for bit:  acc = gout[p];  for q in the same order: if the target is p:
 *   acc = fmaf(-w, gout[p], acc), else if the target is q: acc = fmaf(w, gout[q], acc);  gin[p] = acc.
 *   d_gpos: [n_frames][pos_tris][9] float32, 4-byte aligned, pos_tris at least every frame's triangle count, ADDED into exactly as
 *   srz_frameset_position_grad's d_gpos (the caller zeroes it, or accumulates over several calls — the interior term and this one
 *   into one buffer).  Per pair that has a target, once:
 *     D = 0;  for ch ascending: D = fmaf(gout[tgt][ch], in[src][ch] - in[tgt][ch], D);   g = a > 0 ? D : -D
 *     e = u1 - u0;  q = (g * e) / (d * d);  g_u0 = g * (1.0f - k);  g_u1 = g * k;  g_n0 = q * (-n1);  g_n1 = q * n0
 *     horizontal pair: the x slots of v0, v1 get s * g_u0, s * g_u1, their y slots g_n0, g_n1;  vertical pair: the x slots get
 *     g_n0, g_n1, the y slots s * g_u0, s * g_u1.
 *   The slots are those of N's triangle; z slots and F's triangle get no add.  THE ORDER OF THE ADDS IS UNSPECIFIED, each add
 *   rounds, so d_gpos is NOT BIT-REPRODUCIBLE between launches: with n contributing pairs an element lies within
 *   n 2^-24 / (1 - n 2^-24) * sum |term| of the exact sum of the float32 terms; an element with one contributing pair is exact.  The
 *   adds are hardware float atomics: d_gpos must be ordinary (coarse-grained) device memory.
 * Non-finite values propagate as IEEE has them; no input value makes the passes read or write outside their buffers.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, d_vis, d_in, d_out (forward), d_gout (backward),
 * or both of d_gin and d_gpos; n_ch == 0 or above SRZ_ATTR_MAX_CH; a short out_bytes; pos_tris below some frame's triangle count
 * when d_gpos is given; a misaligned pointer; any bit of `flags` but SRZ_FUSED_CLEAR; an output that overlaps an input (d_vis, d_in,
 * d_gout) or the other output — in place is not allowed, the forward reads neighbours; a ctx whose shard world is above 1 (a
 * vertical pair across a band edge needs another rank's rows: the same refusal as SRZ_MV_TARGET). */
int srz_frameset_antialias(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_in, uint32_t n_ch, void *d_out, size_t out_bytes,
                           uint32_t flags, void *stream);
int srz_frameset_antialias_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_in, const void *d_gout, uint32_t n_ch,
                                void *d_gin, uint32_t pos_tris, float *d_gpos, uint32_t flags, void *stream);
/* CALLER TEXTURES over a visibility buffer, and their gradients: a float32 texture of the caller's own sampled BILINEARLY at the uv
 * planes srz_frameset_interpolate wrote for a two-channel attribute (or srz_frameset_gbuffer(SRZ_GB_UV)), and the backward of that
 * lookup, to the texels and to u, v: the texture lookup of a differentiable renderer (a nearest-texel fetch, which is what the
 * built-in shaders and SRZ_GB_ALBEDO do with an uploaded 8-bit texture, has no gradient in uv).
 * d_vis: a visibility buffer of THIS set on this ctx's shard.  d_uv: [frame][2][local_rows][width] float32 (u, then v),
 * srz_frameset_interpolate_bytes(2) bytes.  d_tex and d_gtex: [tex_frames][tex_h][tex_w][n_ch] float32, channels last, 4-byte aligned;
 * tex_frames is 1 (every frame samples the same texture) or the set's frame count; 1 <= tex_w, tex_h <= SRZ_TEX_MAX_SIZE;
 * 1 <= n_ch <= SRZ_ATTR_MAX_CH.  d_out and d_gout: [frame][n_ch][local_rows][width] float32, srz_frameset_interpolate_bytes(n_ch)
 * bytes.  d_guv: d_uv's shape.  Band sharding (each rank adds the partial sums of its own bands), local_rows, stream semantics,
 * asynchrony, the 16-byte alignment of the visibility buffer and every plane buffer (d_uv, d_out, d_gout, d_guv), and owner and nobody
 * ((id & 0x7fffffff) - 1 < the frame's triangle count; the class bit plays no part) as srz_frameset_interpolate.  The passes read no
 * position, record or uploaded texture: a sceneset does not run its vertex stage, nothing else is launched.  A nobody pixel's words
 * of d_out and d_guv are 0 with SRZ_FUSED_CLEAR (frame flags | flags) and left untouched without it; the words of d_uv and d_gout at
 * nobody's pixels never reach a result: they may hold anything.
 * THE RULE, all of it float32, nothing fused except where fmaf is written, always the exact arithmetic (SRZ_OPT_APPROX_SHADE has no
 * effect).  Per owned pixel, per axis — shown for x with u and W = tex_w; y with v and H = tex_h likewise:
 *   unsampled: u or v not finite (!(fabsf(u) < INFINITY)) -> every channel of out is 0 (written: the pixel has an owner),
 *              guv = (0, 0), no add
 *   WRAP:   u = u - floorf(u)
 *   fx = u * (float)W - 0.5f                  (texel i's centre is (i + 0.5) / W: the texel grid of the built-in shaders' fetch, no flip in v)
 *   CLAMP:  in_x = fx > 0.0f && fx < (float)(W - 1);  fx = fminf(fmaxf(fx, 0.0f), (float)(W - 1))      WRAP: in_x = true
 *   x0f = floorf(fx);  tx = fx - x0f;  x0 = (int)x0f;  x1 = x0 + 1
 *   CLAMP:  x1 = min(x1, W - 1)               WRAP: if (x0 < 0) x0 += W;  if (x1 >= W) x1 -= W
 * FORWARD, deterministic, bit for bit: per channel, with t_rc = tex[y_r][x_c],
 *   top = fmaf(tx, t01 - t00, t00);  bot = fmaf(tx, t11 - t10, t10);  out = fmaf(ty, bot - top, top)
 * BACKWARD: d_gout, the same d_uv and d_vis; at least one of d_gtex and d_guv is non-null.
 *   d_gtex (d_tex itself may be null when only d_gtex is asked for): w00 = (1.0f - tx) * (1.0f - ty), w01 = tx * (1.0f - ty),
 *   w10 = (1.0f - tx) * ty, w11 = tx * ty; for every sampled pixel, corner and channel the float32 product w_rc * gout[ch] is ADDED
 *   to gtex[ft][y_r][x_c][ch] (ft = 0 when tex_frames == 1); two corners that coincide (a clamped border, a one-texel axis) both
 *   add.  The caller zeroes the buffer, or accumulates over several calls.  THE ORDER OF THE ADDS IS UNSPECIFIED, each add rounds, so
 *   d_gtex is NOT BIT-REPRODUCIBLE between launches, like d_gattr: with n contributing adds an element lies within
 *   n 2^-24 / (1 - n 2^-24) * sum |term| of the exact sum of the float32 terms; an element with one contributing add is exact.  The
 *   adds are hardware float atomics: d_gtex must be ordinary (coarse-grained) device memory.
 *   d_guv, needs d_tex, deterministic, bit for bit: au = av = 0; for ch ascending:
 *     au = fmaf(gout[ch], fmaf(ty, (t11 - t10) - (t01 - t00), t01 - t00), au);  av = fmaf(gout[ch], bot - top, av)
 *   du = in_x ? au * (float)W : 0.0f;  dv = in_y ? av * (float)H : 0.0f.  It has the layout of srz_frameset_interpolate_grad's
 *   d_gout at n_ch = 2: the chain texture_grad -> interpolate_grad -> position_grad runs on the device.
 * Every conversion to an integer follows the float clamp (CLAMP) or the fraction (WRAP): no value of uv makes a pass read or write
 * outside its buffers.  Non-finite texels and gradients propagate as IEEE has them.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, d_vis, d_uv, d_tex (forward; backward with d_guv),
 * d_out, d_gout, or both of d_gtex and d_guv; tex_w or tex_h 0 or above SRZ_TEX_MAX_SIZE; n_ch == 0 or above SRZ_ATTR_MAX_CH;
 * tex_frames not 1 or the frame count; a mode other than SRZ_TEX_CLAMP and SRZ_TEX_WRAP; a short out_bytes; a misaligned pointer; any
 * bit of `flags` but SRZ_FUSED_CLEAR; an output that overlaps an input (d_out with d_vis, d_uv or d_tex; d_gtex or d_guv with d_vis,
 * d_uv, d_gout or d_tex) or the other output. */
#define SRZ_TEX_CLAMP 0u
#define SRZ_TEX_WRAP 1u
#define SRZ_TEX_MAX_SIZE 16384u
int srz_frameset_texture(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_uv, const float *d_tex, uint32_t tex_w,
                         uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t mode, void *d_out, size_t out_bytes, uint32_t flags,
                         void *stream);
int srz_frameset_texture_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_uv, const void *d_gout, const float *d_tex,
                              uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t mode, float *d_gtex, void *d_guv,
                              uint32_t flags, void *stream);
/* A CUBE MAP LOOKED UP BY DIRECTION over a visibility buffer, and its gradients: a float32 cube map of the caller's own (an
 * environment map, irradiance, a learned lighting probe) sampled BILINEARLY and SEAMLESSLY at the direction planes
 * srz_frameset_interpolate wrote for a three-channel attribute (normals, reflection vectors), and the backward of that lookup, to the
 * texels and to the direction.  No level of detail in this pair: the lookup over a cube's mip pyramid is
 * srz_frameset_texture_cube_mip, in the section MIPMAPPED CUBE-MAP LOOKUP below.
 * d_vis: a visibility buffer of THIS set on this ctx's shard.  d_dir: [frame][3][local_rows][width] float32 (x, y, z),
 * srz_frameset_interpolate_bytes(3) bytes; the directions need not be normalised.  d_tex and d_gtex: [tex_frames][6][n][n][n_ch]
 * float32 — face, row, column, channel; channels last — 4-byte aligned; tex_frames is 1 (every frame samples the same cube) or the
 * set's frame count; 1 <= n <= SRZ_TEX_MAX_SIZE; 1 <= n_ch <= SRZ_ATTR_MAX_CH.  d_out and d_gout: [frame][n_ch][local_rows][width]
 * float32, srz_frameset_interpolate_bytes(n_ch) bytes.  d_gdir: d_dir's shape.  Band sharding (each rank adds the partial sums of its
 * own bands), local_rows, stream semantics, asynchrony, the 16-byte alignment of the visibility buffer and every plane buffer (d_dir,
 * d_out, d_gout, d_gdir), owner and nobody, what a nobody pixel's words of d_out and d_gdir become with and without SRZ_FUSED_CLEAR,
 * and what the passes do not read or launch: all as srz_frameset_texture.  The words of d_dir and d_gout at nobody's pixels never
 * reach a result: they may hold anything.
 * THE FACES, in the order +X -X +Y -Y +Z -Z.  Face f has a normal n and in-face axes su, sv, signed unit axis vectors; a point of the
 * face is n + s su + t sv with s, t in [-1, 1], and texel (x, y) — column x, row y — has its centre at s = (2 x + 1) / N - 1,
 * t = (2 y + 1) / N - 1:
 *     face   n           su          sv
 *     +X     ( 1, 0, 0)  (0, 0, -1)  (0, -1, 0)
 *     -X     (-1, 0, 0)  (0, 0,  1)  (0, -1, 0)
 *     +Y     (0,  1, 0)  (1, 0, 0)   (0, 0,  1)
 *     -Y     (0, -1, 0)  (1, 0, 0)   (0, 0, -1)
 *     +Z     (0, 0,  1)  ( 1, 0, 0)  (0, -1, 0)
 *     -Z     (0, 0, -1)  (-1, 0, 0)  (0, -1, 0)
 * THE RULE, all of it float32, nothing fused except where fmaf is written, the divisions the IEEE division, always the exact
 * arithmetic (SRZ_OPT_APPROX_SHADE has no effect).  Per owned pixel with the direction (dx, dy, dz), a? = fabsf(d?):
 *   unsampled: a component not finite (!(fabsf(c) < INFINITY)), or max(ax, ay, az) == 0 -> every channel of out is 0 (written: the
 *              pixel has an owner), gdir = (0, 0, 0), no add
 *   major axis: x if ax >= ay && ax >= az; else y if ay >= az; else z;   face = 2 * axis + (its component > 0 ? 0 : 1)
 *   ma = fabsf(major component);  sc = the component su names, negated where su is negative;  tc likewise with sv
 *   s = sc / ma;  t = tc / ma                     (both in [-1, 1]: the division is correctly rounded and |sc|, |tc| <= ma)
 *   per axis — shown for x with s; y with t likewise:
 *     u = fmaf(s, 0.5f, 0.5f);  fx = u * (float)N - 0.5f;  x0f = floorf(fx);  tx = fx - x0f;  x0 = (int)x0f;  x1 = x0 + 1
 * Every conversion to an integer follows a float in [-0.5, N - 0.5]: x0, y0 lie in [-1, N - 1] and x1, y1 in [0, N].
 * SEAMS.  A corner texel with x or y in {-1, N} is RESOLVED onto the neighbouring face: the lookup is seamless, there is no clamp
 * mode.  Crossing in +s (x = N) or -s (x = -1), the neighbour g is the face whose normal is +su or -su, and the resolved texel is the
 * texel of g whose centre is n_g + (1 - 1 / N) n_f + t sv_f, t the corner's own; crossing in +-t likewise with su and sv exchanged.
 * In integers that is a fixed map per (face, side) — one index of the neighbour becomes 0 or N - 1, the other is the index i along
 * the edge, kept or mirrored (N - 1 - i) — and the passes use that table of 24 rows, no float reprojection:
 *     face   x = -1         x = N          y = -1             y = N
 *     +X     +Z (N-1, i)    -Z (0, i)      +Y (N-1, N-1-i)    -Y (N-1, i)
 *     -X     -Z (N-1, i)    +Z (0, i)      +Y (0, i)          -Y (0, N-1-i)
 *     +Y     -X (i, 0)      +X (N-1-i, 0)  -Z (N-1-i, 0)      +Z (i, 0)
 *     -Y     -X (N-1-i, N-1) +X (i, N-1)   +Z (i, N-1)        -Z (N-1-i, N-1)
 *     +Z     -X (N-1, i)    +X (0, i)      +Y (i, N-1)        -Y (i, 0)
 *     -Z     +X (N-1, i)    -X (0, i)      +Y (N-1-i, 0)      -Y (N-1-i, N-1)
 *   (the resolved (column, row); i = the corner's row for the x sides, its column for the y sides).
 *   A corner outside in BOTH axes — at most one per lookup, and only within half a texel of a cube vertex, where three faces meet and
 *   no fourth texel exists — has its row clamped into [0, N - 1] first and then crosses in x.  That is a CHOICE: within that half
 *   texel the lookup is continuous only up to the spread of the three vertex texels; everywhere else, across every edge, a direction
 *   gives the same word through either adjacent face.
 * FORWARD, deterministic, bit for bit: per channel, with t_rc the resolved texel of corner (y_r, x_c),
 *   top = fmaf(tx, t01 - t00, t00);  bot = fmaf(tx, t11 - t10, t10);  out = fmaf(ty, bot - top, top)
 * BACKWARD: d_gout, the same d_dir and d_vis; at least one of d_gtex and d_gdir is non-null.
 *   d_gtex (d_tex itself may be null when only d_gtex is asked for): srz_frameset_texture_grad's four weights w_rc, the float32
 *   product w_rc * gout[ch] ADDED at the RESOLVED texels (ft = 0 when tex_frames == 1): a pixel near an edge adds into both faces, and
 *   two corners that coincide (N == 1; the clamped corner at a vertex) both add.  THE ORDER OF THE ADDS IS UNSPECIFIED, each add
 *   rounds, so d_gtex is NOT BIT-REPRODUCIBLE between launches: srz_frameset_texture_grad's bound, n 2^-24 / (1 - n 2^-24) * sum |term|
 *   with n contributing adds, exact at n = 1; hardware float atomics, so d_gtex must be ordinary (coarse-grained) device memory.
 *   d_gdir, needs d_tex, deterministic, bit for bit: au, av exactly as srz_frameset_texture_grad's d_guv sums over the four
 *   resolved texels, then
 *     gs = au * (0.5f * (float)N);  gt = av * (0.5f * (float)N);  inv = 1.0f / ma
 *     g_sc = gs * inv;  g_tc = gt * inv;  g_ma = -(fmaf(gs, s, gt * t) * inv)
 *     gdir[sc's axis] = g_sc, negated where su is negative;  gdir[tc's axis] = g_tc, negated where sv is negative
 *     gdir[major axis] = (major component > 0 ? g_ma : -g_ma)
 *   (the face and the texels are held fixed; the lookup does not depend on the direction's length, so dot(gdir, d) is 0 up to
 *   rounding).  It has the layout of srz_frameset_interpolate_grad's d_gout at n_ch = 3: the chain texture_cube_grad ->
 *   interpolate_grad -> corner_attr_grad -> mesh_normals_grad runs on the device.
 * SUBNORMALS are numbers: the library is built without flush-to-zero (binary32 denormals on, the division the correctly rounded
 * one), so a direction of subnormal components is sampled like any other and s, t are what IEEE division gives; inv = 1.0f / ma
 * overflows to +inf for ma below 2^-128, and gdir is then inf or NaN as IEEE has it.  Non-finite texels and gradients propagate as
 * IEEE has them; no value of the direction makes a pass read or write outside its buffers.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, d_vis, d_dir, d_tex (forward; backward with
 * d_gdir), d_out, d_gout, or both of d_gtex and d_gdir; n == 0 or above SRZ_TEX_MAX_SIZE; n_ch == 0 or above SRZ_ATTR_MAX_CH;
 * tex_frames not 1 or the frame count; a short out_bytes; a misaligned pointer; any bit of `flags` but SRZ_FUSED_CLEAR; an output
 * that overlaps an input (d_out with d_vis, d_dir or d_tex; d_gtex or d_gdir with d_vis, d_dir, d_gout or d_tex) or the other
 * output. */
int srz_frameset_texture_cube(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_dir, const float *d_tex, uint32_t n,
                              uint32_t n_ch, uint32_t tex_frames, void *d_out, size_t out_bytes, uint32_t flags, void *stream);
int srz_frameset_texture_cube_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_dir, const void *d_gout,
                                   const float *d_tex, uint32_t n, uint32_t n_ch, uint32_t tex_frames, float *d_gtex, void *d_gdir,
                                   uint32_t flags, void *stream);
/* BLINN-PHONG LIGHTING UNDER POINT LIGHTS over a visibility buffer, for the caller's own planes, and its gradients: the link between
 * the interpolated normals, positions and albedo and an image loss.  The lights, the eye and the material are device data with a
 * gradient of their own.  This pass is for caller data and reproduces NOTHING of the reference or of the built-in shaders
 * (srz_frameset_shade_visibility): DELIBERATELY DIFFERENT are the true 1 / r² attenuation (not the x/y distance), the NORMALISED half
 * vector, the albedo on the ambient and diffuse terms only, and NO CLAMP and no scale by 255 (the caller's units; a clamp would cut
 * the gradient).
 * d_vis: a visibility buffer of THIS set on this ctx's shard.  d_nrm, d_pos, d_kd (forward and backward: may be NULL, albedo
 * (1, 1, 1)), d_out, d_gout, d_gnrm, d_gpos, d_gkd: [frame][3][local_rows][width] float32, srz_frameset_interpolate_bytes(3) bytes each —
 * what srz_frameset_interpolate, _texture or _gbuffer write.  d_par and d_gpar: [par_frames][SRZ_LIGHT_PAR(n_lights)] float32 in device
 * memory, 4-byte aligned, a parameter frame being eye[3] ka[3] ks[3], then n_lights x {pos[3], intensity[3]} (srz_light's layout);
 * par_frames is 1 (every frame shares the one parameter frame) or the set's frame count; 1 <= n_lights <= SRZ_LIGHT_MAX.  p: the
 * specular exponent, an INTEGER in [1, 256], the same for every frame, a host argument (so a bad one is refused without reading device
 * memory); there is no gradient to p.  Band sharding, local_rows, stream semantics, asynchrony, the 16-byte alignment of the visibility
 * buffer and every plane buffer, owner and nobody (id 0, the bare class bit, an index outside the frame's triangles), what a nobody
 * pixel's words of the output planes become with and without SRZ_FUSED_CLEAR (zeros; untouched), and what the passes do not read or
 * launch: all as srz_frameset_texture_cube.  The words of the input planes at nobody's pixels never reach a result.
 * THE RULE, all of it float32, nothing fused except where fmaf is written, / and sqrtf the correctly rounded ones, always the exact
 * arithmetic (SRZ_OPT_APPROX_SHADE has no effect).  dot(a, b) = fmaf(ax, bx, fmaf(ay, by, az * bz)); a vector times a scalar is three
 * products.  Per owned pixel with the normal n, the position P, the albedo kd:
 *   nn = dot(n, n);  lit = nn > 0 && nn < INFINITY;   not lit -> out = (0, 0, 0) (written), every gradient of the pixel 0, no term
 *   inl = 1 / sqrtf(nn);  N = n * inl
 *   V = eye - P;  vv = dot(V, V);  view = vv > 0 && vv < INFINITY;  iv = 1 / sqrtf(vv);  Vd = view ? V * iv : (0, 0, 0)
 *   acc = (0, 0, 0);  for each light in order, position lpos, intensity I:
 *     Lv = lpos - P;  r2 = dot(Lv, Lv);  if !(r2 > 0 && r2 < INFINITY) the light is SKIPPED at this pixel (no term, no gradient)
 *     ir = 1 / sqrtf(r2);  Ld = Lv * ir;  att = 1 / r2
 *     cdr = dot(N, Ld);  cd = cdr > 0 ? cdr : 0
 *     Hs = Ld + Vd;  h2 = dot(Hs, Hs);  spec = view && h2 > 0
 *     spec:  ih = 1 / sqrtf(h2);  H = Hs * ih;  csr = dot(N, H);  cs = csr > 0 ? csr : 0;  sp = powi(cs, p);   else sp = 0
 *     E_c = I_c * att
 *     acc_c = acc_c + (kd_c * fmaf(E_c, cd, ka_c * I_c) + (ks_c * E_c) * sp)
 *   out_c = acc_c
 * powi(x, n): r = 1, b = x in binary64; while n: if (n & 1) r = r * b;  b = b * b;  n >>= 1;  rounded once to binary32 (powi(x, 0) = 1).
 * BACKWARD: the exact derivative of the rule with its branches held, in THIS order of operations (g = gout of the pixel; a not-lit or
 * nobody's pixel gives zeros and no term).  gN = gVd = gP = gkd = tka = tks = (0, 0, 0);  for each light that is not skipped, in order:
 *     gk_c = g_c * kd_c;  gs_c = g_c * ks_c
 *     gkd_c = gkd_c + g_c * fmaf(E_c, cd, ka_c * I_c)
 *     tka_c = tka_c + gk_c * I_c;   tks_c = tks_c + (g_c * E_c) * sp
 *     tI_c  = g_c * (kd_c * fmaf(att, cd, ka_c) + (ks_c * att) * sp)                        (the light's intensity term)
 *     ge_c  = g_c * fmaf(kd_c, cd, ks_c * sp)
 *     g_cd = cdr > 0 ? dot(gk, E) : 0;   g_sp = dot(gs, E);   g_att = dot(ge, I)
 *     gLd = g_cd * N;   gN_c = gN_c + g_cd * Ld_c
 *     if spec && csr > 0:  g_cs = g_sp * ((float)p * powi(cs, p - 1));  gH = g_cs * N;  gN_c = gN_c + g_cs * H_c;  d = dot(gH, H)
 *                          gHs_c = (gH_c - H_c * d) * ih;   gLd_c = gLd_c + gHs_c;   gVd_c = gVd_c + gHs_c
 *     d = dot(gLd, Ld);   w = 2 * -((g_att * att) * att)
 *     tL_c = fmaf(Lv_c, w, (gLd_c - Ld_c * d) * ir)                                         (the light's position term)
 *     gP_c = gP_c - tL_c
 *   then:  view:  d = dot(gVd, Vd);  tE_c = (gVd_c - Vd_c * d) * iv;  gP_c = gP_c - tE_c;    else tE = (0, 0, 0)      (the eye's term)
 *          d = dot(gN, N);  gn_c = (gN_c - N_c * d) * inl
 *   d_gnrm = gn, d_gpos = gP, d_gkd = gkd: per pixel, deterministic, bit for bit.  Each may be NULL, not all four outputs; d_gkd must be
 *   NULL when d_kd is.  They have the layouts srz_frameset_interpolate_grad and srz_frameset_texture_grad take as d_gout.
 *   d_gpar (needs d_work, at least srz_frameset_light_work_bytes bytes, 4-byte aligned, scratch: what it holds afterwards is
 *   unspecified) is WRITTEN, not added into: entry k of a frame's row is the sum over the frame's lit pixels on this shard of the
 *   pixel's float32 term — eye: tE; ka: tka; ks: tks (each summed over the lights first, in light order); a light's pos: tL, its
 *   intensity: tI (0 where the light is skipped) — in a FIXED tree, no atomics: a pixel (x, y) of a 32 x 32 tile belongs to lane
 *   (y % 8) * 8 + x % 32 / 4 of wave y % 32 / 8; a lane adds its up to four pixels' terms left to right, from +0; the 64 lanes of a wave
 *   are summed by the butterfly v = v + v[lane ^ o], o = 32, 16, 8, 4, 2, 1; the four waves as ((w0 + w1) + w2) + w3; a frame's tiles
 *   in tile order (bands, then columns), from +0; and with par_frames == 1 the frames' rows — each exactly the row the same call with
 *   per-frame parameters of the same values writes — in frame order, from +0.  So d_gpar is BIT-REPRODUCIBLE for a given shard
 *   layout: two launches give the same words, and with one lit pixel in all it is that pixel's term (a term of -0 comes out +0).
 *   Against the exact sum of the terms it lies within n 2^-24 / (1 - n 2^-24) * sum |term|, n the contributing pixels of the entry:
 *   the bound of any summation tree.  An entry no pixel contributes to is +0.  Ranks each write the sums of their own bands.
 * SUBNORMALS are numbers, as in srz_frameset_texture_cube; non-finite albedo, intensities and gradients propagate as IEEE has them;
 * no value of any plane makes a pass read or write outside its buffers.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, d_vis, d_nrm, d_pos, d_par, d_out, d_gout, or all
 * of d_gnrm, d_gpos, d_gkd, d_gpar; n_lights == 0 or above SRZ_LIGHT_MAX; par_frames not 1 or the frame count; p outside [1, 256]; a
 * short out_bytes, or work_bytes with d_gpar; a misaligned pointer; any bit of `flags` but SRZ_FUSED_CLEAR; an output (d_work with
 * d_gpar counts as one) that overlaps an input or another output; d_gkd without d_kd; d_gpar without d_work. */
#define SRZ_LIGHT_MAX 8
/* floats of one parameter frame: eye[3] ka[3] ks[3], then n_lights x {pos[3], intensity[3]} (srz_light's layout) */
#define SRZ_LIGHT_PAR(n_lights) (9u + 6u * (n_lights))
int srz_frameset_light(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const void *d_kd,
                       const float *d_par, uint32_t n_lights, uint32_t par_frames, uint32_t p, void *d_out, size_t out_bytes, uint32_t flags,
                       void *stream);
size_t srz_frameset_light_work_bytes(srz_ctx *ctx, srz_frameset *fs, uint32_t n_lights);
int srz_frameset_light_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const void *d_kd,
                            const float *d_par, uint32_t n_lights, uint32_t par_frames, uint32_t p, const void *d_gout, void *d_gnrm,
                            void *d_gpos, void *d_gkd, float *d_gpar, void *d_work, size_t work_bytes, uint32_t flags, void *stream);
/* COOK-TORRANCE SHADING UNDER POINT LIGHTS over a visibility buffer, for the caller's own planes, and its gradients: the
 * metallic-roughness material the chain's other passes feed — a GGX normal distribution, the separable Schlick-Smith visibility and
 * Schlick's Fresnel term — with PER-PIXEL roughness and metallic, both with a gradient.  A sibling of srz_frameset_light, not a change
 * to it; like it, for caller data, nothing of the reference or of the built-in shaders, no clamp of the result, the caller's units.
 * d_vis: a visibility buffer of THIS set on this ctx's shard.  d_nrm, d_pos, d_base (forward and backward: may be NULL, base colour
 * (1, 1, 1)), d_out, d_gout, d_gnrm, d_gpos, d_gbase: [frame][3][local_rows][width] float32, srz_frameset_interpolate_bytes(3) bytes
 * each.  d_mat (required) and d_gmat: [frame][2][local_rows][width], srz_frameset_interpolate_bytes(2) bytes: plane 0 the roughness,
 * plane 1 the metallic.  d_par and d_gpar: [par_frames][SRZ_MICROFACET_PAR(n_lights)] float32 in device memory, 4-byte aligned, a
 * parameter frame being eye[3] amb[3], then n_lights x {pos[3], intensity[3]} (srz_light's layout); par_frames is 1 or the set's frame
 * count; 1 <= n_lights <= SRZ_LIGHT_MAX.  Band sharding, local_rows, stream semantics, asynchrony, the 16-byte alignment of the
 * visibility buffer and every plane buffer, owner and nobody, what a nobody pixel's words of the output planes become with and without
 * SRZ_FUSED_CLEAR (zeros; untouched), and what the passes do not read or launch: all as srz_frameset_light.  The words of the input
 * planes at nobody's pixels never reach a result.
 * THE RULE, all of it float32, nothing fused except where fmaf is written, / and sqrtf the correctly rounded ones, always the exact
 * arithmetic (SRZ_OPT_APPROX_SHADE has no effect); no transcendental function.  dot, the test l_pos(x) = x > 0 && x < INFINITY and
 * 1 / sqrtf(x) (two roundings) as in srz_frameset_light.  INV_PI = 0x1.45f306p-2f, RMIN = 0.0625f.  Per owned pixel with the normal n,
 * the position P, the base colour base, the material (mat0, mat1):
 *   nn, lit, inl, N, V, vv, view, iv, Vd: exactly as srz_frameset_light          (not lit -> out = (0, 0, 0) (written), no gradient, no term)
 *   r = mat0;  rc = r > RMIN ? (r < 1 ? r : 1) : RMIN;  r_in = r > RMIN && r < 1                         (a NaN: RMIN, no gradient)
 *   m = mat1;  mc = m > 0 ? (m < 1 ? m : 1) : 0;        m_in = m > 0 && m < 1                            (a NaN: 0, no gradient)
 *   al = rc * rc;  a2 = al * al;  k = 0.5f * al;  omk = 1 - k;  om = 1 - mc
 *   F0_c = fmaf(mc, base_c - 0.04f, 0.04f);  cdif_c = base_c * om
 *   nv = view ? dot(N, Vd) : 0
 *   acc = (0, 0, 0);  for each light in order, position lpos, intensity I:
 *     Lv = lpos - P;  r2 = dot(Lv, Lv);  if !l_pos(r2) the light is SKIPPED at this pixel (no term, no gradient)
 *     ir = 1 / sqrtf(r2);  Ld = Lv * ir;  att = 1 / r2;  E_c = I_c * att
 *     nl = dot(N, Ld);  if !(nl > 0) the light adds nothing at this pixel (no term, no gradient)
 *     Hs = Ld + Vd;  h2 = dot(Hs, Hs);  spec = view && h2 > 0 && nv > 0
 *     spec:  ih = 1 / sqrtf(h2);  H = Hs * ih
 *            nhr = dot(N, H);   nh = nhr > 0 ? (nhr < 1 ? nhr : 1) : 0;   vhr = dot(Vd, H);  vh = vhr > 0 ? (vhr < 1 ? vhr : 1) : 0
 *            t = fmaf(nh * nh, a2 - 1, 1);  tt = t * t;  D = (a2 * INV_PI) / tt
 *            gl = fmaf(nl, omk, k);  gv = fmaf(nv, omk, k);  Vs = 0.25f / (gl * gv);  DV = D * Vs
 *            x = 1 - vh;  x2 = x * x;  x4 = x2 * x2;  x5 = x4 * x;  F_c = fmaf(1 - F0_c, x5, F0_c)
 *            f_c = fmaf(cdif_c * INV_PI, 1 - F_c, F_c * DV)
 *     else:  f_c = cdif_c * INV_PI
 *     acc_c = acc_c + (f_c * E_c) * nl
 *   out_c = fmaf(amb_c, base_c, acc_c)
 * RMIN keeps D at or below INV_PI * 2^16; the separable visibility divides by no cosine (gl, gv >= k >= 2^-9); every clamp is a pair
 * of comparisons, so a NaN takes the stated branch.
 * BACKWARD: the exact derivative of the rule with its branches and clamps held, in THIS order of operations (g = gout of the pixel; a
 * not-lit or nobody's pixel gives zeros and no term).  gN = gVd = gP = (0, 0, 0);  g_a2 = g_k = g_nv = g_om = g_mc = 0;
 * gb_c = g_c * amb_c;  tamb_c = g_c * base_c (the amb term);  for each light that adds something, in order:
 *     gq = g_c * nl;  gf_c = gq * E_c;  ge_c = gq * f_c;  q_c = f_c * E_c;  tI_c = ge_c * att      (the light's intensity term)
 *     g_nl = dot(g, q);  g_att = dot(ge, I);  gLd = (0, 0, 0)
 *     spec:  gcd_c = (gf_c * (1 - F_c)) * INV_PI;  gF_c = gf_c * (DV - cdif_c * INV_PI);  gF0_c = gF_c * (1 - x5)
 *            gb_c = gb_c + gF0_c * mc;   g_mc = g_mc + dot(gF0, base - 0.04f)
 *            gDV = dot(gf, F);  gD = gDV * Vs;  gVs = gDV * D
 *            gx = dot(gF, 1 - F0) * (5 * x4);   g_vhr = vhr > 0 && vhr < 1 ? -gx : 0
 *            gw = -(gVs * Vs);  ggl = gw / gl;  ggv = gw / gv
 *            g_nl = fmaf(ggl, omk, g_nl);  g_nv = fmaf(ggv, omk, g_nv);  g_k = g_k + fmaf(ggl, 1 - nl, ggv * (1 - nv))
 *            g_t = -((2 * (gD * D)) / t);  g_a2 = g_a2 + fmaf(g_t, nh * nh, gD * (INV_PI / tt))
 *            g_nhr = nhr > 0 && nhr < 1 ? g_t * ((2 * nh) * (a2 - 1)) : 0
 *            gH_c = fmaf(g_nhr, N_c, g_vhr * Vd_c);  gN_c = gN_c + g_nhr * H_c;  gVd_c = gVd_c + g_vhr * H_c
 *            d = dot(gH, H);  gHs_c = (gH_c - H_c * d) * ih;  gLd_c = gHs_c;  gVd_c = gVd_c + gHs_c
 *     else:  gcd_c = gf_c * INV_PI
 *     g_om = g_om + dot(gcd, base);  gb_c = gb_c + gcd_c * om
 *     gLd_c = fmaf(g_nl, N_c, gLd_c);  gN_c = gN_c + g_nl * Ld_c
 *     d = dot(gLd, Ld);  w = 2 * -((g_att * att) * att)
 *     tL_c = fmaf(Lv_c, w, (gLd_c - Ld_c * d) * ir)                                                 (the light's position term)
 *     gP_c = gP_c - tL_c
 *   then:  view:  gN_c = fmaf(g_nv, Vd_c, gN_c);  gVd_c = fmaf(g_nv, N_c, gVd_c);  d = dot(gVd, Vd)
 *                 tE_c = (gVd_c - Vd_c * d) * iv;  gP_c = gP_c - tE_c;                 else tE = (0, 0, 0)        (the eye's term)
 *          d = dot(gN, N);  gn_c = (gN_c - N_c * d) * inl
 *          g_al = fmaf(g_a2, 2 * al, 0.5f * g_k);  gmat0 = r_in ? g_al * (2 * rc) : 0;  gmat1 = m_in ? g_mc - g_om : 0
 *   d_gnrm = gn, d_gpos = gP, d_gbase = gb, d_gmat = (gmat0, gmat1): per pixel, deterministic, bit for bit.  Each may be NULL, not all
 *   five outputs; d_gbase must be NULL when d_base is.
 *   d_gpar (needs d_work, at least srz_frameset_microfacet_work_bytes bytes, 4-byte aligned, scratch) is WRITTEN, not added into:
 *   entry k of a frame's row is the sum over the frame's lit pixels on this shard of the pixel's float32 term — eye: tE; amb: tamb; a
 *   light's pos: tL, its intensity: tI (0 where the light adds nothing) — in srz_frameset_light_grad's FIXED tree, word for word (the
 *   lane's four pixels, the xor butterfly, the four waves, the tiles in order, and with par_frames == 1 the frames in order): so d_gpar
 *   is BIT-REPRODUCIBLE for a given shard layout, with one lit pixel in all it is that pixel's term (a term of -0 comes out +0), and
 *   against the exact sum of the terms it lies within n 2^-24 / (1 - n 2^-24) * sum |term|, n the contributing pixels of the entry.
 *   An entry no pixel contributes to is +0.  Ranks each write the sums of their own bands; a rank without bands writes +0.
 * SUBNORMALS are numbers; non-finite base colours, intensities and gradients propagate as IEEE has them; no value of any plane makes
 * a pass read or write outside its buffers.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, d_vis, d_nrm, d_pos, d_mat, d_par, d_out, d_gout,
 * or all of d_gnrm, d_gpos, d_gbase, d_gmat, d_gpar; n_lights == 0 or above SRZ_LIGHT_MAX; par_frames not 1 or the frame count; a
 * short out_bytes, or work_bytes with d_gpar; a misaligned pointer; any bit of `flags` but SRZ_FUSED_CLEAR; an output (d_work with
 * d_gpar counts as one) that overlaps an input or another output; d_gbase without d_base; d_gpar without d_work. */
/* floats of one parameter frame: eye[3] amb[3], then n_lights x {pos[3], intensity[3]} (srz_light's layout) */
#define SRZ_MICROFACET_PAR(n_lights) (6u + 6u * (n_lights))
int srz_frameset_microfacet(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const void *d_base,
                            const void *d_mat, const float *d_par, uint32_t n_lights, uint32_t par_frames, void *d_out, size_t out_bytes,
                            uint32_t flags, void *stream);
size_t srz_frameset_microfacet_work_bytes(srz_ctx *ctx, srz_frameset *fs, uint32_t n_lights);
int srz_frameset_microfacet_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos,
                                 const void *d_base, const void *d_mat, const float *d_par, uint32_t n_lights, uint32_t par_frames,
                                 const void *d_gout, void *d_gnrm, void *d_gpos, void *d_gbase, void *d_gmat, float *d_gpar, void *d_work,
                                 size_t work_bytes, uint32_t flags, void *stream);
/* TANGENT-SPACE NORMAL MAPPING over a visibility buffer, for the caller's own planes, and its gradients: the interpolated normal, the
 * interpolated tangent with its handedness (srz_mesh_tangents through srz_sceneset_corner_attr and srz_frameset_interpolate at 4
 * channels) and a tangent-space normal m, AS THE CALLER DECODED IT (srz_frameset_texture's output, or a learned map that stores signed
 * values), give the unit shading normal srz_frameset_light and srz_frameset_texture_cube take.  Nothing of the built-in BUMP shader.
 * d_vis: a visibility buffer of THIS set on this ctx's shard.  d_nrm, d_m, d_out, d_gout, d_gnrm, d_gm: [frame][3][local_rows][width]
 * float32, srz_frameset_interpolate_bytes(3) bytes each; d_tan, d_gtan: [frame][4][local_rows][width], _interpolate_bytes(4).  Band
 * sharding, local_rows, stream semantics, asynchrony, the 16-byte alignment, owner and nobody, what a nobody pixel's words of the
 * output planes become with and without SRZ_FUSED_CLEAR (zeros; untouched): all as srz_frameset_light.  The words of the input planes
 * at nobody's pixels never reach a result.
 * THE RULE, all of it float32, nothing fused except where fmaf is written, / and sqrtf the correctly rounded ones, always the exact
 * arithmetic (SRZ_OPT_APPROX_SHADE has no effect).  dot(a, b) = fmaf(ax, bx, fmaf(ay, by, az * bz));  cross(u, w) = (u.y w.z - u.z w.y,
 * u.z w.x - u.x w.z, u.x w.y - u.y w.x);  a vector times a scalar is three products.  Per owned pixel with the normal n, the tangent t
 * (t.xyz, t.w) and m:
 *   nn = dot(n, n);  !(nn > 0 && nn < INFINITY) -> out = (0, 0, 0) (written), every gradient of the pixel 0     (light: not lit)
 *   inl = 1 / sqrtf(nn);  N = n * inl
 *   d = dot(N, t.xyz);  Tp = t.xyz - N * d;  tt = dot(Tp, Tp)
 *   !(tt > 0 && tt < INFINITY) -> out = N                                          (no frame: the unperturbed normal)
 *   it = 1 / sqrtf(tt);  T = Tp * it;  hw = t.w < 0 ? -1 : +1;  B = cross(N, T) * hw
 *   R_c = fmaf(m.x, T_c, fmaf(m.y, B_c, m.z * N_c));  rr = dot(R, R)
 *   !(rr > 0 && rr < INFINITY) -> out = N
 *   ir = 1 / sqrtf(rr);  out = R * ir
 * BACKWARD: the exact derivative of the rule with its branches held, in THIS order of operations (g = gout of the pixel):
 *   out = R * ir:   dq = dot(g, out);  gR_c = (g_c - out_c * dq) * ir
 *                   gm = (dot(gR, T), dot(gR, B), dot(gR, N))
 *                   gT_c = m.x * gR_c;  gC_c = (m.y * gR_c) * hw;  gN_c = m.z * gR_c
 *                   gN = gN + cross(T, gC);  gT = gT + cross(gC, N)
 *                   dT = dot(gT, T);  gTp_c = (gT_c - T_c * dT) * it;  gd = -dot(gTp, N)
 *                   gN_c = (gN_c - gTp_c * d) + gd * t_c;   gt_c = gTp_c + gd * N_c;   gt.w = +0
 *   out = N:        gN = g;  gt = (0, 0, 0, 0);  gm = (0, 0, 0)
 *   then both:      dn = dot(gN, N);  gn_c = (gN_c - N_c * dn) * inl
 *   d_gnrm = gn, d_gtan = gt (four planes, the w plane +0: there is no gradient to the handedness), d_gm = gm: per pixel,
 *   deterministic, bit for bit.  Each may be NULL, not all three.  d_gtan has the layout srz_frameset_interpolate_grad takes as d_gout
 *   at 4 channels, d_gm the one srz_frameset_texture_grad takes.
 * SUBNORMALS are numbers; non-finite m and gradients propagate as IEEE has them (a NaN in m makes rr a NaN: out = N); no value of any
 * plane makes a pass read or write outside its buffers.  No LDS, no atomics.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, d_vis, d_nrm, d_tan, d_m, d_out, d_gout, or all of
 * d_gnrm, d_gtan, d_gm; a short out_bytes; a misaligned pointer; any bit of `flags` but SRZ_FUSED_CLEAR; an output that overlaps an
 * input or another output. */
int srz_frameset_normal_map(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_tan, const void *d_m,
                            void *d_out, size_t out_bytes, uint32_t flags, void *stream);
int srz_frameset_normal_map_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_tan, const void *d_m,
                                 const void *d_gout, void *d_gnrm, void *d_gtan, void *d_gm, uint32_t flags, void *stream);
/* SHADOW-MAP LOOKUP over a visibility buffer, and its gradients: PERCENTAGE-CLOSER FILTERING of a float32 depth map of the caller's
 * own at caller coordinates — the four texels around (sx, sy) are each COMPARED with the pixel's depth sd, and the four results are
 * blended bilinearly — and the backward of that, to the map and to the coordinates.  `width` turns the hard depth test into a linear
 * ramp, so that a gradient exists in depth.  The pieces a shadow needs besides are passes that exist: a light's view is another
 * frameset, plane 0 of ITS visibility buffer is the depth map (+inf where nobody is: lit), srz_frameset_position_grad with d_gz
 * makes that map differentiable in the occluders' positions, and the light set's screen positions, read as a [T][3][3] per-corner attribute and run through
 * srz_frameset_interpolate over the CAMERA set, are every camera pixel's coordinates in the map.
 * d_vis: a visibility buffer of THIS (the camera's) set on this ctx's shard.  d_sc: [frame][3][local_rows][width] float32 — sx, sy,
 * sd: srz_frameset_interpolate's output at three channels.  sx and sy are in map texel units with the texel CENTRES ON THE INTEGERS:
 * a render samples a pixel at its integer corner, so texel (x, y) of a depth plane is the depth at screen (x, y) and fx = sx, with no
 * -0.5 (srz_frameset_texture's grid has the centres at i + 0.5).  sd is in the map's depth units.  d_map and d_gmap:
 * [map_frames][map_h][map_w] float32, dense, 4-byte aligned; map_frames is 1 (every frame looks up the same map) or the set's frame
 * count; 1 <= map_w, map_h <= SRZ_TEX_MAX_SIZE.  The map is WHOLE, never band-sharded: on a sharded ctx the caller gathers it, as a
 * texture.  bias, width: host floats, finite, width >= 0 (0: the hard test); neither gets a gradient.  d_out and d_gout:
 * [frame][1][local_rows][width] float32, srz_frameset_interpolate_bytes(1) bytes; d_gsc: d_sc's shape.  Owner and nobody, the fused
 * clear (a nobody pixel's words of d_out and d_gsc are 0 with SRZ_FUSED_CLEAR (frame flags | flags), else left untouched), band
 * sharding (each rank adds the partial sums of its own bands to d_gmap), local_rows, stream semantics, asynchrony and the 16-byte
 * alignment of the visibility buffer and every plane buffer (d_sc, d_out, d_gout, d_gsc): all as srz_frameset_texture.  The words of
 * d_sc and d_gout at nobody's pixels never reach a result.
 * THE RULE, all of it float32, nothing fused except where fmaf is written, `/` the IEEE division, always the exact arithmetic
 * (SRZ_OPT_APPROX_SHADE has no effect).  Per owned pixel:
 *   unsampled: sx, sy or sd not finite (!(fabsf(s) < INFINITY)) -> out = 1.0f (written: the pixel has an owner; no occluder is
 *              known: lit), gsc = (0, 0, 0), no add
 *   per axis — shown for x with sx and W = map_w; y with sy and H = map_h likewise:
 *     in_x = sx > -1.0f && sx < (float)W;   fx = fminf(fmaxf(sx, -1.0f), (float)W)
 *     x0f = floorf(fx);  tx = fx - x0f;  x0 = (int)x0f;  x1 = x0 + 1                  (x0 in [-1, W], x1 in [0, W + 1])
 *   corner (r, c) OUTSIDE the map (x_c < 0 || x_c >= W || y_r < 0 || y_r >= H): v = 1.0f, not moving; never read, never added to
 *     (beyond the map nothing is known to occlude: the result fades to lit across the map's last texel)
 *   corner inside:  m = map[fm][y_r][x_c] (fm = 0 when map_frames == 1);  e = (m + bias) - sd
 *     width == 0:  v = e >= 0.0f ? 1.0f : 0.0f;  not moving                            (a NaN gives 0; m = +inf gives 1)
 *     width  > 0:  q = e / width + 0.5f;  v = fminf(fmaxf(q, 0.0f), 1.0f) (a NaN gives 0);  moving = q > 0.0f && q < 1.0f
 * FORWARD, deterministic, bit for bit:
 *   top = fmaf(tx, v01 - v00, v00);  bot = fmaf(tx, v11 - v10, v10);  out = fmaf(ty, bot - top, top)
 * BACKWARD: d_gout, the same d_sc, d_map and d_vis; at least one of d_gmap and d_gsc is non-null.  With g = gout:
 *   gsx = in_x ? g * fmaf(ty, (v11 - v10) - (v01 - v00), v01 - v00) : 0.0f;   gsy = in_y ? g * (bot - top) : 0.0f
 *   w00 = (1.0f - tx) * (1.0f - ty), w01 = tx * (1.0f - ty), w10 = (1.0f - tx) * ty, w11 = tx * ty
 *   d_rc = moving_rc ? (w_rc * g) / width : 0.0f;   gsd = -(((d00 + d01) + d10) + d11)
 *   d_gsc = (gsx, gsy, gsd): per pixel, deterministic, bit for bit; the layout srz_frameset_interpolate_grad takes as d_gout at
 *   n_ch = 3 (the hard test leaves gsd = -0.0f: the sum of four +0 terms, negated).
 *   d_gmap: for every MOVING corner of every sampled pixel d_rc is ADDED to gmap[fm][y_r][x_c] (two corners of one pixel never
 *   coincide: x1 = x0 + 1 always).  width == 0 is allowed and adds nothing.  The caller zeroes the buffer, or accumulates over
 *   several calls.  THE ORDER OF THE ADDS IS UNSPECIFIED, each add rounds, so d_gmap is NOT BIT-REPRODUCIBLE between launches, like
 *   d_gtex: with n contributing adds an element lies within n 2^-24 / (1 - n 2^-24) * sum |term| of the exact sum of the float32
 *   terms; an element with one contributing add is exact.  The adds are hardware float atomics: d_gmap must be ordinary
 *   (coarse-grained) device memory.
 * Every conversion to an integer follows the float clamp, and a corner is touched only where its own coordinates lie inside the map:
 * no value of d_sc makes a pass read or write outside its buffers.  Non-finite texels and gradients propagate as IEEE has them
 * through the comparisons above.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, d_vis, d_sc, d_map, d_out (forward), d_gout
 * (backward), or both of d_gmap and d_gsc; map_w or map_h 0 or above SRZ_TEX_MAX_SIZE; map_frames not 1 or the frame count; a bias or
 * width that is not finite; width < 0; a short out_bytes; a misaligned pointer; any bit of `flags` but SRZ_FUSED_CLEAR; an output that
 * overlaps an input (d_out with d_vis, d_sc or d_map; d_gmap or d_gsc with d_vis, d_sc, d_gout or d_map) or the other output. */
int srz_frameset_shadow(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_sc, const float *d_map, uint32_t map_w,
                        uint32_t map_h, uint32_t map_frames, float bias, float width, void *d_out, size_t out_bytes, uint32_t flags,
                        void *stream);
int srz_frameset_shadow_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_sc, const void *d_gout, const float *d_map,
                             uint32_t map_w, uint32_t map_h, uint32_t map_frames, float bias, float width, float *d_gmap, void *d_gsc,
                             uint32_t flags, void *stream);
/* MIPMAPPED TEXTURE SAMPLING over a visibility buffer, and its gradients: the TRILINEAR lookup over a mip pyramid of the caller's
 * texture that goes with the bilinear lookup above, its level chosen from the screen-space derivatives of uv.  Three pieces: the
 * pyramid (build, and fold: its backward), the derivatives of an interpolated attribute, the lookup and its backward.  All of it
 * float32, nothing fused except where fmaf is written, division and sqrtf the IEEE operations (SRZ_OPT_APPROX_SHADE has no effect).
 * THE PYRAMID.  Level 0 is the caller's texture [tex_frames][H][W][C] as srz_frameset_texture takes it.  Level l + 1 exists iff
 * (w_l > 1 or h_l > 1) and w_l is even or 1 and h_l is even or 1; then w_(l+1) = max(1, w_l / 2), h_(l+1) likewise — an odd extent
 * ends the chain (100 x 70: 2 levels; 96 x 64: 6, down to 3 x 2; 32 x 8: 6, ... 4 x 1, 2 x 1, 1 x 1; 5 x 7 and 1 x 1: 1).
 * srz_texture_mip_levels: the levels including level 0 (1024^2: 11, 16384^2: SRZ_TEX_MAX_LEVELS); 0 for an extent of 0 or above
 * SRZ_TEX_MAX_SIZE.  srz_texture_mip_bytes: the bytes of levels 1 .. n_levels - 1, LEVEL-MAJOR — level l is [tex_frames][h_l][w_l][C]
 * float32, the levels one after another without padding; 0 for n_levels <= 1, n_levels above srz_texture_mip_levels, n_ch == 0 or
 * above SRZ_ATTR_MAX_CH, tex_frames == 0 or above 65536.  Both are pure host functions.
 * srz_texture_mip_build: d_tex -> d_mip (levels 1 .. n_levels - 1), each level from the level above it, deterministic, bit for bit,
 * whatever the wrap mode will be: where both extents halve out = ((t00 + t01) + (t10 + t11)) * 0.25f with t_rc at (2y + r, 2x + c);
 * where one extent is already 1, out = (t0 + t1) * 0.5f along the other.  A ctx-level call (no set); stream and asynchrony as the
 * frameset passes.  n_levels == 1 succeeds and launches nothing.
 * srz_texture_mip_fold: the backward of the build: the gradient pyramid d_gmip (d_mip's layout, read only) folded into d_gtex
 * (level 0, ADDED INTO by one fma per element).  A gather, no atomics, deterministic, bit for bit: per texel (y, x) of level 0 and
 * channel, with g_l the element of level l at (y >> l, x >> l), k_l the build's factor into level l (0.25f or 0.5f) and
 * L = n_levels:  acc = g_(L-1);  for l = L - 2 .. 1: acc = fmaf(k_(l+1), acc, g_l);  gtex = fmaf(k_1, acc, gtex).
 * SRZ_E_INVALID from either, nothing launched: a null ctx or pointer (the pyramid's may be null at n_levels == 1); tex_w or tex_h 0
 * or above SRZ_TEX_MAX_SIZE; n_ch 0 or above SRZ_ATTR_MAX_CH; tex_frames 0 or above 65536; n_levels 0 or above
 * srz_texture_mip_levels(tex_w, tex_h); mip_bytes below srz_texture_mip_bytes; a pointer not 4-byte aligned; the pyramid overlapping
 * the texture (n_levels > 1).
 * THE DERIVATIVES.  srz_frameset_interpolate_deriv: the signature, band sharding, owner and nobody and SRZ_FUSED_CLEAR of
 * srz_frameset_interpolate, except 1 <= n_ch <= SRZ_ATTR_MAX_CH / 2 and d_out [frame][2 * n_ch][local_rows][width],
 * srz_frameset_interpolate_bytes(2 * n_ch) bytes: plane 2 ch is d/dx, plane 2 ch + 1 d/dy of channel ch per one-pixel step.  The
 * positions are the set's own, read exactly as srz_frameset_position_grad reads them (a sceneset runs its vertex stage first); the
 * class bit plays no part.  Interpolation is affine in the sample point with owners held fixed, so the derivative is a constant of
 * the owner: with its nine floats ax ay z0 bx by z1 cx cy z2,
 *   area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);  r = 1.0f / area
 *   gax = (by - cy) * r;  gay = (cx - bx) * r;  gbx = (cy - ay) * r;  gby = (ax - cx) * r
 * and per channel, with the corner values a, b, c:  da = a - c;  db = b - c;
 *   d/dx = fmaf(da, gax, db * gbx);  d/dy = fmaf(da, gay, db * gby)
 * A zero area propagates inf / NaN as IEEE has it; no input value makes the pass read or write outside its buffers.  Deterministic,
 * bit for bit.  There is no backward: the derivative planes only select a level.
 * THE LOOKUP.  srz_frameset_texture_mip: srz_frameset_texture's arguments, plus d_uvd [frame][4][local_rows][width] — the planes
 * ux, uy, vx, vy (du/dx, du/dy, dv/dx, dv/dy) srz_frameset_interpolate_deriv writes at n_ch = 2, 16-byte aligned —, d_mip (the
 * pyramid srz_texture_mip_build wrote for THIS d_tex, 4-byte aligned) and n_levels.  n_levels == 1 reads neither d_uvd nor d_mip
 * (both may be null): the output is srz_frameset_texture's, bit for bit.  Unsampled pixels (u or v not finite), nobody's pixels and
 * SRZ_FUSED_CLEAR as the bilinear pass.  THE LEVEL of a sampled pixel, with L = n_levels and W, H the extents of level 0:
 *   fin = all four of ux, uy, vx, vy finite (fabsf(.) < INFINITY)
 *   ax = ux * (float)W;  ay = vx * (float)H;  bx = uy * (float)W;  by = vy * (float)H
 *   rx = fmaf(ax, ax, ay * ay);  ry = fmaf(bx, bx, by * by);  r2 = rx > ry ? rx : ry
 *   if (!fin || !(r2 < INFINITY))            l0 = L - 1, f = 0
 *   else { rho = sqrtf(r2)
 *     if (!(rho > 1.0f))                     l0 = 0, f = 0            (magnified, or no footprint)
 *     else { m = frexpf(rho, &e)             (rho = m * 2^e, 0.5 <= m < 1)
 *            l = e - 1;  f = fmaf(2.0f, m, -1.0f)                     (exact)
 *            if (l >= L - 1) l0 = L - 1, f = 0  else l0 = l } }
 * lambda = l0 + f is continuous and monotone in rho, equals log2(rho) at every power of two and lies within 0.0861 of it between
 * them: a PIECEWISE-LINEAR log2, a deliberate deviation from the true logarithm — it needs no transcendental function, so the rule
 * is exact on every implementation.  No level bias, no anisotropy.
 * THE SAMPLE: c_l is the bilinear sample of level l by the per-axis rule above with n = w_l, h_l (and this level's texels);
 *   out = c_l0 when f == 0 (level l0 + 1 is not read), else out = fmaf(f, c_(l0+1) - c_l0, c_l0).
 * BACKWARD, srz_frameset_texture_mip_grad: d_gout and the same d_vis, d_uv, d_uvd; at least one of (d_gtex with d_gmip) and d_guv.
 * d_gtex and d_gmip come together whenever n_levels > 1 (d_gmip is not touched, and may be null, at n_levels == 1).  LAMBDA IS HELD
 * FIXED, as owners are: there is no gradient to d_uvd.  d_tex and d_mip may be null when only the texel gradients are asked for.
 *   texels: for level l0 the level weight is lw = 1.0f - f, for level l0 + 1 it is lw = f, and that level gets no add when f == 0.
 *   Per corner and channel the float32 product (w_rc * lw) * gout[ch] (w_rc as the bilinear pass, from this level's tx, ty) is ADDED
 *   to the corner's texel of that level: level 0 in d_gtex, the others in d_gmip (d_mip's layout).  The caller zeroes the buffers,
 *   or accumulates; srz_texture_mip_fold then folds d_gmip into d_gtex.  THE ORDER OF THE ADDS IS UNSPECIFIED, each add rounds, so
 *   d_gtex and d_gmip are NOT BIT-REPRODUCIBLE between launches, like d_gtex of the bilinear pass: with n contributing adds an element
 *   lies within n 2^-24 / (1 - n 2^-24) * sum |term| of the exact sum of the float32 terms; an element with one contributing add is
 *   exact.  The adds are hardware float atomics: d_gtex and d_gmip must be ordinary (coarse-grained) device memory.
 *   d_guv, needs d_tex (and d_mip at n_levels > 1), deterministic, bit for bit: du_l, dv_l are the bilinear pass's du, dv at level l
 *   (its fma chains over the channels, the in_x / in_y gates and the factors (float)w_l, (float)h_l of that level);
 *   du = du_l0 when f == 0, else fmaf(f, du_(l0+1) - du_l0, du_l0); dv likewise.  The layout is srz_frameset_interpolate_grad's d_gout
 *   at n_ch = 2: the chain into interpolate_grad and position_grad continues unchanged.
 * Every level index follows the clamp to L - 1 and every texel index the clamp or the fraction of its own level: no value of uv or
 * uvd makes a pass read or write outside its buffers.
 * SRZ_E_INVALID, the outputs untouched and nothing launched: what the bilinear pair refuses, and n_levels 0 or above
 * srz_texture_mip_levels(tex_w, tex_h); with n_levels > 1 a null d_uvd, a null d_mip (forward; backward with d_guv), one of d_gtex /
 * d_gmip without the other; a misaligned pointer (16 bytes: the plane buffers, d_uvd among them; 4 bytes: d_tex, d_mip, d_gtex,
 * d_gmip); an output that overlaps an input (d_uvd and d_mip among the inputs, d_gmip among the outputs) or another output. */
#define SRZ_TEX_MAX_LEVELS 15u
uint32_t srz_texture_mip_levels(uint32_t tex_w, uint32_t tex_h);
size_t srz_texture_mip_bytes(uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels);
int srz_texture_mip_build(srz_ctx *ctx, const float *d_tex, uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames,
                          uint32_t n_levels, float *d_mip, size_t mip_bytes, void *stream);
int srz_texture_mip_fold(srz_ctx *ctx, const float *d_gmip, size_t mip_bytes, uint32_t tex_w, uint32_t tex_h, uint32_t n_ch,
                         uint32_t tex_frames, uint32_t n_levels, float *d_gtex, void *stream);
int srz_frameset_interpolate_deriv(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_attr, uint32_t n_ch,
                                   uint32_t attr_frames, uint32_t attr_tris, void *d_out, size_t out_bytes, uint32_t flags, void *stream);
int srz_frameset_texture_mip(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_uv, const void *d_uvd, const float *d_tex,
                             uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t mode, const float *d_mip,
                             uint32_t n_levels, void *d_out, size_t out_bytes, uint32_t flags, void *stream);
int srz_frameset_texture_mip_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_uv, const void *d_uvd, const void *d_gout,
                                  const float *d_tex, const float *d_mip, uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames,
                                  uint32_t mode, uint32_t n_levels, float *d_gtex, float *d_gmip, void *d_guv, uint32_t flags, void *stream);
/* MIPMAPPED CUBE-MAP LOOKUP by direction AND LEVEL over a visibility buffer, and its gradients: srz_frameset_texture_cube's lookup
 * over a mip pyramid of the cube, blended between two levels by a per-pixel level of detail lam that the CALLER supplies — a
 * roughness for a prefiltered specular probe, or the footprint level srz_frameset_cube_level derives for minified reflections — with
 * gradients to every level's texels, to the direction and to lam itself.  Four pieces: the pyramid (build, and fold: its backward),
 * the lookup, its backward, the level from the footprint.  All of it float32, nothing fused except where fmaf is written, division
 * and sqrtf the IEEE operations (SRZ_OPT_APPROX_SHADE has no effect).  Unless said otherwise, band sharding, local_rows, stream
 * semantics and asynchrony, the alignment (16 bytes: the plane buffers and the visibility buffer; 4 bytes: texels), owner, nobody and
 * SRZ_FUSED_CLEAR, overlap and refusal rules are srz_frameset_texture_cube's and srz_frameset_texture_mip's.
 * THE PYRAMID OF A CUBE.  Level 0 is the caller's cube [tex_frames][6][n][n][C].  Level l + 1 exists iff n_l > 1 and n_l is even; then
 * n_(l+1) = n_l / 2 (96: 6 levels, down to 3; 64: 7; 6: 2; 1 and 5: 1).  Each face is box-filtered ON ITS OWN — a 2 x 2 block never
 * crosses a face —, so every level is a cube that the 24-row seam table above resolves with N = n_l.  The layout is LEVEL-MAJOR:
 * level l is [tex_frames][6][n_l][n_l][C] float32, the levels 1 .. L - 1 one after another without padding.  That is exactly
 * srz_texture_mip_build / _fold on the cube viewed as 6 * tex_frames textures of n x n, and the four functions are that:
 *   srz_cube_mip_levels(n) = srz_texture_mip_levels(n, n)
 *   srz_cube_mip_bytes(n, n_ch, tex_frames, n_levels) = srz_texture_mip_bytes(n, n, n_ch, 6 * tex_frames, n_levels); 0 for
 *     tex_frames == 0 or 6 * tex_frames > 65536
 *   srz_cube_mip_build / srz_cube_mip_fold = srz_texture_mip_build / _fold with tex_w = tex_h = n and 6 * tex_frames frames, bit for
 *     bit, with their refusals; SRZ_E_INVALID also for tex_frames == 0 or 6 * tex_frames > 65536.
 * A caller may equally hand in a pyramid of their own in this layout (a GGX-prefiltered one, which srz_cube_prefilter writes level
 * by level): the lookup does not care who wrote it.
 * THE LOOKUP.  srz_frameset_texture_cube_mip: srz_frameset_texture_cube's arguments, plus d_mip (the levels 1 .. L - 1, 4-byte
 * aligned), n_levels = L, 1 <= L <= srz_cube_mip_levels(n), and d_lam [frame][1][local_rows][width] float32,
 * srz_frameset_interpolate_bytes(1) bytes, 16-byte aligned: the level of detail per pixel.  n_levels == 1 reads neither d_lam nor d_mip
 * (both may be null): the output is srz_frameset_texture_cube's, bit for bit.  A pixel is unsampled exactly as in the flat pass (a
 * direction component not finite, or the zero direction); the words of d_lam at unsampled and at nobody's pixels never reach a result.
 * THE LEVEL of a sampled pixel, with lam its word of d_lam:
 *   if (!(lam > 0.0f))                  l0 = 0, f = 0                 (NaN, negative, +-0)
 *   else if (lam >= (float)(L - 1))     l0 = L - 1, f = 0             (+inf too)
 *   else { lf = floorf(lam);  l0 = (int)lf;  f = lam - lf }           (exact)
 * Every level index follows these clamps: no value of lam makes a pass read or write outside its buffers.
 * THE SAMPLE: c_l is the flat pass's seamless bilinear sample of level l — the per-axis rule, the seam resolution and the three
 * fma's, with N = n_l and that level's texels.  The face and s, t do not depend on the level, only the per-axis step does.
 *   out = c_l0 when f == 0 (level l0 + 1 is not read), else out = fmaf(f, c_(l0+1) - c_l0, c_l0).
 * BACKWARD, srz_frameset_texture_cube_mip_grad: d_gout and the same d_vis, d_dir, d_lam; at least one of (d_gtex with d_gmip),
 * d_gdir and d_glam.  d_gtex and d_gmip come together whenever L > 1 (d_gmip is not touched, and may be null, at L == 1).  d_tex
 * and d_mip may be null when only the texel gradients are asked for.
 *   texels: for level l0 the level weight is lw = 1.0f - f, for level l0 + 1 it is lw = f, and that level gets no add when f == 0.
 *   Per corner and channel the float32 product (w_rc * lw) * gout[ch] (w_rc as the flat pass, from this level's tx, ty) is ADDED at
 *   the RESOLVED texel of that level: level 0 in d_gtex, the others in d_gmip (d_mip's layout).  The caller zeroes the buffers, or
 *   accumulates.  srz_cube_mip_fold then folds d_gmip into d_gtex for a box-built pyramid; a caller-made pyramid keeps d_gmip as its
 *   own gradient.  THE ORDER OF THE ADDS IS UNSPECIFIED, each add rounds, so d_gtex and d_gmip are NOT BIT-REPRODUCIBLE between
 *   launches: srz_frameset_texture_mip_grad's bound — with n contributing adds an element lies within n 2^-24 / (1 - n 2^-24) *
 *   sum |term| of the exact sum of the float32 terms; an element with one contributing add is exact.  Hardware float atomics: d_gtex
 *   and d_gmip must be ordinary (coarse-grained) device memory.
 *   d_gdir, needs d_tex (and d_mip at L > 1), deterministic, bit for bit: gdir_l is srz_frameset_texture_cube_grad's gdir computed at
 *   level l — au, av over that level's resolved texels, the factor 0.5f * (float)n_l, the chain through s, t and ma;
 *   gdir = gdir_l0 when f == 0, else per component fmaf(f, gdir_(l0+1) - gdir_l0, gdir_l0).  srz_frameset_texture_cube_grad's layout.
 *   d_glam [frame][1][local_rows][width], needs d_tex (and d_mip at L > 1), deterministic, bit for bit:
 *     where lam >= 0.0f && lam < (float)(L - 1):  acc = 0;  for ch in order: acc = fmaf(gout[ch], c_(l0+1)[ch] - c_l0[ch], acc);
 *       glam = acc — the RIGHT-HAND derivative: it reads level l0 + 1 even when f == 0, so a level initialised at an integer is not
 *       stuck at a zero gradient;
 *     elsewhere glam = 0: NaN, a negative lam (-0.0f counts as 0), lam at or beyond L - 1, L == 1, an unsampled pixel; nobody's
 *     pixels as the fused-clear rule has them.
 * THE LEVEL FROM THE FOOTPRINT.  srz_frameset_cube_level: d_dir, and d_dird [frame][6][local_rows][width] — the planes
 * srz_frameset_interpolate_deriv or _interpolate_deriv_persp writes for the direction's attribute at n_ch = 3 (plane 2 c is d/dx,
 * plane 2 c + 1 d/dy of component c), srz_frameset_interpolate_bytes(6) bytes — with n and n_levels = L -> a d_lam plane in d_out,
 * srz_frameset_interpolate_bytes(1) bytes.  Per sampled pixel take the flat pass's face, s, t and inv = 1.0f / ma.  For the x step,
 * dsc, dtc, dma are the components of (d dx/dx, d dy/dx, d dz/dx) that the face's su, sv and major axis name, with the sign flips of
 * sc, tc and ma (dma is negated where the major component is not positive); then
 *   sx = (dsc - s * dma) * inv;  tx = (dtc - t * dma) * inv;  ax = sx * (0.5f * (float)n);  ay = tx * (0.5f * (float)n)
 * and sy, ty, bx, by likewise from the y step (ax, bx from s; ay, by from t).  From there srz_frameset_texture_mip's rule word for
 * word, with fin = all four of sx, tx, sy, ty finite:  rx = fmaf(ax, ax, ay * ay);  ry = fmaf(bx, bx, by * by);  r2 = rx > ry ? rx : ry;
 * !fin or !(r2 < INFINITY) -> l0 = L - 1, f = 0;  rho = sqrtf(r2);  !(rho > 1.0f) -> l0 = 0, f = 0;  else m = frexpf(rho, &e),
 * l = e - 1, f = fmaf(2.0f, m, -1.0f), and l >= L - 1 -> l0 = L - 1, f = 0.  The output is lam = (float)l0 + f, a float32 sum that
 * may round: the lookup derives l0 and f from lam again.  An unsampled pixel writes 0; nobody's pixels follow the fused-clear rule.
 * There is no backward: the footprint level is held fixed, as in srz_frameset_texture_mip.  Deterministic, bit for bit.
 * SRZ_E_INVALID, the outputs untouched and nothing launched: what srz_frameset_texture_cube and _texture_cube_grad refuse, and
 * n_levels 0 or above srz_cube_mip_levels(n); with n_levels > 1 a null d_lam, a null d_mip (forward; backward with d_gdir or
 * d_glam), one of d_gtex / d_gmip without the other, 6 * tex_frames above 65536; d_gdir or d_glam without d_tex; none of the four
 * outputs; a misaligned pointer (16 bytes: the plane buffers, d_lam, d_glam and d_dird among them; 4 bytes: d_tex, d_mip, d_gtex,
 * d_gmip); a short out_bytes; any bit of `flags` but SRZ_FUSED_CLEAR; an output that overlaps an input (d_lam, d_mip and d_dird
 * among the inputs, d_gmip and d_glam among the outputs) or another output.  srz_frameset_cube_level: a null pointer, n 0 or above
 * SRZ_TEX_MAX_SIZE, n_levels 0 or above srz_cube_mip_levels(n), and the same alignment, size, flag and overlap rules. */
uint32_t srz_cube_mip_levels(uint32_t n);
size_t srz_cube_mip_bytes(uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels);
int srz_cube_mip_build(srz_ctx *ctx, const float *d_tex, uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels, float *d_mip,
                       size_t mip_bytes, void *stream);
int srz_cube_mip_fold(srz_ctx *ctx, const float *d_gmip, size_t mip_bytes, uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels,
                      float *d_gtex, void *stream);
int srz_frameset_texture_cube_mip(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_dir, const void *d_lam, const float *d_tex,
                                  uint32_t n, uint32_t n_ch, uint32_t tex_frames, const float *d_mip, uint32_t n_levels, void *d_out,
                                  size_t out_bytes, uint32_t flags, void *stream);
int srz_frameset_texture_cube_mip_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_dir, const void *d_lam,
                                       const void *d_gout, const float *d_tex, const float *d_mip, uint32_t n, uint32_t n_ch,
                                       uint32_t tex_frames, uint32_t n_levels, float *d_gtex, float *d_gmip, void *d_gdir, void *d_glam,
                                       uint32_t flags, void *stream);
int srz_frameset_cube_level(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_dir, const void *d_dird, uint32_t n,
                            uint32_t n_levels, void *d_out, size_t out_bytes, uint32_t flags, void *stream);
/* A CUBE PREFILTERED WITH A LOBE, and the exact transpose of that as its backward: what turns an environment cube into the levels
 * srz_frameset_texture_cube_mip blends by roughness (GGX) and into the irradiance cube srz_frameset_texture_cube looks up by the
 * normal (COSINE), with the gradient carried back to the environment's texels.  It is an all-pairs convolution, O(n_dst^2 n_src^2)
 * per channel.  No set and no visibility buffer are involved; stream semantics and asynchrony as srz_cube_mip_build.
 * d_src and d_gsrc: [tex_frames][6][n_src][n_src][n_ch] float32, srz_frameset_texture_cube's cube layout, faces and axes from its
 * table.  d_dst and d_gdst: the same layout with n_dst.  d_den: [6][n_dst][n_dst] float32, the normaliser: it depends on the
 * geometry, kind, roughness and cmin only, not on texel values or frames; the forward writes it when non-null, the backward needs it
 * as the forward wrote it (for the same n_src, n_dst, kind, roughness, cmin).  n_src and n_dst are independent, each 1 ..
 * SRZ_TEX_MAX_SIZE, any parity; 1 <= n_ch <= SRZ_ATTR_MAX_CH; 1 <= tex_frames <= 65536, every frame convolved alike.  d_work: scratch
 * of srz_cube_prefilter_work_bytes(n_src, n_dst, n_ch, tex_frames) bytes, 16-byte aligned, the same size for both calls (0 for
 * sizes out of range); its contents mean nothing between calls.  Every other pointer is 4-byte aligned.
 * THE RULE, all of it float32, nothing fused except where fmaf is written, / and sqrtf the correctly rounded operations, always the
 * exact arithmetic (SRZ_OPT_APPROX_SHADE has no effect).
 *   TEXEL GEOMETRY of texel (f, y, x) — face, row, column — of a cube of N x N faces:
 *     s = (float)(2 x + 1) / (float)N - 1.0f;  t = (float)(2 y + 1) / (float)N - 1.0f       (the texel centre of the cube section)
 *     p = n_f + s su_f + t sv_f, exact: in the order (x, y, z) the component along the face's normal is +-1, the component su names
 *       is s, negated where su is negative, the component sv names is t, negated where sv is negative — +X: (1, -t, -s);
 *       -X: (-1, -t, s);  +Y: (s, 1, t);  -Y: (s, -1, -t);  +Z: (s, -t, 1);  -Z: (-s, -t, -1)
 *     r2 = fmaf(s, s, fmaf(t, t, 1.0f));  inv = 1.0f / sqrtf(r2);  d = p * inv per component;  jac = (inv * inv) * inv
 *     (jac is the texel's solid angle up to the constant 4 / N^2, which cancels in the normalisation)
 *   PAIR WEIGHT of output texel o (geometry at N = n_dst) and source texel i (at N = n_src):
 *     c = fmaf(d_o.x, d_i.x, fmaf(d_o.y, d_i.y, d_o.z * d_i.z));  c = c > 1.0f ? 1.0f : c
 *     the pair is SKIPPED iff !(c > cmin): not added — never multiplied by zero — so an infinite or NaN texel behind the cutoff
 *     reaches no result.  cmin is finite and in [0, 1): the backward hemisphere is always skipped.
 *     SRZ_PREFILTER_COSINE:  w = c * jac_i
 *     SRZ_PREFILTER_GGX, with N = V = R, so that nh^2 = (1 + c) / 2 needs no square root:
 *       r = roughness < 0.0625f ? 0.0625f : roughness;  a = r * r;  a2 = a * a
 *       nh2 = fmaf(0.5f, c, 0.5f);  t = fmaf(nh2, a2 - 1.0f, 1.0f);  w = (c * jac_i) / (t * t)
 *     The weight is D (n.l) dw; pi and a2 cancel in the normalisation.  That is a CHOICE among the published prefilters (no
 *     importance sampling, no mip-biased source level, the lobe not renormalised by 1 / (4 v.h)).  At roughness 1 it is COSINE bit
 *     for bit (t = 1), and every roughness below 0.0625 is 0.0625.
 *   SUMS per output texel and channel, three levels in a fixed order, each from +0.0f:
 *     within a source row, columns ascending:  num = fmaf(w, src, num);  den = den + w
 *     the rows of a face, ascending, by plain adds;  the six faces in order, by plain adds
 *     dst = den > 0.0f ? num / den : 0.0f  (always written);  d_den gets den
 *   (a sequential sum is bounded at n_src terms, and the work may be split by row or by face without changing a bit.)
 *   BACKWARD, srz_cube_prefilter_grad:  q[o][ch] = den_o > 0.0f ? gdst[o][ch] / den_o : 0.0f, and gsrc[i][ch] is the same three-level
 *     sum over the OUTPUT texels — a row of the output cube, its faces, the cube — of acc = fmaf(w(o, i), q[o][ch], acc), with w by
 *     the identical text and the identical skip.  It is a gather: bit-reproducible, and d_gsrc is WRITTEN, not added into.  There
 *     is no gradient with respect to roughness or cmin.
 * An output texel that no pair reaches (a narrow cutoff over a coarse source) has den = 0, the value 0 and no share in the backward.
 * SUBNORMALS are numbers; non-finite texels and gradients propagate as IEEE has them through the pairs that are not skipped.  Both
 * passes use no atomics: two calls with the same arguments give the same words.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, d_src, d_dst, d_gdst, d_gsrc, d_work, or d_den in the
 * backward; n_src or n_dst 0 or above SRZ_TEX_MAX_SIZE; n_ch 0 or above SRZ_ATTR_MAX_CH; tex_frames 0 or above 65536; an unknown
 * kind; a roughness that is not finite or outside [0, 1]; a cmin that is not finite or outside [0, 1); work_bytes below
 * srz_cube_prefilter_work_bytes; d_work not 16-byte aligned, another pointer not 4-byte aligned; an output (d_dst, d_den, d_gsrc,
 * d_work) that overlaps an input or another output. */
#define SRZ_PREFILTER_COSINE 0u
#define SRZ_PREFILTER_GGX 1u
size_t srz_cube_prefilter_work_bytes(uint32_t n_src, uint32_t n_dst, uint32_t n_ch, uint32_t tex_frames);
int srz_cube_prefilter(srz_ctx *ctx, const float *d_src, uint32_t n_src, float *d_dst, uint32_t n_dst, uint32_t n_ch, uint32_t tex_frames,
                       uint32_t kind, float roughness, float cmin, float *d_den, void *d_work, size_t work_bytes, void *stream);
int srz_cube_prefilter_grad(srz_ctx *ctx, const float *d_gdst, const float *d_den, uint32_t n_src, uint32_t n_dst, uint32_t n_ch,
                            uint32_t tex_frames, uint32_t kind, float roughness, float cmin, float *d_gsrc, void *d_work, size_t work_bytes,
                            void *stream);
/* SH9 LIGHTING: the diffuse environment as NINE SPHERICAL-HARMONIC COEFFICIENTS PER CHANNEL (order 2), with gradients — the usual
 * unknown of inverse rendering in place of a cube of texels: 27 numbers for RGB, which carry the irradiance of any environment to
 * about 1 % (Ramamoorthi and Hanrahan).  Two pieces: srz_cube_sh projects a cube to its coefficients in one O(n^2) pass (no all-pairs
 * prefilter), srz_frameset_sh evaluates coefficients at each pixel's normal.  On srz_frameset_ibl's scale (E / pi), so the output is a
 * drop-in for srz_frameset_texture_cube of srz_cube_prefilter's COSINE cube at the normal.
 * THE CONSTANTS, binary32, each the binary32 nearest to the binary64 value (the products of the H's taken in binary64, rounded once):
 *   Yc0 = sqrt(1 / 4 pi) = 0x1.20dd76p-2f (0x3e906ebb);  Yc1 = sqrt(3 / 4 pi) = 0x1.f45438p-2f (0x3efa2a1c);
 *   Yc2 = sqrt(15 / 4 pi) = 0x1.17b142p+0f (0x3f8bd8a1);  Yc3 = sqrt(5 / 16 pi) = 0x1.42f602p-2f (0x3ea17b01);
 *   Yc4 = sqrt(15 / 16 pi) = 0x1.17b142p-1f (0x3f0bd8a1);  FOURPI = 12.566371f = 0x1.921fb6p+3f
 *   the band factors A_l / pi = 1, 2 / 3, 1 / 4 folded in:  H0 = Yc0 = 0x1.20dd76p-2f;  H1 = Yc1 * 2 / 3 = 0x1.4d8d7ap-2f;
 *   H2 = Yc2 / 4 = 0x1.17b142p-2f;  H3 = Yc3 / 4 = 0x1.42f602p-4f;  H4 = Yc4 / 4 = 0x1.17b142p-3f
 * THE POLYNOMIALS of a unit vector (x, y, z), in the standard real-SH order k = 0 .. 8:
 *   p = 1, y, z, x, x * y, y * z, fmaf(3.0f * z, z, -1.0f), x * z, fmaf(x, x, -(y * y));  constant index per k: 0, 1, 1, 1, 2, 2, 3, 2, 4
 *   (Yc[k], H[k] below: the constant of k's index.)
 * All of it float32, nothing fused except where fmaf is written, / and sqrtf the correctly rounded operations, always the exact
 * arithmetic (SRZ_OPT_APPROX_SHADE has no effect).  SUBNORMALS are numbers; non-finite values propagate as IEEE has them.
 *
 * srz_cube_sh / srz_cube_sh_grad / srz_cube_sh_work_bytes: A CUBE TO ITS SH9 COEFFICIENTS.  No set and no visibility buffer are
 * involved; stream semantics and asynchrony as srz_cube_mip_build.  d_src and d_gsrc: [tex_frames][6][n][n][n_ch] float32,
 * srz_frameset_texture_cube's layout; d_sh and d_gsh: [tex_frames][9][n_ch] float32; d_den: one float32, the normaliser: it depends
 * on n only; the forward writes it when non-null, the backward needs it as the forward wrote it (for the same n).  n is 1 ..
 * SRZ_TEX_MAX_SIZE, any parity; 1 <= n_ch <= SRZ_SH_MAX_CH; 1 <= tex_frames <= 65536.  d_work: scratch of
 * srz_cube_sh_work_bytes(n, n_ch, tex_frames) bytes (0 for sizes out of range), the same size for both calls; its contents mean
 * nothing between calls.  Every pointer is 4-byte aligned.
 * THE RULE: the texel geometry d, jac of texel (f, y, x) is srz_cube_prefilter's TEXEL GEOMETRY at N = n, word for word.
 *   b_k = Yc[k] * p_k(d);  w_k = jac * b_k                                                    (k = 0 .. 8; b_0 = Yc0 * 1.0f)
 *   per frame, k and channel, the numerator is summed in a FIXED TREE: within a face row, lane j of 64 takes the columns j, j + 64,
 *   ... ascending, with a = fmaf(w_k, src, a) from +0; the 64 lane sums go through the butterfly v = v + v[lane ^ o], o = 32, 16, 8,
 *   4, 2, 1 (a lane without a column holds +0); the rows of a face are added ascending by plain adds from +0; the six faces in order
 *   by plain adds from +0.  den is the same tree over a = a + jac.
 *   sh[k][c] = (FOURPI * num) / den        (always written)
 * BACKWARD, srz_cube_sh_grad, a gather per source texel, no atomics, d_gsrc WRITTEN, not added into:
 *   q[k][c] = (FOURPI * gsh[k][c]) / den;   gsrc[c] = w_0 * q[0][c], then gsrc[c] = fmaf(w_k, q[k][c], gsrc[c]) for k = 1 .. 8,
 *   w_k by the identical text.  Both directions are bit-reproducible: two calls with the same arguments give the same words.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, d_src, d_sh, d_gsh, d_gsrc, d_work, or d_den in the
 * backward; n 0 or above SRZ_TEX_MAX_SIZE; n_ch 0 or above SRZ_SH_MAX_CH; tex_frames 0 or above 65536; work_bytes below
 * srz_cube_sh_work_bytes; a pointer not 4-byte aligned; an output (d_sh, d_den, d_gsrc, d_work) that overlaps an input or another
 * output.
 *
 * srz_frameset_sh / srz_frameset_sh_grad / srz_frameset_sh_work_bytes: SH9 EVALUATED AT EACH PIXEL'S NORMAL over a visibility
 * buffer.  d_vis, d_nrm (3 planes), d_out / d_gout (n_ch planes, srz_frameset_interpolate_bytes(n_ch) bytes) and d_gnrm: exactly as in
 * srz_frameset_light — band sharding, local_rows, stream semantics, asynchrony, the 16-byte alignment, owner and nobody, what a nobody
 * pixel's words of the output planes become with and without SRZ_FUSED_CLEAR (zeros; untouched).  d_sh and d_gsh:
 * [sh_frames][9][n_ch] float32 in device memory, 4-byte aligned; sh_frames is 1 (every frame shares the coefficients) or the set's
 * frame count; 1 <= n_ch <= SRZ_SH_MAX_CH.  kind, a host argument: SRZ_SH_IRRADIANCE (K = H: the cosine-convolved function, E / pi)
 * or SRZ_SH_RADIANCE (K = Yc: the function itself, for a low-frequency background or a test); no gradient to it.
 * THE RULE, dot as srz_frameset_light's.  Per owned pixel with the normal n:
 *   nn = dot(n, n);  lit = nn > 0 && nn < INFINITY;   not lit -> out = 0 in every channel (written), every gradient of the pixel 0, no term
 *   inl = 1 / sqrtf(nn);  N = n * inl;  e_0 = K[0];  e_k = K[k] * p_k(N)  (k = 1 .. 8)
 *   out_c = sh[0][c] * e_0, then out_c = fmaf(sh[k][c], e_k, out_c) for k = 1 .. 8.        There is NO CLAMP (SH ringing can go
 *   slightly negative; a clamp would cut the gradient).
 * BACKWARD: the exact derivative with the lit branch held, in THIS order of operations (g = gout of the pixel, N = (x, y, z)):
 *   ge_k = g_0 * sh[k][0], then ge_k = fmaf(g_c, sh[k][c], ge_k) for c = 1 .. n_ch - 1;   gp_k = ge_k * K[k]       (k = 1 .. 8)
 *   gN_x = fmaf(2.0f * x, gp_8, fmaf(gp_7, z, fmaf(gp_4, y, gp_3)))
 *   gN_y = fmaf(-2.0f * y, gp_8, fmaf(gp_5, z, fmaf(gp_4, x, gp_1)))
 *   gN_z = fmaf(6.0f * z, gp_6, fmaf(gp_7, x, fmaf(gp_5, y, gp_2)))
 *   d = dot(gN, N);  gn_i = (gN_i - N_i * d) * inl
 *   d_gnrm = gn: per pixel, deterministic, bit for bit.  d_gsh (needs d_work, at least srz_frameset_sh_work_bytes bytes, 4-byte
 *   aligned, scratch) is WRITTEN, not added into: entry (k, c) is the sum over the frame's lit pixels on this shard of the float32
 *   term g_c * e_k in srz_frameset_light_grad's FIXED tree, word for word (lane quads left to right, the butterfly, the four waves
 *   through LDS, the tiles in tile order, then with sh_frames == 1 the frames in frame order): no atomics, BIT-REPRODUCIBLE for a
 *   given shard layout, with one lit pixel in all that pixel's term (-0 comes out +0), +0 where nobody contributes, and within
 *   n 2^-24 / (1 - n 2^-24) * sum |term| of the exact sum.  Ranks each write the sums of their own bands.  Each of d_gnrm and d_gsh
 *   may be NULL, not both.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, d_vis, d_nrm, d_sh, d_out, d_gout, or both of
 * d_gnrm, d_gsh; n_ch == 0 or above SRZ_SH_MAX_CH; sh_frames not 1 or the frame count; an unknown kind; a short out_bytes, or
 * work_bytes with d_gsh; a misaligned pointer; any bit of `flags` but SRZ_FUSED_CLEAR; an output (d_work with d_gsh counts as one)
 * that overlaps an input or another output; d_gsh without d_work. */
#define SRZ_SH_MAX_CH 7 /* 9 * n_ch <= 63: a row of the fixed tree's 64 */
#define SRZ_SH_IRRADIANCE 0u
#define SRZ_SH_RADIANCE 1u
size_t srz_cube_sh_work_bytes(uint32_t n, uint32_t n_ch, uint32_t tex_frames);
int srz_cube_sh(srz_ctx *ctx, const float *d_src, uint32_t n, uint32_t n_ch, uint32_t tex_frames, float *d_sh, float *d_den, void *d_work,
                size_t work_bytes, void *stream);
int srz_cube_sh_grad(srz_ctx *ctx, const float *d_gsh, const float *d_den, uint32_t n, uint32_t n_ch, uint32_t tex_frames, float *d_gsrc,
                     void *d_work, size_t work_bytes, void *stream);
int srz_frameset_sh(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const float *d_sh, uint32_t n_ch, uint32_t sh_frames,
                    uint32_t kind, void *d_out, size_t out_bytes, uint32_t flags, void *stream);
size_t srz_frameset_sh_work_bytes(srz_ctx *ctx, srz_frameset *fs, uint32_t n_ch);
int srz_frameset_sh_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const float *d_sh, uint32_t n_ch,
                         uint32_t sh_frames, uint32_t kind, const void *d_gout, void *d_gnrm, float *d_gsh, void *d_work, size_t work_bytes,
                         uint32_t flags, void *stream);
/* IMAGE-BASED LIGHTING over a visibility buffer, for the caller's own planes, with gradients: the three pieces between
 * srz_cube_prefilter's cubes, the cube lookups and srz_frameset_microfacet's material — the reflection vector, the split-sum table of
 * srz_frameset_microfacet's OWN specular lobe, and the combine.  The chain: srz_brdf_table once; srz_frameset_reflect -> R and n.v;
 * srz_frameset_texture_cube_mip at R and roughness * (levels - 1) over the GGX levels -> spec; srz_frameset_texture_cube of the
 * cosine cube at the normal -> irr; srz_frameset_ibl -> the colour, to which srz_frameset_microfacet's point lights add.  Band
 * sharding, local_rows, stream semantics, asynchrony, the 16-byte alignment of the visibility buffer and every plane buffer, owner and
 * nobody, what a nobody pixel's words of the output planes become with and without SRZ_FUSED_CLEAR (zeros; untouched), and what the
 * passes do not read or launch: all as srz_frameset_microfacet.  The words of the input planes at nobody's pixels never reach a
 * result.  All of it float32, nothing fused except where fmaf is written, / and sqrtf the correctly rounded ones, always the exact
 * arithmetic; NO TRANSCENDENTAL FUNCTION: /, sqrtf, fmaf, floorf, products and a fifth power by multiplication.  dot, l_pos,
 * 1 / sqrtf(x), INV_PI and RMIN as in srz_frameset_microfacet.
 *
 * srz_frameset_reflect: d_nrm, d_pos, d_gnrm, d_gpos [frame][3][local_rows][width]; d_eye [par_frames][3] float32 in device memory,
 * 4-byte aligned, par_frames 1 or the set's frame count; d_out and d_gout [frame][4][local_rows][width],
 * srz_frameset_interpolate_bytes(4) bytes.  Per owned pixel:
 *   nn, lit, inl, N, V, vv, view, iv, Vd: exactly as srz_frameset_light (the eye is d_eye's)
 *   not lit, or no view -> out = (0, 0, 0, 0) (written), no gradient: a zero direction is srz_frameset_texture_cube's "unsampled"
 *   nv = dot(N, Vd);  t2 = 2 * nv;  R_c = fmaf(t2, N_c, -Vd_c);  out = (R_0, R_1, R_2, nv)
 * Plane 3 is the RAW nv, not clamped: the consumer clamps it.
 * BACKWARD (g = gout of the pixel, gR its first three words), through both normalisations:
 *   g_nv = fmaf(2, dot(gR, N), g_3);  gN_c = fmaf(g_nv, Vd_c, gR_c * t2);  gVd_c = fmaf(g_nv, N_c, -gR_c)
 *   dv = dot(gVd, Vd);  gpos_c = -((gVd_c - Vd_c * dv) * iv);  dn = dot(gN, N);  gnrm_c = (gN_c - N_c * dn) * inl
 * per pixel, no atomics, bit for bit.  d_gnrm or d_gpos may be NULL, not both.  THERE IS NO EYE GRADIENT in this ABI: R and nv depend
 * on eye - P only, so the gradient of a frame's eye is minus the sum of that frame's d_gpos over its owned pixels (over every frame
 * when the eye is shared); the caller takes that sum.
 *
 * srz_brdf_table: no set and no visibility buffer; d_tab [n][n][2] float32 (A, B), 4-byte aligned, WRITTEN; 2 <= n <=
 * SRZ_BRDF_TABLE_MAX; 1 <= m <= 256.  Entry (i, j): nv = (float)i / (float)(n - 1);  rc = fmaf(0.9375f, (float)j / (float)(n - 1),
 * RMIN): the nodes lie on the clamp edges, so the lookup never extrapolates.  F0 * A + B is the directional albedo of exactly the
 * lobe srz_frameset_microfacet shades with (its D, its Vs with k = al / 2, Schlick's F), by a deterministic, rational quadrature
 * over the projected half vector with the GGX density taken out analytically:
 *   al = rc * rc;  a2 = al * al;  k = 0.5f * al;  omk = 1 - k;  vx = sqrtf(fmaf(-nv, nv, 1));  gv = fmaf(nv, omk, k);  fm = (float)m
 *   A = B = +0;  for ring a = 0 .. m - 1 in order:
 *     u = ((float)a + 0.5f) / fm;  q = 1 - u;  xi = fmaf(-q, q, 1);  wr = (2 * q) / fm
 *     s = (a2 * xi) / fmaf(-xi, 1 - a2, 1);  r = sqrtf(s);  hz = sqrtf(1 - s)                   (the inverse of the GGX CDF in r^2)
 *     ra = rb = +0;  for b = 0 .. m - 1 in order:
 *       t = ((float)b + 0.5f) / fm;  tt = t * t;  den = 1 + tt;  c = (1 - tt) / den;  wa = (2 / den) / fm        (the rational circle)
 *       for hx = r * c, then hx = -(r * c)  (the half y < 0 is the mirror image: INV_PI carries its factor):
 *         vh = fmaf(vx, hx, nv * hz);  nl = fmaf(2 * vh, hz, -nv);  take = vh > 0 && nl > 0  (a select: a sample not taken adds +0)
 *         gl = fmaf(nl, omk, k);  f = (nl * vh) / (hz * (gl * gv))
 *         x = 1 - (vh < 1 ? vh : 1);  x2 = x * x;  x4 = x2 * x2;  x5 = x4 * x
 *         ra = ra + (take ? (f * (1 - x5)) * wa : 0);  rb = rb + (take ? (f * x5) * wa : 0)
 *     A = fmaf(ra, wr, A);  B = fmaf(rb, wr, B)
 *   tab = (A * INV_PI, B * INV_PI)
 * The sums run in THIS order whatever the launch shape: two calls, and any implementation of this text, give the same words.  The
 * error is the quadrature's; the substitution xi = 1 - q^2 is part of the rule (it tames the 1 / hz tail).  No gradient: the table
 * has no differentiable input.
 *
 * srz_frameset_ibl: d_base (may be NULL: ones; d_gbase must then be NULL), d_irr, d_spec, d_out, d_gout, d_gbase, d_girr, d_gspec
 * [frame][3][local_rows][width]; d_mat, d_gmat [frame][2][..] (roughness, metallic); d_nv, d_gnv [frame][1][..] (srz_frameset_reflect's
 * plane 3, or any cosine); d_tab and d_gtab [n][n][2] float32, 4-byte aligned, one table for every frame, 2 <= n <=
 * SRZ_BRDF_TABLE_MAX.  Per owned pixel:
 *   rc, r_in, mc, m_in: exactly as srz_frameset_microfacet clamps them
 *   nvc = nv > 0 ? (nv < 1 ? nv : 1) : 0;  nv_in = nv > 0 && nv < 1                                       (a NaN: 0, no gradient)
 *   sx = (float)(n - 1);  sy = (float)(n - 1) / 0.9375f;  x = nvc * sx;  y = (rc - RMIN) * sy
 *   x0 = min((int)floorf(x), n - 2);  tx = x - (float)x0;  y0 = min((int)floorf(y), n - 2);  ty = y - (float)y0
 *   for e = A, B, with t00 = tab[x0][y0][e], t01 = tab[x0][y0 + 1][e], t10 = tab[x0 + 1][y0][e], t11 = tab[x0 + 1][y0 + 1][e]:
 *     d0 = t01 - t00;  d1 = t11 - t10;  top = fmaf(ty, d0, t00);  bot = fmaf(ty, d1, t10);  dx_e = bot - top;  e = fmaf(tx, dx_e, top)
 *     dy_e = fmaf(tx, d1 - d0, d0)                                                      (the cell's bilinear slopes, for the backward)
 *   om = 1 - mc;  F0_c = fmaf(mc, base_c - 0.04f, 0.04f);  cdif_c = base_c * om;  sc_c = fmaf(F0_c, A, B)
 *   out_c = fmaf(cdif_c, irr_c, spec_c * sc_c)
 * There is no pi (srz_cube_prefilter's cosine cube is already the normalised average) and no clamp of the result.  The clamps leave x
 * and y finite and inside [0, n - 1] up to a rounding, and the min holds the cell: NO PLANE VALUE MAKES A PASS READ OUTSIDE THE TABLE.
 * A coordinate exactly on a node below the last returns the node's word (tx = 0); on the last node tx = 1 and the word is
 * fmaf(1, t01 - t00, t00), the node's word wherever that difference is exact.
 * BACKWARD (g = gout of the pixel), in THIS order of operations:
 *   gcd_c = g_c * irr_c;  girr_c = g_c * cdif_c;  gs_c = g_c * spec_c;  gspec_c = g_c * sc_c;  gF0_c = gs_c * A
 *   gbase_c = fmaf(gF0_c, mc, gcd_c * om);  gA = dot(gs, F0);  gB = dot(g, spec)
 *   g_mc = dot(gF0, base - 0.04f);  g_om = dot(gcd, base);  g_x = fmaf(gA, dx_A, gB * dx_B);  g_y = fmaf(gA, dy_A, gB * dy_B)
 *   gmat0 = r_in ? g_y * sy : 0;  gmat1 = m_in ? g_mc - g_om : 0;  gnv = nv_in ? g_x * sx : 0
 * per pixel, no atomics, bit for bit.  d_gtab is ADDED INTO, like srz_frameset_texture_grad's d_gtex: with ux = 1 - tx, uy = 1 - ty
 * and the weights w = (ux * uy, ux * ty, tx * uy, tx * ty) of (x0, y0), (x0, y0 + 1), (x0 + 1, y0), (x0 + 1, y0 + 1), each owned
 * pixel adds the float32 terms w_q * gA to A and w_q * gB to B of its four entries.  Float adds in no fixed order: NOT
 * bit-reproducible; against the exact sum of the terms a word lies within n 2^-24 / (1 - n 2^-24) * sum |term|, n its contributing
 * pixels (+ 1 for the add into the caller's word); with one contributing pixel and a zeroed table it is that pixel's term.  Any of
 * d_gbase, d_gmat, d_gnv, d_girr, d_gspec, d_gtab may be NULL, not all six.
 * SUBNORMALS are numbers; non-finite values propagate as IEEE has them.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set (the table: not needed), d_vis, a null required
 * input (d_nrm, d_pos, d_eye; d_mat, d_nv, d_irr, d_spec, d_tab), d_out, d_gout, or every output of a backward; par_frames not 1 or
 * the frame count; n outside [2, SRZ_BRDF_TABLE_MAX]; m outside [1, 256]; a short out_bytes or tab_bytes; a misaligned pointer; any
 * bit of `flags` but SRZ_FUSED_CLEAR; an output that overlaps an input or another output; d_gbase without d_base. */
#define SRZ_BRDF_TABLE_MAX 64u
int srz_frameset_reflect(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const float *d_eye,
                         uint32_t par_frames, void *d_out, size_t out_bytes, uint32_t flags, void *stream);
int srz_frameset_reflect_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const float *d_eye,
                              uint32_t par_frames, const void *d_gout, void *d_gnrm, void *d_gpos, uint32_t flags, void *stream);
int srz_brdf_table(srz_ctx *ctx, float *d_tab, size_t tab_bytes, uint32_t n, uint32_t m, void *stream);
int srz_frameset_ibl(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_base, const void *d_mat, const void *d_nv,
                     const void *d_irr, const void *d_spec, const float *d_tab, uint32_t n, void *d_out, size_t out_bytes, uint32_t flags,
                     void *stream);
int srz_frameset_ibl_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_base, const void *d_mat, const void *d_nv,
                          const void *d_irr, const void *d_spec, const float *d_tab, uint32_t n, const void *d_gout, void *d_gbase,
                          void *d_gmat, void *d_gnv, void *d_girr, void *d_gspec, float *d_gtab, uint32_t flags, void *stream);
/* THE ENVIRONMENT BEHIND A VISIBILITY BUFFER, BY VIEW RAY, and its gradients: the COMPLEMENT of every pass above.  They write the
 * pixels somebody owns; this one writes the pixels nobody owns (or, on request, all of them): it forms the pixel's view ray from a small
 * device block, looks that ray up in a caller cube by srz_frameset_texture_cube's rule, seams included, and its backward goes to the
 * cube's texels and to the ray block — so an environment can be fitted to the pixels around an object, srz_frameset_antialias has a
 * background to blend an outline with, and the camera's rotation and intrinsics are learnable from the backdrop.
 * d_tex, d_gtex, n, n_ch, tex_frames, d_out, d_gout: exactly srz_frameset_texture_cube's — shapes, limits, alignment, band sharding,
 * stream semantics, asynchrony.  d_ray and d_gray: [ray_frames][9] float32 in device memory, 4-byte aligned; ray_frames is 1 (every
 * frame shares the one block) or the set's frame count; a row is r0[3] rx[3] ry[3].  d_vis: a visibility buffer of THIS set on this
 * ctx's shard.
 * `where`: SRZ_BG_NOBODY — the pass's pixels are those nobody owns: id 0, the bare class bit, or an index outside the frame's
 * triangles —, or SRZ_BG_ALL — every pixel of the frame is the pass's; d_vis may be NULL and is not read: an environment preview, and
 * the layer behind the last peel of a composite.
 * OWNED PIXELS (SRZ_BG_NOBODY) are what nobody's pixels are to the other passes: their words of d_out are 0 with SRZ_FUSED_CLEAR
 * (frame flags | `flags`), otherwise LEFT UNTOUCHED — a caller can pass its shaded buffer and have the holes filled in place.  The
 * words of d_gout there are never read.
 * THE RULE, all of it float32, nothing fused except where fmaf is written, the divisions the IEEE division, always the exact
 * arithmetic (SRZ_OPT_APPROX_SHADE has no effect).  A pixel's sample point is its INTEGER CORNER (x, y), as in srz_frameset_antialias
 * and srz_frameset_motion; y is the frame's row, not the shard-local one:
 *   d_c = fmaf((float)y, ry_c, fmaf((float)x, rx_c, r0_c))                for c = x, y, z
 * and from d on the forward is srz_frameset_texture_cube's rule, word for word: unsampled (a component not finite, or the zero
 * vector), the major axis, s and t, the seams, the three fmafs.  An unsampled pixel of the pass writes zeros and contributes nothing.
 * BACKWARD: at least one of d_gtex and d_gray is non-null.
 *   d_gtex (d_tex may be null when only d_gtex is asked for): srz_frameset_texture_cube_grad's adds at the resolved texels, the same
 *   contract — float atomics, combined per tile and distinct texel first, the order unspecified, NOT BIT-REPRODUCIBLE, within
 *   n 2^-24 / (1 - n 2^-24) * sum |term| with n contributing adds, exact at n = 1; ordinary (coarse-grained) device memory.
 *   d_gray (needs d_tex, and d_work of at least srz_frameset_background_work_bytes bytes, 4-byte aligned, scratch: what it holds
 *   afterwards is unspecified) is WRITTEN, not added into.  Per sampled pixel gdir is formed exactly as srz_frameset_texture_cube_grad
 *   forms it; the nine terms of the pixel are gdir_c (r0), (float)x * gdir_c (rx), (float)y * gdir_c (ry); entry k of a frame's row
 *   is the sum of the pixels' terms in srz_frameset_light_grad's FIXED tree, word for word: a lane's up to four pixels left to right,
 *   from +0; the xor butterfly over the 64 lanes, o = 32, 16, 8, 4, 2, 1; the four waves as ((w0 + w1) + w2) + w3; a frame's tiles in
 *   tile order, from +0; and with ray_frames == 1 the frames' rows in frame order, from +0.  So d_gray is BIT-REPRODUCIBLE for a given
 *   shard layout, with one sampled pixel in all it is that pixel's term (a term of -0 comes out +0), and against the exact sum it
 *   carries that section's bound.  Ranks each write the sums of their own bands.
 * SUBNORMALS, non-finite texels and gradients: as srz_frameset_texture_cube.  No value of the block or of a texel makes a pass read
 * or write outside its buffers.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, d_ray, d_tex (forward; backward with d_gray),
 * d_out, d_gout, d_vis with SRZ_BG_NOBODY, or both of d_gtex and d_gray; n == 0 or above SRZ_TEX_MAX_SIZE; n_ch == 0 or above
 * SRZ_ATTR_MAX_CH; ray_frames or tex_frames not 1 or the frame count; `where` above 1; a short out_bytes, or work_bytes with d_gray;
 * a misaligned pointer; any bit of `flags` but SRZ_FUSED_CLEAR; an output (d_work with d_gray counts as one) that overlaps an input
 * or another output; d_gray without d_work or d_tex. */
#define SRZ_BG_NOBODY 0u
#define SRZ_BG_ALL 1u
int srz_frameset_background(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_ray, uint32_t ray_frames, const float *d_tex,
                            uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t where, void *d_out, size_t out_bytes, uint32_t flags,
                            void *stream);
size_t srz_frameset_background_work_bytes(srz_ctx *ctx, srz_frameset *fs);
int srz_frameset_background_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_ray, uint32_t ray_frames,
                                 const void *d_gout, const float *d_tex, uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t where,
                                 float *d_gtex, float *d_gray, void *d_work, size_t work_bytes, uint32_t flags, void *stream);
/* COMPOSITING DEPTH LAYERS FRONT TO BACK, and its gradients: the step that turns the shaded layers of a depth peel
 * (srz_frameset_peel_visibility) into one image, in one pass over the tiles.  A call takes n_layers layers, 1 .. SRZ_COMPOSITE_MAX,
 * NEAREST FIRST, in a HOST array of srz_composite_layer (read before the call returns).  A layer is: `vis`, a visibility buffer of
 * THIS set on this ctx's shard, of which only the id plane is read; `color`, n_ch planes (1 .. SRZ_ATTR_MAX_CH) in
 * srz_frameset_interpolate's output layout [frame][n_ch][local_rows][width]; and `alpha`, one plane [frame][1][local_rows][width],
 * or, if `alpha` is NULL, the scalar `opacity` for every pixel of the layer.  d_bg (may be NULL): n_ch planes behind everything,
 * srz_frameset_background's output for one.  want_through (0 or 1): the transmittance T is appended to the output as plane n_ch, so
 * d_out and d_gout are [frame][n_ch + want_through][local_rows][width] and out_bytes covers srz_frameset_interpolate_bytes of that
 * many planes.  Stream semantics, asynchrony, local_rows and band sharding: exactly srz_frameset_normal_map's.
 * COVERAGE.  Layer k covers a pixel when its id word names an owner: id 0, the bare class bit and an index outside the frame's
 * triangles are nobody, as in every pass above.  A layer that does not cover the pixel is SKIPPED: its colour and alpha words at that
 * pixel never reach a result (they may be NaN).  THE LAYERS NEED NOT COME FROM ONE PEEL CHAIN: a nobody layer does not end the
 * pixel, and the same buffer may be passed as two layers.
 * THE RULE, all of it float32, nothing fused except where fmaf is written.  FORWARD, per pixel: T = 1, acc_c = +0; for each covering
 * layer in order, with a its alpha (the plane's word, or opacity) and col_c its colour:
 *   w = a * T;   acc_c = acc_c + col_c * w   for every channel c;   T = T * (1 - a)
 * then, with d_bg, acc_c = acc_c + bg_c * T.  The output is acc_c, and T in plane n_ch if asked for.  THERE IS NO CLAMP OF a AND NO
 * EARLY EXIT at T == 0: a covered layer behind an opaque one is still read, because the opaque layer's alpha gradient needs it.
 * EVERY WORD OF d_out IN THE SHARD'S OWNED ROWS IS WRITTEN, whatever `flags` (as srz_frameset_peel_visibility): a pixel no layer
 * covers is bg_c (or +0) with T = 1.  Padding rows of a shard keep what they held.
 * BACKWARD.  g_c are d_gout's first n_ch planes, gT its plane n_ch, or 0 when want_through is 0.  T_k (the T layer k met) and
 * w_k = a_k * T_k are recomputed as in the forward pass, T_n is the final T.  No division appears, so a = 1 is an ordinary value.
 *   gbg_c = g_c * T_n
 *   S = gT;   with d_bg: S = fmaf(g_c, bg_c, S) for c = 0, 1, .. in channel order
 *   for the covering layers FROM LAST TO FIRST:
 *     d = +0;   d = fmaf(g_c, col_c, d) for c = 0, 1, .. in channel order
 *     gcol_c = g_c * w_k
 *     galpha = T_k * (d - S)
 *     S = fmaf(a, d, (1 - a) * S)
 * d_gcolor and d_galpha are HOST arrays of n_layers device pointers (color's and alpha's shapes), or NULL: none of them; each entry
 * may be NULL; d_gbg has d_bg's shape.  At least one output is asked for.  d_galpha[k] may be asked for even when layer k's alpha is
 * the scalar: the scalar's gradient is the sum of that plane.  Every word of an asked-for plane in the owned rows is WRITTEN, +0 where
 * the layer does not cover the pixel; per pixel, no atomics: BIT-REPRODUCIBLE.  Without any d_galpha the colour planes are not read.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, layers, a layer's vis or color, d_out, d_gout;
 * n_layers 0 or above SRZ_COMPOSITE_MAX; n_ch 0 or above SRZ_ATTR_MAX_CH; want_through above 1; a short out_bytes; a pointer that is
 * not 16-byte aligned; any bit of `flags` but SRZ_FUSED_CLEAR (which changes nothing here); an output that overlaps an input or
 * another output (inputs may alias each other); a gradient call with nothing asked for; d_gbg without d_bg. */
#define SRZ_COMPOSITE_MAX 8
typedef struct srz_composite_layer {
  const void *vis;   /* device: the layer's visibility buffer */
  const void *color; /* device: [frame][n_ch][local_rows][width] */
  const void *alpha; /* device: [frame][1][local_rows][width], or NULL: `opacity` */
  float opacity;
  uint32_t _pad;
} srz_composite_layer;
int srz_frameset_composite(srz_ctx *ctx, srz_frameset *fs, const srz_composite_layer *layers, uint32_t n_layers, uint32_t n_ch,
                           const void *d_bg, uint32_t want_through, void *d_out, size_t out_bytes, uint32_t flags, void *stream);
int srz_frameset_composite_grad(srz_ctx *ctx, srz_frameset *fs, const srz_composite_layer *layers, uint32_t n_layers, uint32_t n_ch,
                                const void *d_bg, uint32_t want_through, const void *d_gout, void *const *d_gcolor,
                                void *const *d_galpha, void *d_gbg, uint32_t flags, void *stream);
/* TEXTURE SETS: srz_frameset_texture with the texture of each pixel chosen by its owner's batch, and the gradients of that — the
 * first texture lookup of a scene with more than one material in one pass over the tiles.  A call takes n_slots textures,
 * 1 .. SRZ_TEXSET_MAX, in a HOST array of srz_texset_slot (read before the call returns, like srz_composite_layer's array), and
 * d_batch_slot, DEVICE memory of n_batch_slot bytes (1 .. 65536): ONE map for every frame of the set, indexed by the owner's batch
 * within its frame — for a sceneset its draw, the value SRZ_GB_BATCH writes minus 1.  A slot is d_tex [tex_frames][tex_h][tex_w][n_ch]
 * as srz_frameset_texture takes it, its own tex_w, tex_h, tex_frames (1 or the set's frame count) and mode (SRZ_TEX_CLAMP /
 * SRZ_TEX_WRAP), and, in the backward only, d_gtex of d_tex's shape (ADDED INTO) or NULL: this slot's texel gradient is not wanted.
 * n_ch is one value for the call: every slot's texture has n_ch channels.  d_vis, d_uv, d_out, d_gout, d_guv: srz_frameset_texture's.
 * THE RULE.  Owner and nobody: exactly as srz_frameset_texture.  THE SLOT of an owned pixel: with b the owner's batch,
 *   s = b < n_batch_slot ? d_batch_slot[b] : SRZ_TEXSET_NONE
 * If s >= n_slots (so in particular SRZ_TEXSET_NONE) the pixel is UNSAMPLED in srz_frameset_texture's sense: every channel of out
 * is 0 (written: the pixel has an owner), guv = (0, 0), no add.  No byte of the map makes a pass read or write outside its
 * buffers; the host cannot validate device bytes and does not try.  Otherwise the pixel follows srz_frameset_texture's rule, word
 * for word, with slot s's d_tex, tex_w, tex_h, tex_frames and mode: the forward, d_guv, and the adds into slot s's d_gtex (none when
 * that is NULL).  Two slots MAY share one d_tex (one image clamped for one mesh and wrapped for another).
 * As srz_frameset_texture / _texture_grad: the fused clear at nobody's pixels, band sharding (each rank adds the partial sums of its
 * own bands), asynchrony and stream semantics, the 16-byte alignment of the plane buffers and the 4-byte alignment of the textures,
 * SRZ_OPT_APPROX_SHADE having no effect.  BACKWARD: at least one of d_guv and some slot's d_gtex is asked for; d_guv needs every
 * slot's d_tex.  The d_gtex buffers are NOT BIT-REPRODUCIBLE, within srz_frameset_texture_grad's bound; d_guv and the forward are
 * deterministic, bit for bit.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, d_vis, d_uv, slots, d_batch_slot, d_out, d_gout,
 * a slot's d_tex (forward; backward with d_guv), or no d_guv and no d_gtex; n_slots 0 or above SRZ_TEXSET_MAX; n_batch_slot 0 or
 * above 65536; per slot everything srz_frameset_texture refuses of a texture; a short out_bytes; a misaligned pointer; any bit of
 * `flags` but SRZ_FUSED_CLEAR; an output that overlaps an input (the map's bytes count as one) or another output — two slots'
 * d_gtex ranges that overlap each other included. */
#define SRZ_TEXSET_MAX 8u     /* slots of one call */
#define SRZ_TEXSET_NONE 0xffu /* conventional "no slot" value of the map */
typedef struct srz_texset_slot {
  const float *d_tex; /* [tex_frames][tex_h][tex_w][n_ch], as srz_frameset_texture takes it */
  float *d_gtex;      /* backward only: ADDED INTO, or NULL — this slot's texel gradient is not wanted */
  uint32_t tex_w, tex_h, tex_frames, mode; /* per slot: sizes, 1 or the set's frame count, SRZ_TEX_CLAMP / SRZ_TEX_WRAP */
} srz_texset_slot;
int srz_frameset_texture_set(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_uv, const srz_texset_slot *slots,
                             uint32_t n_slots, const uint8_t *d_batch_slot, uint32_t n_batch_slot, uint32_t n_ch, void *d_out,
                             size_t out_bytes, uint32_t flags, void *stream);
int srz_frameset_texture_set_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_uv, const void *d_gout,
                                  const srz_texset_slot *slots, uint32_t n_slots, const uint8_t *d_batch_slot, uint32_t n_batch_slot,
                                  uint32_t n_ch, void *d_guv, uint32_t flags, void *stream);
/* PERSPECTIVE-CORRECT BARYCENTRICS of a visibility buffer, their gradients, and the attribute derivatives under them.  A visibility
 * buffer's alpha, beta are LINEAR IN SCREEN SPACE, the reference's rule and the default of every pass above.  Under a vertex stage
 * that divides by a real w they name the wrong point of the triangle.  With q_k = 1 / w_k the reciprocal clip w of the owner's
 * corners (the divisor the vertex stage used), the weights of the point that projects onto the pixel are
 *   alpha' = alpha q0 / s,  beta' = beta q1 / s,  s = alpha q0 + beta q1 + gamma q2.
 * srz_frameset_perspective writes them into a buffer of the visibility buffer's own four-plane layout, z and the ids copied (the
 * post-divide depth is affine in screen space), so the ATTRIBUTE-SIDE passes run on that buffer unchanged and are then perspective
 * correct: srz_frameset_interpolate, _interpolate_grad (its d_gattr, and its d_gbary, which is then d/dalpha', d/dbeta'), _gbuffer,
 * _shade_visibility, and everything that takes their planes (_texture, _texture_mip, _texture_cube).  The GEOMETRIC passes keep
 * taking the ORIGINAL buffer, whose alpha, beta are the screen-space ones their rules are stated in: srz_frameset_position_grad,
 * _motion, _antialias / _antialias_grad, _peel_visibility, _interpolate_deriv.  srz_frameset_perspective_grad is the backward of the
 * rewrite: from the gradient with respect to alpha', beta' (the planes srz_frameset_interpolate_grad writes on the perspective
 * buffer) to the gradient with respect to the screen-linear alpha, beta — exactly the planes srz_frameset_position_grad takes, with
 * the ORIGINAL buffer — and to q.  srz_frameset_interpolate_deriv_persp gives the per-pixel screen derivatives of an attribute under
 * this interpolation, for srz_frameset_texture_mip, in srz_frameset_interpolate_deriv's planes.
 * d_vis: a visibility buffer of THIS set on this ctx's shard (the original one, in all three calls).  d_q: [q_frames][q_tris][3]
 * float32, 4-byte aligned: srz_frameset_interpolate's attribute layout at one channel (srz_sceneset_corner_attr at n_ch = 1 produces
 * it); q_frames is 1 or the set's frame count, q_tris at least every frame's triangle count.  d_out of srz_frameset_perspective: a
 * visibility buffer, srz_frameset_out_bytes() bytes, 16-byte aligned.  d_gbary_p, d_gbary: [frame][2][local_rows][width] float32,
 * srz_frameset_interpolate_bytes(2) bytes, 16-byte aligned.  d_gq: d_q's shape, ADDED into.  d_attr, n_ch, attr_frames, attr_tris and
 * d_out of srz_frameset_interpolate_deriv_persp: as srz_frameset_interpolate_deriv has them, 1 <= n_ch <= SRZ_ATTR_MAX_CH / 2.  Band
 * sharding, local_rows, stream semantics, asynchrony, owner and nobody ((id & 0x7fffffff) - 1 < the frame's triangle count means an
 * owner, bit 31 of id is the class, gamma = 1 - (alpha + beta) for V and (1 - alpha) - beta for S) as srz_frameset_interpolate /
 * _interpolate_grad.  The first two calls read no position, record or texture and run no vertex stage; the third reads the set's
 * positions exactly as srz_frameset_interpolate_deriv does (a sceneset runs its vertex stage first).
 * THE RULE, in float32, nothing fused but the written fmaf, IEEE divisions.  Per owned pixel, q0, q1, q2 its owner's three words of q
 * (frame 0's when q_frames == 1):
 *   n0 = alpha * q0;  n1 = beta * q1;  n2 = gamma * q2;  s = (n0 + n1) + n2
 *   valid = each of q0, q1, q2 and s is a positive NORMAL float: x >= 2^-126 && x < INFINITY (float compares: a NaN fails).  (Zero,
 *           negative, subnormal, infinite and NaN values all fail, so the rule does not depend on a device's denormal mode: a
 *           corner at or behind the camera plane, or one whose w overflowed, makes its pixels fall back.)
 * FORWARD, srz_frameset_perspective, bit for bit:
 *   valid: alpha' = n0 / s;  beta' = n1 / s;  else alpha' = alpha, beta' = beta (the words copied).
 *   Planes 0 and 1 (z, id): the words of d_vis copied, for EVERY pixel of the shard; a pixel nobody owns (id 0, or a stranger id: an
 *   index outside the frame's triangles) has all four words copied.  Every word of d_out is written whatever `flags` says, so the
 *   result is always a complete buffer.
 * BACKWARD, srz_frameset_perspective_grad: at least one of d_gbary and d_gq is non-null.  ga, gb = d_gbary_p's two words (gamma''s
 * share already folded in, as srz_frameset_interpolate_grad writes them); alpha', beta', s recomputed as above.
 *   valid:  t = fmaf(ga, alpha', gb * beta');  r = 1.0f / s;  g0 = (ga - t) * r;  g1 = (gb - t) * r;  g2 = (-t) * r
 *           galpha = fmaf(g0, q0, -(g2 * q2));  gbeta = fmaf(g1, q1, -(g2 * q2))          -> d_gbary, deterministic, bit for bit
 *           gq[fq][tri][0] += g0 * alpha;  [1] += g1 * beta;  [2] += g2 * gamma            -> d_gq (fq = 0 when q_frames == 1)
 *   else:   galpha = ga, gbeta = gb, and no add.
 *   Nobody pixels of d_gbary: 0 with SRZ_FUSED_CLEAR (frame flags | flags), untouched without, as srz_frameset_interpolate_grad.
 *   d_gq has d_gattr's contract: THE ORDER OF THE ADDS IS UNSPECIFIED, each add rounds, so it is NOT BIT-REPRODUCIBLE between
 *   launches; with n contributing pixels an element lies within n 2^-24 / (1 - n 2^-24) * sum |term| of the exact sum of the float32
 *   terms, and an element with one contributing pixel is exact.  The adds are hardware float atomics: d_gq must be ordinary
 *   (coarse-grained) device memory.  On a sharded ctx each rank produces the partial sums of its own bands.  Words of d_gbary_p at
 *   nobody pixels never reach a result.
 * DERIVATIVES, srz_frameset_interpolate_deriv_persp, bit for bit: area, r, gax, gay, gbx, gby as srz_frameset_interpolate_deriv; per
 * channel with corner values a, b, c and u = the channel interpolated under alpha', beta' and gamma' (gamma' from alpha', beta' by the
 * owner's class) by srz_frameset_interpolate's expression for that class:
 *   e0 = (a - u) * q0;  e1 = (b - u) * q1;  e2 = (c - u) * q2
 *   d/dx = fmaf(e0 - e2, gax, (e1 - e2) * gbx) / s;   d/dy = fmaf(e0 - e2, gay, (e1 - e2) * gby) / s
 *   not valid: srz_frameset_interpolate_deriv's own words (the screen-linear constants).  Nobody pixels as there.  There is no
 *   backward: the planes only select a level.
 * Non-finite alpha, beta propagate as IEEE has them; no input value makes a pass read or write outside its buffers.  Always the exact
 * arithmetic: SRZ_OPT_APPROX_SHADE has no effect.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set, d_vis, d_q, d_out, d_gbary_p or d_attr; both of
 * d_gbary and d_gq null; q_frames not 1 or the frame count; q_tris below some frame's triangle count; what
 * srz_frameset_interpolate_deriv refuses of n_ch, attr_frames and attr_tris; a misaligned pointer; a short out_bytes; any bit of
 * `flags` but SRZ_FUSED_CLEAR; an output that overlaps an input (d_vis, d_q, d_gbary_p, d_attr: d_out == d_vis is an overlap) or the
 * other output. */
int srz_frameset_perspective(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_q, uint32_t q_frames, uint32_t q_tris,
                             void *d_out, size_t out_bytes, uint32_t flags, void *stream);
int srz_frameset_perspective_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_q, uint32_t q_frames, uint32_t q_tris,
                                  const void *d_gbary_p, void *d_gbary, float *d_gq, uint32_t flags, void *stream);
int srz_frameset_interpolate_deriv_persp(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_q, uint32_t q_frames,
                                         uint32_t q_tris, const float *d_attr, uint32_t n_ch, uint32_t attr_frames, uint32_t attr_tris,
                                         void *d_out, size_t out_bytes, uint32_t flags, void *stream);
/* New SHADING DATA for a set made by srz_frameset_create, its triangles untouched (batches[b].tris is ignored and may be NULL): each
 * frame's eye, ka, ks, p, kh, kn, lights and flags, each batch's shader and tex_id.  The structure must be the set's — frame count, size,
 * light counts, batch counts, n_tris per batch — else SRZ_E_INVALID and the set is unchanged; a sceneset is SRZ_E_INVALID (its shading
 * changes with srz_sceneset_update).  Asynchronous copies on the ctx's stream (ordered after the renders submitted there, before the next
 * ones; renders on other streams are the caller's to order), from a pinned staging ring like srz_sceneset_update's.  Every later
 * render and shade of the set uses the new data.  Out of device memory for the work lists of a new build kind: SRZ_E_NOMEM, and
 * renders are refused until an update succeeds (srz_sceneset_update). */
int srz_frameset_update_shading(srz_ctx *ctx, srz_frameset *fs, const srz_frame *frames, int n_frames);
/* display()'s resolve on the device (cv::merge + convertTo(CV_8UC3), src/Render.cpp:61-62): the three colour planes of
 * a rendered buffer (layout of srz_frameset_render) → interleaved 8-bit [frame][local_rows][width][3], round half to even,
 * saturate.  Asynchronous on `stream`.  Any width (sizes whose plane is not a multiple of 4 pixels take a one-pixel-per-thread kernel). */
int srz_frameset_resolve8(srz_ctx *ctx, const srz_frameset *fs, const void *d_planes, void *d_bgr8, size_t bgr8_bytes,
                          void *stream);
/* Re-upload the per-frame data of a sceneset (matrices, eye, lights, shader constants, flags, shader/texture per draw)
 * without re-allocating anything.  The structure must be unchanged: same frame count and size, same mesh slots and face
 * counts per draw, same light counts; otherwise SRZ_E_INVALID (create a new set).  The upload is ONE asynchronous copy
 * on the context's own stream (ordered against srz_target_draw / renders submitted there, no host synchronisation);
 * renders of this set submitted on a caller-provided stream must be ordered against it by the caller. */
int srz_sceneset_update(srz_ctx *ctx, srz_frameset *fs, const srz_scene_frame *frames, int n_frames);

/* ---- the differentiable vertex stage: from the gradient of the SCREEN positions to the mesh and the matrices --------------------
 * srz_frameset_position_grad and srz_frameset_antialias_grad end at d_gpos, nine floats per triangle and frame.  The two calls below
 * close the chain for a sceneset: the set's own positions read out (the values the `pos` graph handle of the torch layer stands
 * for), and the backward of the vertex stage, to what srz_mesh_upload / srz_mesh_update and srz_sceneset_create / _update are given.
 *
 * THE SET'S OWN POSITIONS.  d_pos: [n_frames][pos_tris][9] float32 in the dense stream's order (ax ay z0 bx by z1 cx cy z2), 4-byte
 * aligned, pos_bytes at least n_frames * pos_tris * 36; the triangle index is the visibility buffer's (frame-local); pos_tris at
 * least every frame's triangle count; the triangles behind a frame's last are written as +0.  For a frameset and a sceneset alike: a
 * sceneset runs its vertex stage first, as srz_frameset_position_grad does.  The floats are bit-equal to what the rasteriser reads,
 * whatever the ctx's shard.  Asynchronous on `stream` with the usual semantics.  SRZ_E_INVALID, nothing launched and the output
 * untouched, for: a null ctx, set or d_pos; pos_bytes below the size; a misaligned pointer; pos_tris below a frame's count. */
int srz_frameset_positions(srz_ctx *ctx, srz_frameset *fs, uint32_t pos_tris, float *d_pos, size_t pos_bytes, void *stream);
/* THE BACKWARD OF THE VERTEX STAGE for one mesh slot of a sceneset.  d_gpos: [n_frames][pos_tris][9] float32, what
 * srz_frameset_position_grad and srz_frameset_antialias_grad add into (read only here).  d_gverts: [n_frames][n_verts(mesh_id)][3]
 * float32, the gradient with respect to srz_vertex::pos.  d_gdraw: [n_frames][draw_stride][18] float32, draw_stride at least every
 * frame's draw count; per draw the 16 gradients of ndc_mvp in its own column-major order, then that of zscale, then that of zoffset
 * (a frame's two constants: sum them over its draws).  At least one of the two outputs is non-null; all pointers 4-byte aligned.
 * Only the draws that name mesh_id take part: call once per mesh that is fitted (d_gdraw may be shared between the calls).
 * THE RULE, in float32, nothing fused but the written fmaf, IEEE divisions.  For frame f, vertex v, and each draw j of frame f that
 * names mesh_id, in draw order, with `first` the draw's first frame-local triangle, m and zs the draw's ndc_mvp and zscale, and
 * list(v) the corners (face, k) of the slot's corner list of v, in list order (srz_mesh_upload):
 *   GX = GY = GZ = +0;  for (face, k) in list(v):  p = d_gpos[f][first + face] + 3 k;  GX = GX + p[0];  GY = GY + p[1];  GZ = GZ + p[2]
 *   GX == 0 && GY == 0 && GZ == 0:  this draw contributes nothing for v                      (a NaN is not 0 and goes on)
 *   (x, y, z) = verts[v].pos;   r_i = (m[i] * x + m[4 + i] * y) + (m[8 + i] * z + m[12 + i]),  i = 0..3   (the vertex stage's own expression)
 *   X = r0 / r3;  Y = r1 / r3;  Q = r2 / r3;  inv = 1.0f / r3;  gq = GZ * zs
 *   g0 = GX * inv;  g1 = GY * inv;  g2 = gq * inv;  s = gq * Q;  s = fmaf(GY, Y, s);  s = fmaf(GX, X, s);  g3 = (-s) * inv
 *   c = 0..2:  t = m[4 c] * g0;  t = fmaf(m[4 c + 1], g1, t);  t = fmaf(m[4 c + 2], g2, t);  t = fmaf(m[4 c + 3], g3, t);
 *              d_gverts[f][v][c] = d_gverts[f][v][c] + t
 *   d_gdraw[f][j][4 c + i] += g_i * (x, y, z)[c]  (c = 3: g_i);   d_gdraw[f][j][16] += GZ * Q;   d_gdraw[f][j][17] += GZ
 * d_gverts is a GATHER: the one thread that owns (f, v) adds once per contributing draw, in draw order — DETERMINISTIC, bit for bit;
 * an element with no contributing draw is LEFT UNTOUCHED.  The skip is what keeps hidden, culled and non-finite triangles, whose
 * d_gpos is zero, from poisoning a vertex they share (a vertex on the camera plane, r3 == 0, would otherwise yield 0 * inf).
 * d_gdraw is ADDED into, a sum over the draw's contributing vertices IN AN UNSPECIFIED ORDER AND TREE: not bit-reproducible; with n
 * contributing vertices an element lies within n 2^-24 / (1 - n 2^-24) * sum |term| of the exact sum of its float32 terms, and an
 * element with one term is exact; draws of other slots and the words behind a frame's last draw are untouched.  The adds are
 * hardware float atomics, one per workgroup of 256 vertices, draw and value: d_gdraw must be ordinary (coarse-grained) device memory.
 * Non-finite values propagate as IEEE has them; no input value makes the pass read or write outside its buffers.  The pass reads no
 * visibility buffer and no triangle, and is linear in d_gpos apart from the skip: on a sharded ctx each rank transforms its own
 * partial d_gpos.  The vertices and matrices are what the device holds when the pass runs: order it against srz_mesh_update and
 * srz_sceneset_update as a render is ordered.  Asynchronous on `stream`.
 * SRZ_E_INVALID, the outputs untouched and nothing launched, for: a null ctx, set or d_gpos; a set that is not a sceneset; a mesh_id
 * the set does not draw, or whose slot was uploaded anew (srz_mesh_upload) since the set was created; both outputs null; pos_tris
 * below a frame's triangle count; with d_gdraw, draw_stride below a frame's draw count; a misaligned pointer; an output that
 * overlaps d_gpos or the other output. */
int srz_sceneset_vertex_grad(srz_ctx *ctx, srz_frameset *fs, int mesh_id, const float *d_gpos, uint32_t pos_tris, float *d_gverts,
                             float *d_gdraw, uint32_t draw_stride, void *stream);
/* PER-VERTEX ATTRIBUTES of one mesh slot TO THE SET'S TRIANGLE STREAM, and back.  srz_frameset_interpolate takes attributes per corner,
 * [frame][T][3][n_ch] in the frame's triangle order; these two calls lay a slot's per-vertex data out that way on the device and fold
 * the per-corner gradient back to the vertices.
 * FORWARD.  d_attr: [attr_frames][n_verts(mesh_id)][n_ch] float32, attr_frames 1 (one array for every frame) or the set's frame count,
 * 1 <= n_ch <= SRZ_ATTR_MAX_CH; d_out: [n_frames][pos_tris][3][n_ch] float32 — what srz_frameset_interpolate takes with attr_frames =
 * n_frames and attr_tris = pos_tris; pos_tris at least every frame's triangle count.  For every frame f, every draw of frame f that names
 * mesh_id, with `first` the draw's first frame-local triangle, every face and k = 0..2:
 *   d_out[f][first + face][k][ch] = d_attr[f or 0][faces[face][k]][ch]
 * EVERYTHING ELSE IN d_out IS LEFT UNTOUCHED (the triangles of other slots' draws, those behind a frame's count): call once per slot
 * into one buffer the caller has filled first.
 * BACKWARD.  d_gout: laid out like d_out; d_gattr: [n_frames][n_verts][n_ch] float32, EVERY element written:
 *   sum = +0;  for each draw of frame f that names mesh_id, in draw order:  for corner c in list(v), in list order:
 *     sum = sum + d_gout[f][first + c / 3][c % 3][ch];          d_gattr[f][v][ch] = sum
 * one running float32 sum; a frame that does not draw the slot gets +0.  A GATHER, no atomics: DETERMINISTIC, bit for bit (the
 * gradient of a [n_verts][n_ch] array shared by the frames is the caller's sum over the frames).
 * Both are asynchronous on `stream`; neither runs the vertex stage nor reads a triangle of the set.
 * SRZ_E_INVALID, nothing written and nothing launched, for: a null ctx or set; a set that is not a sceneset; a mesh_id the set does
 * not draw, or whose slot was uploaded anew (srz_mesh_upload) since the set was created; n_ch == 0 or above SRZ_ATTR_MAX_CH; pos_tris
 * below a frame's triangle count; a null buffer; attr_frames not 1 or the frame count; a pointer that is not 4-byte aligned; an
 * output that overlaps the input. */
int srz_sceneset_corner_attr(srz_ctx *ctx, srz_frameset *fs, int mesh_id, const float *d_attr, uint32_t n_ch, uint32_t attr_frames,
                             float *d_out, uint32_t pos_tris, void *stream);
int srz_sceneset_corner_attr_grad(srz_ctx *ctx, srz_frameset *fs, int mesh_id, const float *d_gout, uint32_t n_ch, float *d_gattr,
                                  uint32_t pos_tris, void *stream);

/* ---- multi-GPU exchange: the band shards of every rank → full row-major frames on every rank ------------------------
 * One process per GPU.  Rank 0 makes an id (srz_comm_unique_id), the host program hands the 128 bytes to every rank
 * (MPI, torch.distributed, a file), and every rank calls srz_comm_create, which builds the RCCL communicator (librccl is
 * loaded on first use) and sets the ctx's shard like srz_set_shard(ctx, rank, world).
 * srz_frameset_allgather = ncclAllGather over xGMI of this rank's shard (what srz_frameset_render / _resolve8 wrote:
 * [frame][4 planes | 1][local_rows][W x 4 | W x 3 bytes]) into d_gathered (world x shard bytes), then one HIP pass that
 * de-interleaves the round-robin bands into d_full = [frame][planes][bands_per_rank*world*32 rows][row] (rows >= height
 * are padding).  Asynchronous on `stream`; to overlap the exchange of step k with the render of step k+1 give the two
 * different streams and shard buffers and order them with events (bench.py does).  srz_frameset_deinterleave is the second
 * half alone (for a host program that brings its own collective). */
#define SRZ_EXCHANGE_PLANES 0 /* the 4 float planes, 16 bytes per pixel */
#define SRZ_EXCHANGE_BGR8 1   /* display()'s resolved image, 3 bytes per pixel */
typedef struct srz_comm srz_comm;
int srz_comm_unique_id(uint8_t *out128);
int srz_comm_create(srz_ctx *ctx, const uint8_t *id128, int rank, int world, srz_comm **out);
void srz_comm_destroy(srz_ctx *ctx, srz_comm *comm);
size_t srz_frameset_exchange_bytes(const srz_ctx *ctx, const srz_frameset *fs, int what); /* bytes of this rank's shard */
int srz_frameset_allgather(srz_ctx *ctx, srz_comm *comm, const srz_frameset *fs, const void *d_shard, void *d_gathered,
                           void *d_full, int what, void *stream);
int srz_frameset_deinterleave(srz_ctx *ctx, const srz_frameset *fs, const void *d_gathered, void *d_full, int what,
                              void *stream);
/* The exchange WITHOUT a second pass.  The rank renders (srz_frameset_render) or resolves (srz_frameset_resolve8) its shard
 * directly at  d_gathered + rank * srz_frameset_exchange_bytes()  and this call is one IN-PLACE ncclAllGather that fills in the
 * other ranks' shards around it: no staging copy, no de-interleave kernel, nothing but the xGMI transfers.  The result stays in
 * the all-gather's own order, "rank-major shards":
 *     [rank][frame][plane: z,c0,c1,c2 | 1][bands_per_rank * 32 rows][row bytes]
 * row y of a frame lives in the shard of rank rank(y / 32) (THE BAND MAP at srz_set_shard) at local row (y / 32 / world) * 32 + y % 32:
 * srz_frameset_gathered_row_offset() returns that row's byte offset in d_gathered, and srz_frameset_read_gathered_frame() brings
 * one frame to the host as row-major planes ([4][H][W] float, or [H][W][3] bytes for SRZ_EXCHANGE_BGR8), de-interleaving in the
 * device→host copy itself (one strided copy per rank and plane).  A device-side consumer that needs row-major planes uses
 * srz_frameset_allgather (all-gather + one HIP pass) instead.  With world = 1 the call does nothing. */
int srz_frameset_allgather_inplace(srz_ctx *ctx, srz_comm *comm, const srz_frameset *fs, void *d_gathered, int what, void *stream);
size_t srz_frameset_gathered_row_offset(const srz_ctx *ctx, const srz_frameset *fs, int what, int frame, int plane, int row);
int srz_frameset_read_gathered_frame(srz_ctx *ctx, const srz_frameset *fs, const void *d_gathered, int what, int frame,
                                     void *host_out, void *stream);

/* ---- the TILE-SPARSE exchange: every rank sends only the 32x32 tiles its render drew into ----------------------------------------
 * The result is exactly the layout of srz_frameset_allgather_inplace (rank-major shards [rank][frame][plane][bands_per_rank*32][row],
 * rows found by THE BAND MAP at srz_set_shard; srz_frameset_gathered_row_offset / _read_gathered_frame / _deinterleave work on it):
 * the rank renders or resolves into its own slot of d_gathered, and the unpack fills in the other ranks' slots.  Padding rows stay
 * unspecified.
 * A TOUCHED tile of a rank's shard is one its last render did not clear: some triangle's bounding box reaches it (k_bin's tile count
 * is not 0 — the test the fused clear uses), or the frame was rendered WITHOUT SRZ_FUSED_CLEAR (frame flags | render flags), which
 * leaves the caller's old contents in every tile: then every tile of that frame counts as touched.  Every other tile holds the clear
 * values bit for bit (z = +inf, colour 0; SRZ_EXCHANGE_BGR8: bytes 0,0,0) and is written by the receivers themselves.
 * MESSAGE (one per rank, identical layout on every rank, 16-byte aligned; T = n_frames * bands_per_rank * tiles_x, tiles_x = ceil(W/32)):
 *     bytes  0..3   uint32  touched tiles (= tiles in the payload)
 *            4..7   uint32  T
 *            8..15  uint64  message bytes = payload offset + touched * tile bytes
 *     16 ..         uint32  table[frame][local band][tile x]: the tile's slot in the payload, or 0xffffffff (not touched: the clear
 *                           values); bands a rank does not have (a short last group) are never touched
 *     payload offset = 16 + 4 T rounded up to 16:
 *                   the touched tiles, in table order (slot k = the k-th touched tile: per-band counts + a scan, no atomics — two packs
 *                   of one render give the same bytes), each a whole 32x32 block [plane][32 rows][32 pixels]: 16384 bytes for
 *                   SRZ_EXCHANGE_PLANES (z, c0, c1, c2 floats), 3072 for SRZ_EXCHANGE_BGR8 (B,G,R bytes); pixels outside the frame
 *                   (x >= W, rows past the band's end) are 0.
 * srz_frameset_sparse_capacity: bytes of the largest message (every tile touched) — the size of d_msg; 0 for a bad `what`.
 * srz_frameset_sparse_pack: this rank's message from its shard d_shard (what srz_frameset_render / _resolve8 wrote; for the in-place
 *   layout: d_gathered + rank * srz_frameset_exchange_bytes()).  It reads the tile counts of the set's LAST render, so it must be
 *   enqueued AFTER that render on the same stream (or behind it by an event) and BEFORE the set's next render or srz_frameset_stats,
 *   which overwrite them (and before an srz_sceneset_update that changes frame flags).  msg_bytes >= capacity, else SRZ_E_INVALID.
 *   Asynchronous on `stream`.
 * srz_frameset_sparse_unpack: the second half alone, for a caller that brings its own collective (and for one GPU playing every
 *   rank): the message of rank p at d_recv + p * msg_stride (msg_stride a multiple of 16) → the slots of every rank but this one in
 *   d_gathered, real pixels only.  Asynchronous on `stream`.
 * srz_frameset_allgather_sparse: pack first, then this call (every rank, same stream order):
 *   1. ncclAllGather of every rank's message header and recv_bytes into a small device buffer of the communicator;
 *   2. one device→host copy and a stream synchronise: the host learns M, the largest message (rounded up to 16).  THE CALL'S ONE
 *      BLOCKING POINT.  If any rank's recv_bytes < world * M, EVERY rank returns SRZ_E_NOMEM (srz_last_error names the bytes needed):
 *      no rank may leave alone while its peers enter the next collective;
 *   3. ncclAllGather of M bytes of every rank's d_msg (which holds the capacity) into d_recv, then srz_frameset_sparse_unpack with
 *      stride M.
 *   With world = 1 the call does nothing.  The frameset must be of this communicator's shard (SRZ_E_INVALID). */
size_t srz_frameset_sparse_capacity(const srz_ctx *ctx, const srz_frameset *fs, int what);
int srz_frameset_sparse_pack(srz_ctx *ctx, srz_frameset *fs, const void *d_shard, void *d_msg, size_t msg_bytes, int what, void *stream);
int srz_frameset_sparse_unpack(srz_ctx *ctx, const srz_frameset *fs, const void *d_recv, size_t msg_stride, void *d_gathered, int what,
                               void *stream);
int srz_frameset_allgather_sparse(srz_ctx *ctx, srz_comm *comm, const srz_frameset *fs, const void *d_msg, void *d_recv, size_t recv_bytes,
                                  void *d_gathered, int what, void *stream);

/* ---- device-resident framebuffer = RenderingPipeline's m_zBuffer + m_channels kept in HBM between calls ----------
 * clear(Color|Depth) immediately followed by a draw costs nothing (fused into the raster kernel); planes come back to
 * the host only when asked for, and display() only needs the 3-byte resolved image. */
typedef struct srz_target srz_target;
int srz_target_create(srz_ctx *ctx, int width, int height, srz_target **out); /* starts cleared (z=+inf, colour 0) */
void srz_target_destroy(srz_ctx *ctx, srz_target *t);
int srz_target_clear(srz_ctx *ctx, srz_target *t, int color, int depth);      /* = RenderingPipeline::clear(Buffers) */
/* draw frame 0 of a 1-frame set (srz_frameset_create / srz_sceneset_create of the target's size) into the target */
int srz_target_draw(srz_ctx *ctx, srz_target *t, int primitive, srz_frameset *fs, srz_stats *stats);
int srz_target_read(srz_ctx *ctx, srz_target *t, float *z, float *c0, float *c1, float *c2); /* NULL planes are skipped */
int srz_target_read_bgr8(srz_ctx *ctx, srz_target *t, uint8_t *bgr8);         /* display()'s resolve, W*H*3 bytes */
/* synchronous: runs the counting variant of the kernels once and returns the counters */
int srz_frameset_stats(srz_ctx *ctx, srz_frameset *fs, srz_stats *stats);
/* Algorithmic bytes of one render of the frameset on this ctx (SURVEY §8d / DESIGN.md):
 * 16*W*local_rows + 96*N_tri + 24*N_lights + B_tex per frame. n_shaded_tex = texture-shaded pixels. */
uint64_t srz_frameset_algorithmic_bytes(const srz_ctx *ctx, const srz_frameset *fs);
/* Average device time (ms) per srz_frameset_render since the last call with reset!=0, measured with hipEvents on
 * the launch stream: ms4[0] = setup+binning kernels, ms4[1] = raster kernel (visibility), ms4[2] = shade kernel up to
 * the join with the clear kernel that runs beside both on a second stream, ms4[3] = whole pipeline. */
int srz_kernel_time_ms(srz_ctx *ctx, int reset, double *ms4, int *launches);
/* ms4[3] of each timed render since the last reset, in submission order (at most cap values, *n = how many): the
 * per-step distribution (p10 / median / p90) bench.py prints; *span_ms (may be NULL) = from the first of them starting
 * to the last of them ending — renders submitted to different streams overlap, the span is what they took together.
 * Call it before the resetting srz_kernel_time_ms. */
int srz_kernel_time_samples(srz_ctx *ctx, float *out, int cap, int *n, double *span_ms);
/* enabled: 0 off; 1 the whole launch set only (ms4[3]; two events per render); 2 also the three groups (four events per
 * render — every event is a barrier in the launch stream, ≈4 µs each, so throughput is measured with 1 and broken down with 2) */
int srz_set_kernel_timing(srz_ctx *ctx, int enabled);
int srz_sync(srz_ctx *ctx);
/* Page-lock `bytes` of host memory at `ptr` / release it again (hipHostRegister / hipHostUnregister behind the C ABI, so that a
 * binding needs no HIP header).  The host-buffer entry points — srz_draw, srz_draw_scene, srz_draw_batch — move planes that lie in a
 * registered range by DMA at the link's rate instead of through the runtime's pageable staging copies (MI355X, 1024^2: see
 * DESIGN.md §5 "PCIe-inclusive rate").  Register a buffer once after allocating it (the reference's m_zBuffer / m_channels live as
 * long as the pipeline object), unregister it before freeing it.  What these calls replace on the reference's side: nothing — its
 * framebuffer never leaves host memory (src/Render.cpp:46-64); this is the price of the seam at src/Rasterizer.cpp:183-240. */
int srz_host_register(srz_ctx *ctx, void *ptr, size_t bytes);
int srz_host_unregister(srz_ctx *ctx, void *ptr);
/* self-check of the device arithmetic: compares the kernels' short exact reciprocal / square-root sequences with the
 * IEEE expansions on all 2^32 binary32 operands. out4 = {operands on the fast path, rcp, sqrt, 1/sqrt mismatches} */
int srz_verify_fastmath(srz_ctx *ctx, uint64_t *out4);
/* Same for the division-by-reciprocal sequence of the scalar-tail shaders (texel / 255, intensity / distance):
 * out3 = { pairs tested, mismatches vs a / b on pseudo-random in-range pairs, mismatches of texel / 255 for texel 0..255 }. */
int srz_verify_fastdiv(srz_ctx *ctx, uint64_t *out3);
/* Same for the optimistic x^p of the shading builds for non-integer exponents (exp2(p log2 x) in binary64 with a rounding-safety
 * flag): every binary32 x in [2^-40, 1] at exponent p (a non-integer in (0, 4096]) against the correctly rounded path.
 * out4 = { operands, results that differ although the flag was clear (must be 0), flagged operands with a normal result >= 2^-120
 * (ambiguous roundings), flagged operands with a smaller result } — the tiles of flagged pixels are shaded by the generic build. */
int srz_verify_fastpow(srz_ctx *ctx, float p, uint64_t *out4);
/* Same for the attenuation distance of the scalar Blinn-Phong, sqrt(dx^2 + dy^2) evaluated in binary64 and rounded once
 * (src/Shader.cpp:516-523 of the reference): the FAST builds take two binary64 Heron steps from the binary32 root instead of the
 * binary64 square root, with a flag when the result lies within 8 binary64 ulps of a binary32 rounding boundary.  4.3e9 pseudo-random
 * pairs (random / close exponents / few significant bits / scaled Pythagorean pairs whose root IS a rounding boundary):
 * out5 = { pairs, results that differ although the flag was clear (must be 0), flagged random pairs, flagged Pythagorean pairs,
 * flagged few-significant-bit pairs }. */
int srz_verify_fastlen(srz_ctx *ctx, uint64_t *out5);
/* diagnostic only (tests): counters the LAST render of the set left — out6 = { tiles taken by the ordered rasteriser (after srz_frameset_peel_visibility: tiles fed from the frame's stream), tiles the FAST
 * shading builds handed to the generic build, capacity of a tile-list sub-pool, largest demand a sub-pool reported, workgroups of the
 * side-stream clear (a batch-sized set measures them on the device within its first 24 renders, and again every 4096), 1 once that measurement has been taken }; waits for the device */
int srz_frameset_debug_counters(srz_ctx *ctx, srz_frameset *fs, uint32_t *out6);
/* diagnostic only (tests): which builds of the shading kernels the set's next colour render or shade launches — out2 = { mask: bit k =
 * some frame is shaded by FAST build kind k (0..3: 1..4 lights with an integer exponent 0..256; 4..7: the same with a BUMP /
 * DISPLACEMENT batch; 8..11: 1..4 lights with a non-integer exponent in (0, 4096]), 1 if some frame takes the generic build };
 * host state only, launches nothing, does not wait */
int srz_frameset_shade_kinds(srz_ctx *ctx, srz_frameset *fs, uint32_t *out2);
/* diagnostic only: raw device counters of the last stats run (layout = csrc/srz_device.h ST_*); returns their count */
int srz_debug_counters(srz_ctx *ctx, uint64_t *out, int n);

#ifdef __cplusplus
}
#endif
#endif /* SRZ_H_ */
