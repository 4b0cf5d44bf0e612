// srz_device.h — device-side data layout shared by the kernels (srz_kernels.hip) and the C-ABI host code
// (srz_api.hip).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/srz.h"

namespace srz {

constexpr int TILE = 32;             // one wavefront owns one 32x32-pixel tile (its z + owner planes live in LDS)
constexpr int BAND = 32;             // band = one row of tiles; the unit of multi-GPU sharding and of binning
// k_raster: ONE wave (= one tile) per workgroup, so a long tile never pins the LDS / wave slots of finished neighbours and
// the dispatcher load-balances tile by tile.  Its tile state is one 64-bit key per pixel; rows are padded to 33 keys
// (264 B): lanes that hit the same column of consecutive rows land in different bank pairs, and the 33rd key of every
// row doubles as scratch for the item expansion.  8448 B per wave = 19 waves per CU.
constexpr int KEY_STRIDE = TILE + 1;
// LDS row stride (dwords) of the ORDERED rasteriser's z / owner planes (k_raster_slow)
constexpr int LDS_STRIDE = 32;
// ---- which rank owns which 32-row band (round 6) ----------------------------------------------------------------------------------
// Every group g = b / world of `world` consecutive bands hands ONE band to every rank, ROTATED by BAND_ROT steps per group:
//     rank(b) = (b + BAND_ROT * (b / world)) % world,   local band index = b / world,
//     band(lb, rank) = lb * world + (rank - BAND_ROT * lb) mod world.
// (Rounds 1-5: rank = b % world.  A scene whose period in bands is a multiple of `world` — config 4's four rows of cows, 16 bands each,
// on 8 ranks — then gave rank r the SAME two slices of every cow: per-rank render times 1.19-1.21 x their mean.  With a rotation a rank
// meets a different slice in every group.  Measured with one GPU playing every rank of 8 (bench.py emulate_shards, max / mean of the
// per-rank render times, configs 2 / 4 / 5): no rotation 1.05-1.06 / 1.19-1.21 / 1.02-1.04; 1 step 1.15 / 1.07-1.09 / 1.02-1.04; 3 steps
// 1.12 / 1.09 / 1.02; 5 steps 1.06 / 1.09 / 1.04 — five it is (one step where five is a multiple of the world).  Buffers, local indices
// and the exchange are unchanged: the gathered layout is still [rank][frame][plane][local band][32 rows].)
#ifndef SRZ_BAND_ROT
#define SRZ_BAND_ROT 5 /* (A/B builds: 0 = the plain b % world of rounds 1-5) */
#endif
__host__ __device__ inline int band_rot(int world) { return (SRZ_BAND_ROT % world) ? SRZ_BAND_ROT : (SRZ_BAND_ROT ? 1 : 0); }
__host__ __device__ inline int band_of(int lb, int rank, int world) {
  if (world == 1) return lb; // (the single-GPU case pays no division: a wave-uniform branch in the kernels)
  int j = (rank - band_rot(world) * lb) % world;
  return lb * world + (j < 0 ? j + world : j);
}
__host__ __device__ inline int rank_of_band(int b, int world) { return (b + band_rot(world) * (b / world)) % world; }
constexpr uint32_t NO_TRI = 0xffffffffu;
// per-frame atomic counters sit 128 bytes apart: atomics on the words of ONE cache line serialise (~10 ns each across the
// device) as if they were one address — with 16 frames of 4096^2 that was the whole of k_raster's time
constexpr uint32_t CNT_STRIDE = 32;
// FrameDesc::flags, internal (set by the host): 1..4 lights and an integer exponent 0..256 → the FAST build of k_shade for that count
constexpr uint32_t FD_FAST_SHADE = 0x100u, FD_NL_SHIFT = 9; // (+ the light count 1..4 in bits 9..11)
constexpr uint32_t FD_BUMPY = 0x1000u;                   // some batch of the frame is BUMP / DISPLACEMENT (FAST builds with those variants)
constexpr uint32_t FD_PACKED = 0x4000u;                  // fewer than 2^22 - 1 triangles and at most 1024 batches: a tile-list entry is
                                                         // triangle index | batch << 22 (k_shade stages the tile's triangles without
                                                         // a gather of their batch ids), and the depth keys' tie-breaks carry list positions
constexpr uint32_t PACK_IDX_BITS = 22, PACK_IDX_MASK = (1u << PACK_IDX_BITS) - 1u, PACK_MAX_BATCHES = 1024;
constexpr uint32_t FD_GREY = 0x8000u;                    // ka, ks and every light's intensity have three bit-equal channels (FrameK::grey in srz_kernels.hip)
constexpr uint32_t FD_GENPOW = 0x2000u;                  // a non-integer exponent in (0, 4096]: FAST builds whose power is pow_fast (exp2(p log2 x) in binary64 with a rounding-safety flag)
constexpr uint32_t SHADE_KIND_GENERIC = 12;              // k_shade builds: kinds 0..3 = FAST for 1..4 lights, 4..7 = the same + BUMPY,
                                                         // 8..11 = FAST for 1..4 lights with any exponent (GENPOW), 12 = generic
// the build kind that shades a frame of these flags (FrameDesc::flags, as classify_frames in srz_api.hip sets them)
__host__ __device__ constexpr uint32_t frame_kind(uint32_t flags) {
  return (flags & FD_FAST_SHADE) ? ((flags >> FD_NL_SHIFT) & 7u) - 1u + ((flags & FD_BUMPY) ? 4u : 0u) + ((flags & FD_GENPOW) ? 8u : 0u)
                                 : SHADE_KIND_GENERIC;
}
// the kind a <FASTNL, BUMPY> build of k_shade / k_shade_vis serves (FASTNL: 1..4 lights, -1..-4 the same with GENPOW, 0 generic)
template <int FASTNL, bool BUMPY> constexpr uint32_t build_kind() {
  return frame_kind(FASTNL == 0 ? 0u
                                : FD_FAST_SHADE | (uint32_t)(FASTNL < 0 ? -FASTNL : FASTNL) << FD_NL_SHIFT | (BUMPY ? FD_BUMPY : 0u) |
                                      (FASTNL < 0 ? FD_GENPOW : 0u));
}
constexpr uint32_t N_WORK_LISTS = 8 * (SHADE_KIND_GENERIC + 1);
constexpr uint32_t UNLISTED = 0xffffffffu; // tile_off of a tile whose list did not fit the record pool
// Binning is O(triangles): k_setup / k_chunks sort every GROUP of GROUP_TRIS (512) consecutive triangles by the 32-row bands their
// bounding boxes reach (LDS count / scan / fill, no global atomics) into the group's own region of ENT_PER_GROUP 8-byte
// entries {triangle, tile-x range}, and write one descriptor word per (group, local band): first entry << 16 | entries.
// k_bin's (frame, band) workgroup then reads only its own entries.  A group whose entries do not fit the region (on average
// more than 4 bands per triangle: huge triangles) gets DESC_RAW in every band, and the band workgroups walk that group's
// bounding boxes themselves.
#ifndef SRZ_GROUP_K
#define SRZ_GROUP_K 2 // triangles per thread of a k_setup workgroup pass (measured 1 / 2 / 4: setup + bin 52 / 56 / 58 µs per 256 frames
                      // of config 2, 106 / 99 / 104 µs per 32 frames of config 4)
#endif
constexpr uint32_t GROUP_K = SRZ_GROUP_K, GROUP_TRIS = 256u * GROUP_K, ENT_PER_GROUP = 4u * GROUP_TRIS, DESC_RAW = 0xffffffffu,
                   MAX_LOCAL_BANDS = 1024;
constexpr int MAX_TEX = 64;
constexpr int MAX_MESH = 256;

// Screen-space bounding box of a surviving triangle (Triangle::calcBoundingBox, src/Triangle.cpp:243-257),
// 8 bytes so that a wave scans 64 of them with one coalesced 512-B load. Culled / non-finite: sx > ex.
struct __attribute__((aligned(8))) BBox {
  int16_t sx, sy, ex, ey;
};

// The triangle stream in HBM: the boundary's 96-byte srz_tri records (36 bytes of positions, 60 of normals + texture
// coordinates) as uploaded — what k_shade stages per tile — plus a DENSE COPY OF THE POSITIONS, 9 floats per triangle, made at
// upload (or written by k_vertex beside the record).  k_setup streams the dense copy (36 bytes per triangle instead of the 96
// its cache lines used to drag in) and k_raster gathers a tile's triangles from it through the 4-byte indices of the tile's list,
// the bounding box from bbox[] (8 bytes): there is no per-triangle record written by k_setup any more (it was 48 bytes written
// per kept triangle, every frame).  The kernels address triangle i's positions at tri_pos + i * pos_stride; srz_draw, which
// re-uploads one frame's records per call, makes no copy: tri_pos = the records themselves, pos_stride = 24.
// (the per-triangle constants of the coverage tests — 1 / fmsub(ABx,ACy,ACx*ABy) for the V columns, ABx*ACy - ABy*ACx for the
// S columns — are recomputed by k_raster from the positions, once per list entry and 64 entries at a time)
constexpr uint32_t TRI_POS_F = 9, TRI_AOS_F = 24; // floats

// What the Shader object bound to a batch holds (type + texture), resolved on the host at render time
struct __attribute__((aligned(8))) ShadeDescG {
  int32_t shader, tw, th, _pad;
  const uint32_t *tex;
};

// One mesh instance of one frame for the device vertex stage
struct DrawDesc {
  const srz_vertex *verts;
  const uint32_t *faces;
  uint32_t n_faces;
  uint32_t tri_off; // first output triangle (global index into tris[])
  uint32_t frame;   // the frame this draw belongs to (k_vertex's own triangle setup reads its size and eye)
  float zscale, zoffset;
  float ndc_mvp[16], normal_m[16];
};

struct FrameDesc {
  int32_t width, height;
  float eye[3];
  float ka[3];
  float ks[3];
  float p, kh, kn;
  uint32_t n_lights, light_off;  // into lights[]
  uint32_t n_tris, tri_off;      // into tris[] / bbox[] / tri_batch[]
  uint32_t n_batches, batch_off; // into sdesc[]
  uint32_t flags;
  uint32_t n_local_bands;        // bands of this frame owned by this ctx
  uint32_t chunk_off;            // into chunk_rows[]: first 64-triangle chunk of this frame
  uint32_t group_off;            // into band_desc[] / band_ent[]: first group (GROUP_TRIS triangles) of this frame
};

// counters accumulated by the STATS kernel variants (same order as srz_stats)
enum { ST_TRIS = 0, ST_CULLED, ST_PIXEL_TESTS, ST_FRAGMENTS, ST_SHADED, ST_VISIBLE, ST_VISIBLE_TEX,
       ST_DBG_CYC_A, ST_DBG_CYC_B, ST_DBG_CYC_C, ST_DBG_MAX_WAVE, ST_DBG_IEEE_TILES, ST_DBG_BLOCKS, ST_COUNT };

struct RenderArgs {
  const FrameDesc *frames;
  const srz_tri *tris;           // the records (k_shade)
  const float *tri_pos;          // [triangle * pos_stride]: ax ay z0 bx by z1 cx cy z2 (k_setup, k_raster)
  uint32_t pos_stride;           // floats: 9 (the dense copy) or 24 (the records themselves)
  const BBox *bbox;
  uint32_t *chunk_rows;          // per 64-triangle chunk: min sy | max ey << 16 of its kept triangles (k_setup → k_bands)
  uint32_t *band_desc;           // [group][n_local_bands]: first entry << 16 | entries of the group in that band, or DESC_RAW
  uint2 *band_ent;               // [group][ENT_PER_GROUP]: {triangle index in the frame, first tile x | last tile x << 16}
  const uint16_t *tri_batch;
  const srz_light *lights;
  const ShadeDescG *sdesc;       // per batch of the set, in frame order (FrameDesc::batch_off)
  // per-tile triangle lists, UNORDERED (the rasteriser's result does not depend on list order): triangle indices in a pool
  // of n_sub equal sub-pools with one bump allocator each; a (frame, band) workgroup of k_bin takes its band's entries
  // from sub-pool (workgroup id & sub_mask) in one allocation.  A band that does not fit is left UNLISTED: its tiles are
  // rasterised by k_raster_slow straight from the frame's stream, and the host grows the pool before the next render.
  uint32_t *pool;
  uint32_t *pool_heads;          // [n_sub] records requested from each sub-pool by this render (zeroed by k_setup)
  uint32_t *pool_demand;         // pinned host memory laid out like pool_heads: what this render asked of each sub-pool (latency build of k_raster)
  uint32_t pool_sub_cap, pool_sub_mask;
  uint2 *tile_info;              // [frame][local band][tiles_x]: x = entries in the tile's list (0: k_clear's tile), y = its first
                                 // index in pool[], or UNLISTED — one 8-byte load tells a tile's wave both
  uint32_t *slow_list;           // tiles (frame * tiles_per_frame + tile) left to the ordered rasteriser
  uint32_t *slow_count;
  uint32_t other_streams;        // host hint: the previous render of this ctx went to another stream (lanes): k_shade's grid follows
  uint32_t clear_in_raster;      // small jobs: no k_clear is launched, k_raster's waves clear the tiles no bbox reaches
  uint32_t force_ordered;        // every touched tile goes to k_raster_slow (SRZ_ORDERED_RASTER, counting runs)
  uint32_t any_ordered;          // host hint: SRZ_ORDERED_RASTER is set on the render or on some frame (k_raster_slow gets a large grid)
  uint32_t force_generic;        // every frame is shaded by the generic build of k_shade (counting runs)
  uint32_t any_generic;          // some frame is not FD_FAST_SHADE (else the generic build only serves redo_list)
  uint4 *redo_list;              // work-list entries of the tiles the FAST builds of k_shade hand to the generic one
  uint32_t *redo_count;
  uint32_t *vis;                 // owner ids per tile [frame][local band][tile x][PIX_SLOT ids]: 8, 16 or 32 bits each (srz_kernels.hip, the hand-off)
  // k_shade's work lists of the tiles that have an owner, work_cap entries each (srz_kernels.hip, the hand-off)
  uint4 *worklist;
  uint64_t kind_slots;           // storage slot of build kind k in worklist[]: (kind_slots >> 4k) & 15 (srz_kernels.hip, work_slot)
  uint32_t *work_count;          // [list * CNT_STRIDE]: word 0 = entries (zeroed by k_setup, bumped by k_raster), word 1 = k_shade's cursor
  uint32_t work_cap;
  uint32_t tiles_x, n_local_bands, n_frames;
  float *out;             // [frame][4][local_rows][width]
  uint64_t frame_stride;  // floats per frame in out = 4*local_rows*width
  uint32_t local_rows;    // rows per plane in out
  int32_t shard_rank, shard_world;
  uint32_t flags_or;      // OR-ed into every frame's flags (SRZ_FUSED_CLEAR / SRZ_UNIFIED)
  unsigned long long *stats;
  const uint32_t *clear_wgs_dev; // k_clear: workgroups that take part, read on the device (ClearCtl::wgs; 0 = the first candidate); null: the whole grid
};

// The grid of the side-stream clear is MEASURED per frameset, on the device (srz_api.hip, srz_frameset::ClearTune; k_clear_tune): while a
// set measures, k_clear is launched with CLEAR_GRID_MAX workgroups of which the first ClearCtl::wgs take part, and a one-thread kernel at
// the end of every render reads the wall clock, files the time since the previous render's end under the grid in use and moves on —
// candidates a b c (ascending) in blocks of CLEAR_TUNE_BLOCK renders (the first sample of a block, the previous grid's tail, is dropped;
// a grid more than 5 % behind the best smaller one ends this pass: the larger ones would only be worse and are not tried); a grid tried
// after the best of them and more than 5 % behind it is dropped, the others go round once more in the mirrored order c b a (the first
// renders after idle run up to 10 % slower: the mirror takes a linear ramp out of the comparison, and the ramp is why an EARLIER grid is
// never dropped on the first pass), the smallest median of the four samples wins.  No host synchronisation, no event query: the
// decision takes effect with the next render whatever the host's run-ahead, and reaches the host through a word of mapped memory.
constexpr int CLEAR_CANDS = 3, CLEAR_TUNE_BLOCK = 3, CLEAR_TUNE_RENDERS = 2 * CLEAR_CANDS * CLEAR_TUNE_BLOCK;
constexpr uint32_t CLEAR_CAND[CLEAR_CANDS] = {96, 128, 256};
constexpr uint32_t CLEAR_GRID_MAX = 256, CLEAR_GRID_DEFAULT = 96;
struct ClearCtl {
  uint32_t wgs;                  // workgroups of the NEXT render's clear (0: CLEAR_CAND[0] — the state after a memset)
  uint32_t cur, pos, phase, done, alive;
  uint32_t n[CLEAR_CANDS];
  unsigned long long last;       // wall clock (100 MHz) at the end of the previous render
  float t[CLEAR_CANDS][4];       // samples, wall-clock ticks
  float score[CLEAR_CANDS];      // what the decision compared (ticks; 0: dropped after the first pass)
};
void launch_clear_tune(ClearCtl *ctl, uint32_t *h_wgs, hipStream_t s);
void launch_clear_rebase(ClearCtl *ctl, hipStream_t s); // (a render that files no sample: the next one times itself alone)

void launch_vertex(const DrawDesc *draws, uint32_t n_draws, uint32_t max_faces, srz_tri *tris, float *tri_pos, const FrameDesc *frames,
                   BBox *bbox_out, hipStream_t s);
// srz_frameset_positions: every frame's piece of the dense position stream (tri_pos / pos_stride as RenderArgs has them) into the
// caller's [frame][pos_tris][9], +0 behind a frame's last triangle (k_positions).  The host has checked pos_tris >= every frame's count
void launch_positions(const FrameDesc *frames, uint32_t n_frames, const float *tri_pos, uint32_t pos_stride, float *out, uint32_t pos_tris,
                      hipStream_t s);
// srz_sceneset_vertex_grad: the backward of k_vertex for ONE mesh slot (k_vertex_grad), from the gradient of the triangles' screen
// positions to the slot's vertices (gverts, a gather over each vertex's corner list: one owner per element) and to the matrix and
// depth mapping of each draw of the slot (gdraw, reduced per workgroup, then one float add per value).  A draw takes part when its
// DrawDesc names the slot's vertex buffer.  The host has checked pos_tris and draw_stride against every frame's counts
constexpr uint32_t VG_VALS = 18; // per draw: the 16 gradients of ndc_mvp in its own order, zscale, zoffset
struct VertexGradArgs {
  const FrameDesc *frames;     // n_batches / batch_off: the frame's draws in `draws`; tri_off: what a draw's tri_off is relative to
  const DrawDesc *draws;
  const srz_vertex *verts;     // the slot's vertices
  const uint32_t *corner_off;  // [n_verts + 1] into corners
  const uint32_t *corners;     // [3 * n_faces]: 3 * face + k of every corner that names the vertex, increasing
  const float *gpos;           // [frame][pos_tris][9]
  float *gverts;               // [frame][n_verts][3], added into (may be null)
  float *gdraw;                // [frame][draw_stride][18], added into (may be null)
  uint64_t gpos_stride;        // floats per frame in gpos = pos_tris * 9
  uint32_t n_verts, n_frames, draw_stride;
};
void launch_vertex_grad(const VertexGradArgs &a, hipStream_t s);
// srz_mesh_normals / srz_mesh_normals_grad: the area-weighted vertex normals of ONE mesh slot's faces over n_sets position sets
// (k_mesh_normals), and their backward (k_mesh_normals_grad, two launches: gS per vertex into `work`, then the gather over each
// vertex's corner list into gpos).  Vertex v of set s starts at float (s * n_verts + v) * stride of pos / nrm / gnrm; work and gpos are
// packed [n_sets][n_verts][3].  The host has checked the strides, the spans and n_sets <= 65535 (the grid's y)
struct MeshNormalsArgs {
  const float *pos;            // the slot's own records (stride 8) or the caller's sets
  const uint32_t *faces;       // [n_faces][3]
  const uint32_t *corner_off;  // [n_verts + 1] into corners
  const uint32_t *corners;     // [3 * n_faces]: 3 * face + k of every corner that names the vertex, increasing
  float *nrm;                  // forward: the output
  const float *gnrm;           // backward: the gradient of the normals
  float *work, *gpos;          // backward: gS (phase 1 writes, phase 2 reads), the output
  uint32_t pos_stride, nrm_stride, gnrm_stride;
  uint32_t n_verts, n_sets;
};
void launch_mesh_normals(const MeshNormalsArgs &a, hipStream_t s);
void launch_mesh_normals_grad(const MeshNormalsArgs &a, hipStream_t s);
// srz_mesh_tangents / srz_mesh_tangents_grad: the uv-area-weighted vertex tangents (x, y, z) and handedness w of ONE mesh slot's
// faces over n_sets position sets and ONE uv set (k_mesh_tangents), and their backward to the positions (k_mesh_tangents_grad, two
// launches as k_mesh_normals_grad).  Vertex v of set s starts at float (s * n_verts + v) * stride of pos / tan / gtan, uv of vertex v
// at float v * uv_stride; work and gpos are packed [n_sets][n_verts][3].  The host has checked the strides, the spans and n_sets
struct MeshTangentsArgs {
  const float *pos;            // the slot's own records (stride 8) or the caller's sets
  const float *uv;             // the slot's own records + 6 (stride 8) or the caller's one set
  const uint32_t *faces;       // [n_faces][3]
  const uint32_t *corner_off;  // [n_verts + 1] into corners
  const uint32_t *corners;     // [3 * n_faces]
  float *tan;                  // forward: the output, 4 floats a vertex
  const float *gtan;           // backward: the gradient of the tangents (its w is never read)
  float *work, *gpos;          // backward: gS (phase 1 writes, phase 2 reads), the output
  uint32_t pos_stride, uv_stride, tan_stride, gtan_stride;
  uint32_t n_verts, n_sets;
};
void launch_mesh_tangents(const MeshTangentsArgs &a, hipStream_t s);
void launch_mesh_tangents_grad(const MeshTangentsArgs &a, hipStream_t s);
// srz_mesh_laplacian / srz_mesh_laplacian_grad: the mesh Laplacian of ONE mesh slot's connectivity over n_sets per-vertex fields of
// n_ch channels (k_mesh_laplacian: a thread owns (set, vertex, chunk of channels) and walks the vertex's corner list).  Vertex v of
// set s starts at float (s * n_verts + v) * stride of x / out; wpos (COTAN only) is ONE position set, vertex v at float
// v * wpos_stride.  The backward is the same launch over gout: `transpose` picks UMBRELLA's transposed rule, the other two kinds are
// symmetric.  The host has checked the strides, the spans, n_ch 1 .. 64 and n_sets <= 65535 (the grid's y)
struct MeshLaplacianArgs {
  const float *x;              // the field (the backward: gout)
  const float *wpos;           // COTAN: the positions the weights are made from (the slot's own records or the caller's)
  const uint32_t *faces;       // [n_faces][3]
  const uint32_t *corner_off;  // [n_verts + 1] into corners
  const uint32_t *corners;     // [3 * n_faces]
  float *out;                  // the output (the backward: gx)
  uint32_t x_stride, wpos_stride, out_stride, n_ch;
  uint32_t n_verts, n_sets;
};
void launch_mesh_laplacian(const MeshLaplacianArgs &a, int kind, bool transpose, hipStream_t s);
// srz_mesh_edges / srz_mesh_edges_grad: the per-(face, edge) terms of ONE mesh slot over n_sets position sets (k_mesh_edges: a
// thread owns (set, face) and finds the faces across each edge in the shorter corner list of the edge's two ends) and their backward
// to the positions (k_mesh_edges_grad: LENGTH one launch over the vertices; DIHEDRAL two, gN per face into `work`, then the gather
// over each vertex's corner list).  Vertex v of set s starts at float (s * n_verts + v) * pos_stride; face f of set s at float
// (s * n_faces + f) * stride of out / gout; work is packed [n_sets][n_faces][3], gpos [n_sets][n_verts][3].  The host has checked
// the kind, the strides, the spans and n_sets <= 65535 (the grid's y)
struct MeshEdgesArgs {
  const float *pos;            // the slot's own records (stride 8) or the caller's sets
  const uint32_t *faces;       // [n_faces][3]
  const uint32_t *corner_off;  // [n_verts + 1] into corners
  const uint32_t *corners;     // [3 * n_faces]: 3 * face + k of every corner that names the vertex, increasing
  float *out;                  // forward: the output
  const float *gout;           // backward: the gradient of the output
  float *work, *gpos;          // backward: gN (DIHEDRAL's phase 1 writes, phase 2 reads), the output
  uint32_t pos_stride, out_stride, gout_stride;
  uint32_t n_verts, n_faces, n_sets;
};
void launch_mesh_edges(const MeshEdgesArgs &a, int kind, hipStream_t s);
void launch_mesh_edges_grad(const MeshEdgesArgs &a, int kind, hipStream_t s);
// srz_sceneset_corner_attr / _corner_attr_grad: per-vertex attributes of ONE mesh slot to the set's triangle stream
// [frame][pos_tris][3][n_ch], and the stream's gradient back to [frame][n_verts][n_ch] (k_corner_attr, k_corner_attr_grad: a thread
// owns (frame, vertex, channel) and walks the frame's draws of the slot and the vertex's corner list).  A draw takes part when its
// DrawDesc names the slot's vertex buffer.  The host has checked pos_tris against every frame's count
struct CornerAttrArgs {
  const FrameDesc *frames;
  const DrawDesc *draws;
  const srz_vertex *verts;     // the slot's vertices: what a draw of the slot names
  const uint32_t *corner_off, *corners;
  const float *attr;           // forward: [attr_frames][n_verts][n_ch]
  float *out;                  // forward: [frame][pos_tris][3][n_ch]
  const float *gout;           // backward: the same layout
  float *gattr;                // backward: [frame][n_verts][n_ch], every element written
  uint64_t attr_frame_stride;  // floats: 0 (one array for every frame) or n_verts * n_ch
  uint32_t n_verts, n_ch, pos_tris, n_frames;
};
void launch_corner_attr(const CornerAttrArgs &a, hipStream_t s);
void launch_corner_attr_grad(const CornerAttrArgs &a, hipStream_t s);
void launch_chunks(const RenderArgs &a, int n_frames, uint32_t max_tris, hipStream_t s);
void launch_setup(const RenderArgs &a, int n_frames, uint32_t max_tris, bool stats, hipStream_t s);
void launch_bin(const RenderArgs &a, int n_frames, uint32_t max_tris, hipStream_t s);
void launch_raster(const RenderArgs &a, int n_frames, bool stats, hipStream_t s);
// srz_frameset_peel_visibility: in place of launch_raster (k_peel; neither k_raster nor k_raster_slow runs).  prev: the previous layer,
// offset like a.out
void launch_peel(const RenderArgs &a, const float *prev, int n_frames, hipStream_t s);
bool raster_four_waves(const RenderArgs &a); // the latency build of k_raster serves this job (it also reports the pool's demand)
void launch_clear(const RenderArgs &a, uint32_t max_tiles, hipStream_t s, uint32_t wgs);
// kinds: bit k = some frame is shaded by FAST build kind k (frame_kind); approx: the tolerance mode's builds serve kinds 0..3
void launch_shade(const RenderArgs &a, uint32_t max_tiles, bool stats, uint32_t kinds, bool any_generic, bool approx, hipStream_t s);
// the visibility buffer (srz_frameset_render_visibility) in place of launch_shade: planes 1..3 of every owned tile
void launch_visibility(const RenderArgs &a, uint32_t max_tiles, hipStream_t s);
// srz_frameset_shade_visibility: the colour of a visibility buffer (k_shade_vis).  Everything a pixel's shading reads of the set, and the
// two buffers in the layout of srz_frameset_render; in_place: vis == out (only the owned pixels' colour planes are written)
struct ShadeVisArgs {
  const FrameDesc *frames;
  const srz_tri *tris;
  const uint16_t *tri_batch;
  const srz_light *lights;
  const ShadeDescG *sdesc;
  const float *vis;
  float *out;
  uint64_t frame_stride; // floats per frame in vis / out
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or, in_place;
  uint32_t any_generic;  // some frame is not FD_FAST_SHADE (else the generic build only serves redo_list)
  uint32_t *redo_list;   // tiles (frame * tiles per frame + tile) the FAST builds hand to the generic one
  uint32_t *redo_count;  // (zero at launch_shade_vis)
};
// one launch per build kind the set's frames need (kinds / any_generic / approx as for launch_shade); frames of other kinds are skipped
void launch_shade_vis(const ShadeVisArgs &a, uint32_t kinds, bool any_generic, bool approx, hipStream_t s);
// srz_frameset_gbuffer: the attribute planes of a visibility buffer (k_gbuffer).  vis in the layout of srz_frameset_render, out =
// [frame][planes of `what`][local_rows][width]; `out` / `frame_stride` / `local_rows` / the shard are what tile_rect reads
struct GbufArgs {
  const FrameDesc *frames;
  const srz_tri *tris;
  const uint16_t *tri_batch;
  const ShadeDescG *sdesc; // read only when `what` has SRZ_GB_ALBEDO
  const float *vis;
  float *out;
  uint64_t vis_stride;     // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride;   // floats per frame in out = planes * local_rows * width
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or, what;
};
__host__ __device__ constexpr uint32_t gbuf_planes(uint32_t what) {
  return ((what & SRZ_GB_NORMAL) ? 3u : 0u) + ((what & SRZ_GB_UV) ? 2u : 0u) + ((what & SRZ_GB_BATCH) ? 1u : 0u) + ((what & SRZ_GB_ALBEDO) ? 3u : 0u);
}
void launch_gbuffer(const GbufArgs &a, hipStream_t s);
// srz_frameset_motion: where the surface point under each pixel of frame f lies in frame f + delta (k_motion).  vis as above, out =
// [frame][planes of `what`][local_rows][width]; `out` / `frame_stride` / `local_rows` / the shard are what tile_rect reads.  The host
// has checked that every pair (f, f + delta) inside the set has one triangle count, and that TARGET comes with shard_world == 1
struct MotionArgs {
  const FrameDesc *frames;
  const float *tri_pos;    // [triangle * pos_stride], as RenderArgs has it
  uint32_t pos_stride;
  int32_t delta;           // (clamped to [-n_frames, n_frames] by the host: f + delta cannot overflow)
  const float *vis;
  float *out;
  uint64_t vis_stride;     // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride;   // floats per frame in out = planes * local_rows * width
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or, what;
};
__host__ __device__ constexpr uint32_t motion_planes(uint32_t what) {
  return ((what & SRZ_MV_FLOW) ? 2u : 0u) + ((what & SRZ_MV_DEPTH) ? 1u : 0u) + ((what & SRZ_MV_TARGET) ? 2u : 0u);
}
void launch_motion(const MotionArgs &a, hipStream_t s);
// srz_frameset_interpolate / _interpolate_grad: caller attributes [attr frame][triangle][corner][channel] under each pixel's
// barycentrics (k_interp), and the gradients of that with respect to the attributes and to alpha, beta (k_interp_grad).  vis as
// above; `out` is the forward's [frame][n_ch][local_rows][width] or the backward's gbary [frame][2][local_rows][width] (may be null
// there); `out` / `frame_stride` / `local_rows` / the shard are what tile_rect reads.  The host has checked attr_tris >= every
// frame's triangle count
struct InterpArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *attr;          // (backward: may be null when gbary is)
  float *out;
  const float *gout;          // backward: [frame][n_ch][local_rows][width]
  float *gattr;               // backward: attr's shape, added into (may be null)
  uint64_t vis_stride;        // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride;      // floats per frame in out
  uint64_t gout_stride;       // floats per frame in gout = n_ch * local_rows * width
  uint64_t attr_frame_stride; // floats per frame in attr / gattr = attr_tris * 3 * n_ch; 0: one array for every frame
  uint32_t n_ch;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_interp(const InterpArgs &a, hipStream_t s);
void launch_interp_grad(const InterpArgs &a, hipStream_t s);
// srz_frameset_position_grad: the gradients of a visibility buffer's alpha, beta and depth with respect to the owners' positions
// (gpos, added into) and to the pixel's sample point (gpix), from the planes k_interp_grad writes (gbary) and / or the gradient of
// plane 0 (gz) (k_pos_grad).  vis and tri_pos / pos_stride as above; `out` is gpix [frame][2][local_rows][width] (may be null);
// `out` / `frame_stride` / `local_rows` / the shard are what tile_rect reads.  The host has checked pos_tris >= every frame's
// triangle count
struct PosGradArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *tri_pos;  // [triangle * pos_stride], as RenderArgs has it
  const float *gbary;    // [frame][2][local_rows][width]: frame_stride floats per frame (may be null)
  const float *gz;       // [frame][1][local_rows][width] (may be null)
  float *gpos;           // [frame][pos_tris][9], added into (may be null)
  float *out;
  uint64_t vis_stride;   // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride; // floats per frame in out and gbary = 2 * local_rows * width
  uint64_t gz_stride;    // floats per frame in gz = local_rows * width
  uint64_t gpos_stride;  // floats per frame in gpos = pos_tris * 9
  uint32_t pos_stride;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_pos_grad(const PosGradArgs &a, hipStream_t s);
// srz_frameset_antialias / _antialias_grad: the caller's planes blended across the silhouettes of a visibility buffer (k_antialias),
// and the gradients of that with respect to the planes (gin) and to the nearer owners' positions (gpos, added into)
// (k_antialias_grad).  vis and tri_pos / pos_stride as above; `out` is the forward's blended planes or the backward's gin (may be
// null there), [frame][n_ch][local_rows][width] like `in` and `gout`; `out` / `frame_stride` / `local_rows` / the shard are what
// tile_rect reads.  The host has checked shard_world == 1 (a vertical pair may cross a band) and pos_tris >= every frame's count
struct AntialiasArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *tri_pos;  // [triangle * pos_stride], as RenderArgs has it
  const float *in;       // the planes the forward blends
  const float *gout;     // backward: the gradient of the blended planes (forward: null)
  float *gpos;           // backward: [frame][pos_tris][9], added into (may be null)
  float *out;
  uint64_t vis_stride;   // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride; // floats per frame in in / gout / out = n_ch * local_rows * width
  uint64_t gpos_stride;  // floats per frame in gpos = pos_tris * 9
  uint32_t pos_stride;
  uint32_t n_ch;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
};
void launch_antialias(const AntialiasArgs &a, hipStream_t s);
void launch_antialias_grad(const AntialiasArgs &a, hipStream_t s);
// srz_frameset_texture / _texture_grad: a float texture of the caller's [texture frame][row][column][channel] sampled bilinearly at
// the uv planes [frame][2][local_rows][width] under a visibility buffer (k_tex), and the gradients of that with respect to the
// texels (gtex, added into) and to u, v (k_tex_grad).  vis as above; `out` is the forward's [frame][n_ch][local_rows][width] or the
// backward's guv [frame][2][local_rows][width] (may be null there); `out` / `frame_stride` / `local_rows` / the shard are what
// tile_rect reads.  The host has checked 1 <= tex_w, tex_h <= SRZ_TEX_MAX_SIZE and the mode
struct TexArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *uv;
  const float *tex;          // (backward: may be null when guv is)
  float *out;
  const float *gout;         // backward: [frame][n_ch][local_rows][width]
  float *gtex;               // backward: tex's shape, added into (may be null)
  uint64_t vis_stride;       // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride;     // floats per frame in out
  uint64_t uv_stride;        // floats per frame in uv = 2 * local_rows * width
  uint64_t gout_stride;      // floats per frame in gout = n_ch * local_rows * width
  uint64_t tex_frame_stride; // floats per frame in tex / gtex = tex_h * tex_w * n_ch; 0: one texture for every frame
  uint32_t tex_w, tex_h, n_ch, mode;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_tex(const TexArgs &a, hipStream_t s);
void launch_tex_grad(const TexArgs &a, hipStream_t s);
// srz_frameset_texture_cube / _texture_cube_grad: a float cube map of the caller's [texture frame][face][row][column][channel], faces
// n x n, looked up seamlessly by the direction planes [frame][3][local_rows][width] under a visibility buffer (k_cube), and the
// gradients of that with respect to the texels (gtex, added into) and to the direction (k_cube_grad).  vis as above; `out` is the
// forward's [frame][n_ch][local_rows][width] or the backward's gdir [frame][3][local_rows][width] (may be null there).  The host
// has checked 1 <= n <= SRZ_TEX_MAX_SIZE: a texel's index (face * n + row) * n + column stays below 6 * 2^28
struct CubeArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *dir;
  const float *tex;          // (backward: may be null when gdir is)
  float *out;
  const float *gout;         // backward: [frame][n_ch][local_rows][width]
  float *gtex;               // backward: tex's shape, added into (may be null)
  uint64_t vis_stride;       // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride;     // floats per frame in out
  uint64_t dir_stride;       // floats per frame in dir = 3 * local_rows * width
  uint64_t gout_stride;      // floats per frame in gout = n_ch * local_rows * width
  uint64_t tex_frame_stride; // floats per frame in tex / gtex = 6 * n * n * n_ch; 0: one cube for every frame
  uint32_t n, n_ch;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_cube(const CubeArgs &a, hipStream_t s);
void launch_cube_grad(const CubeArgs &a, hipStream_t s);
// srz_frameset_light / _light_grad: Blinn-Phong under point lights for caller data.  nrm, pos, kd (may be null: ones), out, gout and
// the backward's gnrm, gpos, gkd (each may be null) are [frame][3][local_rows][width]; par is [par frames][SRZ_LIGHT_PAR(n_lights)]:
// eye[3] ka[3] ks[3], then per light pos[3] intensity[3].  `out` is the forward's output, null in the backward (which addresses its
// planes by frame_stride itself).  work: the backward's [frame][tile][K] partial sums of the parameter gradient, and behind them
// [frame][K] rows for the fold when every frame shares one parameter frame (null: the planes only)
struct LightArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *nrm, *pos, *kd;
  const float *par;
  float *out;
  const float *gout;
  float *gnrm, *gpos, *gkd;
  float *work;
  uint64_t vis_stride;   // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride; // floats per frame in every three-plane buffer = 3 * local_rows * width
  uint64_t par_stride;   // floats per frame in par = SRZ_LIGHT_PAR(n_lights); 0: one parameter frame for every frame
  uint32_t n_lights, p;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_light(const LightArgs &a, hipStream_t s);
void launch_light_grad(const LightArgs &a, float *gpar, hipStream_t s);
// srz_frameset_background / _background_grad: the environment behind a visibility buffer, looked up in a cube (CubeArgs' tex, gtex,
// n, n_ch, out, gout) by the pixel's view ray r0 + x rx + y ry from the ray block ray [ray frames][9]: r0[3] rx[3] ry[3].  where:
// SRZ_BG_NOBODY (the pixels nobody owns) or SRZ_BG_ALL (every pixel; vis may be null and is not read).  `out` is the forward's
// [frame][n_ch][local_rows][width], null in the backward.  work: the backward's [frame][tile][9] partial sums of the block's
// gradient, and behind them [frame][9] rows for the fold when every frame shares one block (null: gtex only)
struct BgArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *ray;
  const float *tex;          // (backward: may be null when gray is)
  float *out;
  const float *gout;         // backward: [frame][n_ch][local_rows][width]
  float *gtex;               // backward: tex's shape, added into (may be null)
  float *work;
  uint64_t vis_stride;       // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride;     // floats per frame in out
  uint64_t gout_stride;      // floats per frame in gout = n_ch * local_rows * width
  uint64_t tex_frame_stride; // floats per frame in tex / gtex = 6 * n * n * n_ch; 0: one cube for every frame
  uint64_t ray_stride;       // floats per frame in ray = 9; 0: one block for every frame
  uint32_t n, n_ch, where;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_background(const BgArgs &a, hipStream_t s);
void launch_background_grad(const BgArgs &a, float *gray, hipStream_t s);
// srz_frameset_microfacet / _microfacet_grad: Cook-Torrance (GGX, Schlick-Smith, Schlick Fresnel; metallic-roughness) under point
// lights for caller data.  nrm, pos, base (may be null: ones), out, gout and the backward's gnrm, gpos, gbase (each may be null) are
// [frame][3][local_rows][width]; mat and gmat (may be null) [frame][2][local_rows][width]: roughness, metallic; par is
// [par frames][SRZ_MICROFACET_PAR(n_lights)]: eye[3] amb[3], then per light pos[3] intensity[3].  `out` is the forward's output,
// null in the backward (which addresses its planes by frame_stride and mat_stride itself).  work: as LightArgs', K =
// SRZ_MICROFACET_PAR(n_lights)
struct MicrofacetArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *nrm, *pos, *base, *mat;
  const float *par;
  float *out;
  const float *gout;
  float *gnrm, *gpos, *gbase, *gmat;
  float *work;
  uint64_t vis_stride;   // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride; // floats per frame in every three-plane buffer = 3 * local_rows * width
  uint64_t mat_stride;   // floats per frame in mat / gmat = 2 * local_rows * width
  uint64_t par_stride;   // floats per frame in par = SRZ_MICROFACET_PAR(n_lights); 0: one parameter frame for every frame
  uint32_t n_lights;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_microfacet(const MicrofacetArgs &a, hipStream_t s);
void launch_microfacet_grad(const MicrofacetArgs &a, float *gpar, hipStream_t s);
// srz_frameset_reflect / _reflect_grad: the reflection of the view direction about the normal and the raw N.Vd.  nrm, pos and the
// backward's gnrm, gpos (each may be null) are [frame][3][local_rows][width]; eye is [eye frames][3]; `out` is the forward's
// [frame][4][local_rows][width] (R, then nv), null in the backward, whose gout has that shape
struct ReflectArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *nrm, *pos;
  const float *eye;
  float *out;
  const float *gout;
  float *gnrm, *gpos;
  uint64_t vis_stride;   // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride; // floats per frame in out / gout = 4 * local_rows * width
  uint64_t nrm_stride;   // floats per frame in every three-plane buffer = 3 * local_rows * width
  uint64_t eye_stride;   // 3; 0: one eye for every frame
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_reflect(const ReflectArgs &a, hipStream_t s);
void launch_reflect_grad(const ReflectArgs &a, hipStream_t s);
// srz_brdf_table: the split-sum table [n][n][2] of the microfacet pass's specular lobe, m rings of 2 m samples (k_brdf_table).  The
// host has checked 2 <= n <= SRZ_BRDF_TABLE_MAX and 1 <= m <= 256
void launch_brdf_table(float *tab, uint32_t n, uint32_t m, hipStream_t s);
// srz_frameset_ibl / _ibl_grad: the split-sum combine.  base (may be null: ones), irr, spec, out, gout and the backward's gbase, girr,
// gspec are [frame][3][local_rows][width]; mat and gmat [frame][2][..]: roughness, metallic; nv and gnv [frame][1][..]; tab and gtab
// (added into) [n][n][2], one for every frame.  Every backward output may be null.  `out` is the forward's output, null in the
// backward (which addresses its planes by the strides itself).  The host has checked 2 <= n <= SRZ_BRDF_TABLE_MAX
struct IblArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *base, *mat, *nv, *irr, *spec;
  const float *tab;
  float *out;
  const float *gout;
  float *gbase, *gmat, *gnv, *girr, *gspec;
  float *gtab;
  uint64_t vis_stride;   // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride; // floats per frame in every three-plane buffer = 3 * local_rows * width
  uint64_t mat_stride;   // floats per frame in mat / gmat = 2 * local_rows * width
  uint64_t nv_stride;    // floats per frame in nv / gnv = local_rows * width
  uint32_t n;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_ibl(const IblArgs &a, hipStream_t s);
void launch_ibl_grad(const IblArgs &a, hipStream_t s);
// srz_frameset_normal_map / _normal_map_grad: the shading normal of an interpolated normal nrm [frame][3][..], an interpolated tangent
// with handedness tan [frame][4][..] and a tangent-space normal m [frame][3][..] (k_normal_map), and the backward of that to all
// three (k_normal_map_grad: gnrm and gm three planes, gtan four with w written +0; each may be null).  `out` is the forward's output,
// null in the backward, which addresses its planes by frame_stride (three planes) and tan_stride (four) itself
struct NormalMapArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *nrm, *tan, *m;
  float *out;
  const float *gout;
  float *gnrm, *gtan, *gm;
  uint64_t vis_stride;   // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride; // floats per frame in every three-plane buffer = 3 * local_rows * width
  uint64_t tan_stride;   // floats per frame in tan / gtan = 4 * local_rows * width
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_normal_map(const NormalMapArgs &a, hipStream_t s);
void launch_normal_map_grad(const NormalMapArgs &a, hipStream_t s);
// srz_frameset_composite / _composite_grad: n_layers depth layers, nearest first, composited front to back per pixel.  Layer k is a
// visibility buffer lvis[k] [frame][4][..] (only its id plane is read), a colour buffer col[k] [frame][n_ch][..] and an alpha plane
// alpha[k] [frame][1][..] or, null, the scalar opacity[k]; bg [frame][n_ch][..] may be null.  `out` is the forward's
// [frame][n_ch + through][..] (plane n_ch: the transmittance), null in the backward, whose gout has the same planes and whose outputs
// gcol[k] (col's shape), galpha[k] (one plane) and gbg (bg's shape) may each be null.  `vis` is fill_walk's field (layer 0's buffer);
// the kernels read lvis.
struct CompositeArgs {
  const FrameDesc *frames;
  const float *vis;
  float *out;
  const float *lvis[SRZ_COMPOSITE_MAX], *col[SRZ_COMPOSITE_MAX], *alpha[SRZ_COMPOSITE_MAX];
  float opacity[SRZ_COMPOSITE_MAX];
  const float *bg;
  const float *gout;
  float *gcol[SRZ_COMPOSITE_MAX], *galpha[SRZ_COMPOSITE_MAX];
  float *gbg;
  uint64_t vis_stride;   // floats per frame in a visibility buffer = 4 * local_rows * width
  uint64_t frame_stride; // floats per frame in out / gout = (n_ch + through) * local_rows * width
  uint64_t col_stride;   // floats per frame in col / gcol / bg / gbg = n_ch * local_rows * width
  uint32_t n_layers, n_ch, through;
  uint32_t want_d;       // backward: some galpha is asked for (the colour planes are read)
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_composite(const CompositeArgs &a, hipStream_t s);
void launch_composite_grad(const CompositeArgs &a, hipStream_t s);
// srz_frameset_texture_set / _texture_set_grad: TexArgs with n_slots textures, the one of a pixel picked by its owner's batch
// (k_tex_set, k_tex_set_grad).  tri_batch: the set's batch of every triangle, as RenderArgs has it; batch_slot: the caller's
// n_batch_slot bytes, batch -> slot (a byte >= n_slots: the pixel is not sampled).  Per slot: tex (backward: may be null when guv
// is), gtex (backward: tex's shape, added into, may be null), tex_frame_stride (0: one texture for every frame), tex_w, tex_h; bit
// s of wrap_mask: slot s's mode is SRZ_TEX_WRAP.  vis, uv, out, gout and the strides as in TexArgs.  The host has checked every slot
// as srz_frameset_texture checks its texture, 1 <= n_slots <= SRZ_TEXSET_MAX and 1 <= n_batch_slot <= 65536
struct TexSetArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *uv;
  const uint16_t *tri_batch;
  const uint8_t *batch_slot;
  float *out;
  const float *gout;
  const float *tex[SRZ_TEXSET_MAX];
  float *gtex[SRZ_TEXSET_MAX];
  uint64_t tex_frame_stride[SRZ_TEXSET_MAX];
  uint32_t tex_w[SRZ_TEXSET_MAX], tex_h[SRZ_TEXSET_MAX];
  uint64_t vis_stride, frame_stride, uv_stride, gout_stride;
  uint32_t n_slots, n_batch_slot, n_ch, wrap_mask;
  uint32_t want_tex; // backward: some slot's gtex is asked for (the tile's table is kept)
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_tex_set(const TexSetArgs &a, hipStream_t s);
void launch_tex_set_grad(const TexSetArgs &a, hipStream_t s);
// srz_frameset_shadow / _shadow_grad: a float depth map of the caller's [map frame][row][column] compared and filtered at the
// coordinate planes sc [frame][3][local_rows][width] (sx, sy in texels, sd in the map's depth units) under a visibility buffer
// (k_shadow), and the gradients of that with respect to the map (gmap, added into) and to the coordinates (k_shadow_grad).  vis as
// above; `out` is the forward's [frame][1][local_rows][width] or the backward's gsc [frame][3][local_rows][width] (may be null
// there).  The host has checked 1 <= map_w, map_h <= SRZ_TEX_MAX_SIZE (a texel's index stays below 2^28), bias and width finite,
// width >= 0 (0: the hard test)
struct ShadowArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *sc;
  const float *map;
  float *out;
  const float *gout;         // backward: [frame][1][local_rows][width]
  float *gmap;               // backward: map's shape, added into (may be null)
  uint64_t vis_stride;       // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride;     // floats per frame in out
  uint64_t sc_stride;        // floats per frame in sc = 3 * local_rows * width
  uint64_t gout_stride;      // floats per frame in gout = local_rows * width
  uint64_t map_frame_stride; // floats per frame in map / gmap = map_h * map_w; 0: one map for every frame
  uint32_t map_w, map_h;
  float bias, width;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_shadow(const ShadowArgs &a, hipStream_t s);
void launch_shadow_grad(const ShadowArgs &a, hipStream_t s);
// THE MIP PYRAMID of a caller texture (include/srz.h states the geometry): level l of a tex_w x tex_h texture is
// max(1, tex_w >> l) x max(1, tex_h >> l) — every level that exists came from an even (or one-texel) extent, so the shifts are the
// halvings — and the levels 1 .. n_levels - 1 lie one after another, each [tex_frames][h_l][w_l][n_ch].  Host and device share these.
__host__ __device__ inline uint32_t mip_extent(uint32_t n, uint32_t l) { return (n >> l) > 1u ? n >> l : 1u; }
// the texels of one frame in the levels 1 .. l - 1 (below tex_w * tex_h <= 2^28)
__host__ __device__ inline uint32_t mip_texels_before(uint32_t tex_w, uint32_t tex_h, uint32_t l) {
  uint32_t s = 0;
  for (uint32_t k = 1; k < l; ++k) s += mip_extent(tex_w, k) * mip_extent(tex_h, k);
  return s;
}
// the build's factor into level l (>= 1): 0.25f where both extents of level l - 1 halve, 0.5f where one of them is already 1
__host__ __device__ inline float mip_factor(uint32_t tex_w, uint32_t tex_h, uint32_t l) {
  return mip_extent(tex_w, l - 1u) > 1u && mip_extent(tex_h, l - 1u) > 1u ? 0.25f : 0.5f;
}
// srz_texture_mip_build: one level from the level above it (k_mip_build, one launch per level); src [frames][src_h][src_w][n_ch],
// dst [frames][dst_h][dst_w][n_ch]
void launch_mip_build(const float *src, float *dst, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h, uint32_t n_ch,
                      uint32_t tex_frames, hipStream_t s);
// srz_texture_mip_fold: the gradient pyramid gmip (levels 1 .. n_levels - 1) folded into gtex (level 0), a gather (k_mip_fold)
void launch_mip_fold(const float *gmip, float *gtex, uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels,
                     hipStream_t s);
// srz_cube_prefilter / _prefilter_grad (include/srz.h states the rule): an ALL-PAIRS pass between an OWN cube — a lane owns one of
// its texels: the forward's output, the backward's source — and a WALKED cube, whose texels every lane visits in the same order.
// The three-level sum (row, face, cube) lets the walk be cut into `chunks` pieces without changing a bit: 1 (a lane walks the whole
// cube), 6 (a face) or 6 * n_walk (a row); every piece leaves its partial sums in the work buffer, k_prefilter_rows adds a face's rows
// in order and k_prefilter_fold the faces.  Host and device share the choice and the layout of the work buffer:
//   [table: 6 n_walk^2 x {d.x, d.y, d.z, jac}] [backward only: q = gdst / den, [frames][6 n_walk^2][n_ch]]
//   [partials: [chunk][frame][6 n_own^2][n_ch (+ 1 in the forward: den)]] [a walk cut into rows only: the six faces' partials]
constexpr uint32_t PREFILTER_CG = 4u;                 // channels a lane accumulates at a time
constexpr uint64_t PREFILTER_LANES = 1ull << 19;      // the lanes worth having in flight (8 waves per SIMD of 256 CUs)
constexpr uint64_t PREFILTER_ROW_FLOATS = 1ull << 23; // the partials a walk cut into rows may take (32 MiB)
inline uint64_t prefilter_texels(uint32_t n) { return 6ull * n * n; }
inline uint32_t prefilter_groups(uint32_t n_ch) { return (n_ch + PREFILTER_CG - 1u) / PREFILTER_CG; }
inline uint32_t prefilter_chunks(uint32_t n_own, uint32_t n_walk, uint32_t n_ch, uint32_t frames) {
  const uint64_t lanes = prefilter_texels(n_own) * frames * prefilter_groups(n_ch);
  if (lanes >= PREFILTER_LANES) return 1u;
  const uint64_t row_floats = 6ull * n_walk * prefilter_texels(n_own) * frames * (n_ch + 1u);
  return lanes * 6u >= PREFILTER_LANES || row_floats > PREFILTER_ROW_FLOATS ? 6u : 6u * n_walk;
}
inline size_t prefilter_align(size_t bytes) { return (bytes + 15u) & ~(size_t)15u; }
inline size_t prefilter_table_bytes(uint32_t n_walk) { return (size_t)prefilter_texels(n_walk) * 4u * sizeof(float); }
inline size_t prefilter_q_bytes(uint32_t n_dst, uint32_t n_ch, uint32_t frames) {
  return prefilter_align((size_t)prefilter_texels(n_dst) * frames * n_ch * sizeof(float));
}
inline size_t prefilter_part_bytes(uint32_t n_own, uint32_t n_walk, uint32_t n_ch, uint32_t frames, bool backward) {
  const uint32_t chunks = prefilter_chunks(n_own, n_walk, n_ch, frames);
  return (size_t)(chunks > 6u ? chunks + 6u : chunks) * frames * prefilter_texels(n_own) * (n_ch + (backward ? 0u : 1u)) * sizeof(float);
}
struct PrefilterArgs {
  const float *src;   // forward: the source cube; backward: gdst
  const float *den;   // backward: the forward's normaliser [6 n_dst^2]
  float *dst;         // forward: the output cube; backward: gsrc
  float *den_out;     // forward: the normaliser (may be null)
  void *work;         // the layout above
  uint32_t n_src, n_dst, n_ch, frames, kind;
  float roughness, cmin;
};
void launch_prefilter(const PrefilterArgs &a, hipStream_t s);
void launch_prefilter_grad(const PrefilterArgs &a, hipStream_t s);
// srz_cube_sh / _cube_sh_grad (include/srz.h states the rule): a cube projected to nine SH coefficients per channel, one wave per
// face row (k_cube_sh), the rows and then the faces added by k_light_fold, the division by k_cube_sh_finish; the backward a gather
// per source texel (k_cube_sh_grad) behind k_cube_sh_q.  K = 9 n_ch + 1 (the last slot: den) <= 64.  The work buffer, in floats:
//   forward:  [frame][face][row][K] row partials | [frame][face][K] face sums | [frame][K] cube sums
//   backward: [frame][9 n_ch] q = (FOURPI * gsh) / den
inline uint32_t cube_sh_slots(uint32_t n_ch) { return 9u * n_ch + 1u; }
inline size_t cube_sh_work_floats(uint32_t n, uint32_t n_ch, uint32_t frames) {
  return (size_t)frames * (6u * (size_t)n + 6u + 1u) * cube_sh_slots(n_ch);
}
struct CubeShArgs {
  const float *src;  // forward: the cube; backward: gsh [frame][9][n_ch]
  const float *den;  // backward: the forward's normaliser, one float
  float *dst;        // forward: sh [frame][9][n_ch]; backward: gsrc, the cube's shape
  float *den_out;    // forward: the normaliser (may be null)
  float *work;       // the layout above
  uint32_t n, n_ch, frames;
};
void launch_cube_sh(const CubeShArgs &a, hipStream_t s);
void launch_cube_sh_grad(const CubeShArgs &a, hipStream_t s);
// srz_frameset_sh / _sh_grad: SH9 coefficients sh [sh frames][9][n_ch] evaluated at the normal planes nrm [frame][3][..] (k_sh), and
// the backward of that to the normal (gnrm, three planes, may be null) and to the coefficients (k_sh_grad).  `out` is the forward's
// [frame][n_ch][..], null in the backward (which addresses its planes by the strides itself).  work: as LightArgs', K = 9 n_ch
struct ShArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *nrm;
  const float *sh;
  float *out;
  const float *gout;
  float *gnrm;
  float *work;
  uint64_t vis_stride;   // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride; // floats per frame in out / gout = n_ch * local_rows * width
  uint64_t nrm_stride;   // floats per frame in nrm / gnrm = 3 * local_rows * width
  uint64_t sh_stride;    // floats per frame in sh = 9 * n_ch; 0: one set of coefficients for every frame
  uint32_t n_ch, kind;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_sh(const ShArgs &a, hipStream_t s);
void launch_sh_grad(const ShArgs &a, float *gsh, hipStream_t s);
// srz_frameset_interpolate_deriv: the screen-space derivatives of caller attributes (k_interp_deriv).  vis, attr and the walk as
// InterpArgs has them, tri_pos / pos_stride as PosGradArgs; `out` is [frame][2 * n_ch][local_rows][width]
struct InterpDerivArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *tri_pos;       // [triangle * pos_stride], as RenderArgs has it
  const float *attr;
  float *out;
  uint64_t vis_stride;        // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride;      // floats per frame in out = 2 * n_ch * local_rows * width
  uint64_t attr_frame_stride; // floats per frame in attr = attr_tris * 3 * n_ch; 0: one array for every frame
  uint32_t pos_stride, n_ch;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_interp_deriv(const InterpDerivArgs &a, hipStream_t s);
// srz_frameset_perspective / _perspective_grad: a visibility buffer's alpha, beta rewritten into the perspective-correct alpha',
// beta' from the per-corner reciprocal clip w `q` [q frame][triangle][corner] (k_persp), and the backward of that rewrite, to the
// screen-linear alpha, beta and to q (k_persp_grad).  vis and the walk as InterpArgs has them; `out` is the forward's four-plane
// buffer [frame][4][local_rows][width] or the backward's gbary [frame][2][local_rows][width] (may be null there); `out` /
// `frame_stride` / `local_rows` / the shard are what tile_rect reads.  The host has checked q_tris >= every frame's triangle count
struct PerspArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *q;
  float *out;
  const float *gbary_p;    // backward: [frame][2][local_rows][width], the gradient with respect to alpha', beta'
  float *gq;               // backward: q's shape, added into (may be null)
  uint64_t vis_stride;     // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride;   // floats per frame in out (and in gbary_p: the backward's out has its shape)
  uint64_t q_frame_stride; // floats per frame in q / gq = q_tris * 3; 0: one array for every frame
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_persp(const PerspArgs &a, hipStream_t s);
void launch_persp_grad(const PerspArgs &a, hipStream_t s);
// srz_frameset_interpolate_deriv_persp: InterpDerivArgs' fields plus q as PerspArgs has it (k_interp_deriv_persp)
struct PerspDerivArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *tri_pos;       // [triangle * pos_stride], as RenderArgs has it
  const float *attr;
  const float *q;
  float *out;
  uint64_t vis_stride;        // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride;      // floats per frame in out = 2 * n_ch * local_rows * width
  uint64_t attr_frame_stride; // floats per frame in attr = attr_tris * 3 * n_ch; 0: one array for every frame
  uint64_t q_frame_stride;    // floats per frame in q = q_tris * 3; 0: one array for every frame
  uint32_t pos_stride, n_ch;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_interp_deriv_persp(const PerspDerivArgs &a, hipStream_t s);
// srz_frameset_texture_mip / _texture_mip_grad: TexArgs' fields, plus the derivative planes uvd [frame][4][local_rows][width], the
// pyramid `mip` (backward: may be null when guv is), its gradient `gmip` (added into, comes with gtex) and the level count
// (k_tex_mip, k_tex_mip_grad).  n_levels == 1: uvd, mip and gmip are not read.  The host has checked n_levels against the size
struct TexMipArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *uv;
  const float *uvd;
  const float *tex;
  const float *mip;
  float *out;
  const float *gout;
  float *gtex;
  float *gmip;
  uint64_t vis_stride;       // floats per frame in vis and uvd = 4 * local_rows * width
  uint64_t frame_stride;     // floats per frame in out
  uint64_t uv_stride;        // floats per frame in uv = 2 * local_rows * width
  uint64_t gout_stride;      // floats per frame in gout = n_ch * local_rows * width
  uint32_t tex_w, tex_h, n_ch, mode;
  uint32_t tex_frames, n_levels;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_tex_mip(const TexMipArgs &a, hipStream_t s);
void launch_tex_mip_grad(const TexMipArgs &a, hipStream_t s);
// srz_frameset_texture_cube_mip / _texture_cube_mip_grad / srz_frameset_cube_level: CubeArgs' fields, plus the cube's pyramid `mip`
// (levels 1 .. n_levels - 1, level l [tex_frames][6][n >> l][n >> l][n_ch]), its gradient `gmip` (added into, comes with gtex), the
// level plane `lam` [frame][1][local_rows][width] with its gradient `glam`, and for the level pass the derivative planes `dird`
// [frame][6][local_rows][width] (k_cube_mip, k_cube_mip_grad, k_cube_level).  `out` is the forward's [frame][n_ch][local_rows][width],
// the backward's gdir [frame][3][local_rows][width] (may be null there) or the level pass's lam plane.  n_levels == 1: lam, mip and
// gmip are not read.  The host has checked n_levels against n: every level l < n_levels has n >> l >= 1 texels a side, and a
// texel's offset in one frame's concatenated pyramid, 6 * (n^2 + (n >> 1)^2 + ...) + its index in the level, stays below 2^31
struct CubeMipArgs {
  const FrameDesc *frames;
  const float *vis;
  const float *dir;
  const float *dird;         // level pass only
  const float *lam;          // (null at n_levels == 1)
  const float *tex;          // (backward: may be null when only the texel gradients are asked for)
  const float *mip;
  float *out;
  const float *gout;         // backward: [frame][n_ch][local_rows][width]
  float *gtex;               // backward: tex's shape, added into (may be null)
  float *gmip;               // backward: mip's shape, added into (null with gtex, and at n_levels == 1)
  float *glam;               // backward: lam's shape (may be null)
  uint64_t vis_stride;       // floats per frame in vis = 4 * local_rows * width
  uint64_t frame_stride;     // floats per frame in out
  uint64_t dir_stride;       // floats per frame in dir = 3 * local_rows * width (dird: twice that)
  uint64_t gout_stride;      // floats per frame in gout = n_ch * local_rows * width
  uint64_t lam_stride;       // floats per frame in lam / glam = local_rows * width
  uint32_t n, n_ch;
  uint32_t tex_frames, n_levels;
  uint32_t local_rows, tiles_x, n_local_bands, n_frames;
  int32_t shard_rank, shard_world;
  uint32_t flags_or;
};
void launch_cube_mip(const CubeMipArgs &a, hipStream_t s);
void launch_cube_mip_grad(const CubeMipArgs &a, hipStream_t s);
void launch_cube_level(const CubeMipArgs &a, hipStream_t s);
void launch_resolve8(const float *planes, uint8_t *out, uint32_t n_frames, uint32_t rows, uint32_t W, uint64_t frame_stride,
                     hipStream_t s);
void launch_deinterleave(const void *gathered, void *full, uint32_t world, uint32_t n_fp, uint32_t bands_per_rank, uint32_t row_bytes,
                         hipStream_t s);
// ---- tile-sparse exchange (srz_frameset_sparse_*, message format: include/srz.h) -------------------------------------------------
constexpr uint32_t SPARSE_HEADER = 16;          // {touched tiles u32, table entries u32, message bytes u64}
constexpr uint32_t SPARSE_NONE = 0xffffffffu;   // table entry of a tile that is not in the payload (the clear values)
constexpr uint32_t SPARSE_UNPACK_WGS = 2048;    // k_sparse_unpack's grid
struct SparseArgs {
  const void *shard;            // pack: this rank's shard [frame][plane][local_rows][row bytes]
  uint8_t *msg;                 // pack: the message
  const uint2 *tile_info;       // pack: k_bin's [frame][n_local_bands][tiles_x] (.x = triangles whose bbox reaches the tile)
  const FrameDesc *frames;      // pack: FrameDesc::flags of the render the tile counts belong to
  uint32_t *row_cnt;            // pack: scratch, one word per (frame, local band): touched tiles, then their first slot
  uint32_t flags_or;            // pack: that render's flags
  uint32_t n_frames, n_local_bands, bands_per_rank, tiles_x;
  uint32_t width, height, local_rows, rank, world;
  uint32_t planes, row_bytes, px_bytes; // 4 float planes (16 B / px in total) or one 8-bit BGR plane (3 B / px)
  uint64_t payload_off;         // bytes in front of the payload (header + table, 16-byte aligned)
};
void launch_sparse_pack(const SparseArgs &a, hipStream_t s);
void launch_sparse_unpack(const SparseArgs &a, const void *recv, uint64_t msg_stride, void *gathered, hipStream_t s);
void launch_verify_fastmath(unsigned long long *d_out4, hipStream_t s);
void launch_verify_fastdiv(unsigned long long *d_out3, hipStream_t s);
void launch_verify_fastpow(unsigned long long *d_out3, float p, hipStream_t s);
void launch_verify_fastlen(unsigned long long *d_out4, hipStream_t s);
void launch_tex_convert(const uint8_t *d_bgr, int w, int h, int row_stride, uint32_t *d_bgrx, hipStream_t s);

} // namespace srz
