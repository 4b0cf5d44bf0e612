// srz_api.hip — the C ABI declared in include/srz.h (host side: contexts, framesets, uploads, launches).
// No CPU fallback exists: without a usable gfx950 device every compute entry point returns SRZ_E_NODEVICE.
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "srz_device.h"

using namespace srz;

namespace {
std::string g_create_error;

struct EventPair {
  hipEvent_t t0, t1, t2, t3; // t0..t1 setup+binning, t1..t2 raster (visibility + clear), t2..t3 shade
  bool detailed;             // t1 / t2 were recorded (every recorded event is a barrier in the launch stream: ≈4 µs each)
};

// host-side tables: a set's batches (resolve_shading turns them into the device's ShadeDescG) and a ctx's textures
struct BatchDesc {
  int32_t shader, tex_id;
  uint32_t first, count; // triangle range inside the frame
};
struct TexDesc {
  const uint32_t *bgrx; // one dword per texel: B | G<<8 | R<<16
  int32_t w, h;
};

// the flags of srz_frame / srz_scene_frame / a render that the device sees (FrameDesc::flags, RenderArgs::flags_or)
constexpr uint32_t FRAME_FLAGS = SRZ_UNIFIED | SRZ_FUSED_CLEAR | SRZ_ORDERED_RASTER;
constexpr uint32_t GB_GROUPS = SRZ_GB_NORMAL | SRZ_GB_UV | SRZ_GB_BATCH | SRZ_GB_ALBEDO;
constexpr uint32_t MV_GROUPS = SRZ_MV_FLOW | SRZ_MV_DEPTH | SRZ_MV_TARGET;
} // namespace

struct srz_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int shard_rank = 0, shard_world = 1;
  TexDesc h_tex[MAX_TEX];
  uint32_t *d_texmem[MAX_TEX];
  unsigned long long *d_stats = nullptr;
  struct MeshSlot {
    srz_vertex *d_verts = nullptr;
    uint32_t *d_faces = nullptr;
    // the corner lists of srz_sceneset_vertex_grad's gather, one block: corner_off [n_verts + 1], then corners [3 * n_faces] — vertex v is
    // named by the corners corners[corner_off[v] .. corner_off[v + 1]), each 3 * face + k, increasing
    uint32_t *d_corner_off = nullptr;
    uint32_t n_verts = 0, n_faces = 0;
    uint64_t upload = 0; // which srz_mesh_upload of this ctx filled the slot (1, 2, ...): a freed buffer's address can come back, this cannot
  } mesh[MAX_MESH];
  uint64_t mesh_uploads = 0;
  int timing = 0; // 0 off, 1 whole launch set only (2 events per render), 2 per-kernel groups as well (4 events)
  std::vector<EventPair> ev_pool, ev_used;
  double acc_ms[4] = {0, 0, 0, 0}; // bin, raster, shade, total
  uint64_t tex_version = 1;
  int acc_launches = 0;
  std::vector<float> acc_samples; // whole-launch-set time of every timed render since the last reset (bounded)
  // span of the timed renders since the last reset: first t0 → latest t3 (renders on several streams overlap; the span is
  // what their launch sets took together)
  hipEvent_t span_t0 = nullptr;
  bool span_open = false;
  double span_ms = 0.0;
  unsigned long long dbg[ST_COUNT] = {};
  // srz_draw / srz_draw_scene keep their frameset and device framebuffer between calls: a call whose structure (size,
  // batch sizes, shader types, light count) equals the previous one only re-uploads the data
  srz_frameset *draw_fs = nullptr;
  float *draw_out = nullptr;
  std::vector<uint64_t> draw_sig;
  // diagnostic switches, read ONCE when the ctx is created (never per render): frames per sub-batch of a large set (0: the
  // default, sub_batch_frames), 32-bit owner ids even where 16 would do
  int env_sub_batch = 0;
  bool env_no_packed = false; // SRZ_NO_PACKED (tests): see srz_frameset::no_packed
  uint32_t env_clear_wgs = 0; // SRZ_CLEAR_WGS: fixed grid of the side-stream clear (else measured per set, srz_frameset::ClearTune)
  // what sets of this ctx have measured, by shape (clear_memo): a new set of a known shape starts with that grid instead of measuring
  std::vector<std::pair<uint64_t, uint32_t>> clear_memo;
  bool opt_approx_shade = false; // SRZ_OPT_APPROX_SHADE (srz_set_option): framesets created from now on shade in the tolerance mode
  bool opt_pool_lazy = false; // SRZ_OPT_POOL_LAZY (srz_set_option; initial value: the environment variable SRZ_POOL_LAZY, read in srz_create)
  // streams beside the launch stream, each non-null only with all its events (create_side); events are used round-robin: a render never
  // re-records an event that a wait of the previous few renders may still refer to
  static constexpr int EV_RING = 8;
  hipStream_t stream2 = nullptr; // k_clear runs here, next to k_raster
  hipEvent_t ev_fork[EV_RING] = {}, ev_join[EV_RING] = {};
  float *batch_out = nullptr;    // srz_draw_batch's device planes, kept between calls (grown on demand)
  size_t batch_out_bytes = 0;
  hipStream_t stream3 = nullptr; // srz_draw_batch: the read-back of one piece of the batch under the render of the next
  hipEvent_t ev_piece[EV_RING] = {}; // "piece k has been rendered"
  unsigned ev_next = 0;
  // Renders submitted to DIFFERENT streams (LaneRenderer) take turns in the setup..raster phase: the next one's k_setup waits
  // for the previous one's k_raster.  Two k_rasters side by side slow each other (both LDS-bound) and then leave two k_shades
  // side by side (both VALU-bound); taking turns puts one stream's raster beside the other's shade, which is the overlap that
  // pays (MI355X, 2 x 128 frames of 1024^2: 1.13 → 1.09 ms per batch).  Renders on one stream are unaffected.
  hipEvent_t ev_raster[EV_RING] = {};
  unsigned raster_next = 0;
  hipStream_t raster_last_stream = nullptr;
  bool raster_valid = false;
};

struct srz_target {
  int width = 0, height = 0;
  float *d_planes = nullptr; // [z,c0,c1,c2][H][W]
  uint8_t *d_bgr8 = nullptr;
  bool pending_clear = false; // clear(Color|Depth) not yet materialised: the next draw runs with SRZ_FUSED_CLEAR
};

struct srz_frameset {
  int n_frames = 0, width = 0, height = 0;
  int shard_rank = 0, shard_world = 1;
  uint32_t n_bands = 0, n_local_bands = 0, bands_per_rank = 0, local_rows = 0;
  uint32_t max_tris = 0;
  uint64_t total_tris = 0, total_lights = 0;
  std::vector<FrameDesc> h_frames;
  std::vector<BatchDesc> h_batches;
  std::vector<ShadeDescG> h_sdesc;
  std::vector<srz_light> h_lights; // the host copy of the lights, indexed by FrameDesc::light_off (what classify_frames reads)
  FrameDesc *d_frames = nullptr;
  srz_tri *d_tris = nullptr;     // the triangle stream as uploaded
  float *d_tri_pos = nullptr;    // dense copy of its positions (9 floats per triangle); null: srz_draw's one-frame set, re-uploaded per call
  bool tris_aos = false;
  BBox *d_bbox = nullptr;
  uint16_t *d_tri_batch = nullptr;
  srz_light *d_lights = nullptr; // (d_frames / d_lights / d_draws point into d_dyn)
  // per-tile triangle lists: records in a pool of n_sub sub-pools (srz_device.h, RenderArgs); every render reports what
  // it asked of each sub-pool (h_pool_heads: mapped host memory the device stores into), and a render that finds the previous demand
  // above the capacity grows the pool first — so the memory is O(triangle-tile pairs), not O(bands x triangles)
  uint32_t *d_pool = nullptr; // tile lists: triangle indices
  uint32_t pool_sub_cap = 0, pool_n_sub = 1;
  bool pool_sized = false; // the first render has sized the pool by its own demand (render_impl)
  uint32_t *d_pool_heads = nullptr, *h_pool_heads = nullptr;
  static constexpr int DEMAND_PARTS = 8; // h_pool_heads holds one copy of the allocators' lines per sub-batch of a large render
  uint2 *d_tile_info = nullptr;
  // what the tile-sparse exchange needs of the LAST render (srz_frameset_sparse_pack): its flags (the touched test of a frame is
  // (FrameDesc::flags | these) & SRZ_FUSED_CLEAR, as in k_clear) and a word per (frame, local band) of scratch for the slot scan
  uint32_t last_flags = 0;
  bool rendered = false;
  uint32_t *d_sparse_rows = nullptr;
  uint32_t *d_slow_list = nullptr, *d_slow_count = nullptr;
  uint4 *d_redo_list = nullptr; // (its counter is d_slow_count[1])
  uint32_t fast_kinds = 0;  // bit k: some frame is shaded by the FAST build of kind k (srz_device.h, frame_kind; classify_frames)
  bool any_generic = true;  // some frame needs the generic build
  uint32_t *d_vis = nullptr, *d_work_count = nullptr, *d_chunk_rows = nullptr; // d_vis: the per-tile pixel lists (srz_device.h)
  uint4 *d_worklist = nullptr;
  // k_shade's work lists are stored only for the build kinds some frame of the set needs (+ the generic one): slot of kind k =
  // (kind_slots >> 4k) & 15 (RenderArgs::kind_slots); a re-classification that brings a new kind in grows the storage
  uint64_t kind_slots = 0;
  uint32_t kind_mask = 0, n_kind_slots = 0;
  bool approx_shade = false; // SRZ_OPT_APPROX_SHADE at creation: frames of 1..4 lights without BUMP / DISPLACEMENT batches are shaded by the ApproxMath builds
  bool no_packed = false; // SRZ_NO_PACKED (tests): no frame is FD_PACKED — 32-bit owner ids by triangle index, no staged triangles
  uint32_t *d_band_desc = nullptr; // the band sort of k_setup / k_chunks (srz_device.h, GROUP_TRIS): descriptors [group][local band]
  uint2 *d_band_ent = nullptr;     // and entries [group][ENT_PER_GROUP]
  uint64_t total_groups = 0;
  ShadeDescG *d_sdesc = nullptr;
  DrawDesc *d_draws = nullptr; // device vertex stage (srz_sceneset_create), else null
  // every set keeps what an update rewrites in ONE device block [FrameDesc x n | lights | DrawDesc x draws] that is refreshed by a
  // single asynchronous copy from a small ring of pinned staging buffers (upload_dyn; no stream sync per update), made at the first update
  static constexpr int STAGE_RING = 4;
  uint8_t *d_dyn = nullptr;
  size_t dyn_bytes = 0, dyn_lights_off = 0, dyn_draws_off = 0;
  uint8_t *h_stage[STAGE_RING] = {};
  hipEvent_t stage_ev[STAGE_RING] = {};
  bool stage_busy[STAGE_RING] = {};
  unsigned stage_next = 0;
  std::vector<DrawDesc> h_draws;
  std::vector<int> h_draw_mesh;
  std::vector<uint64_t> h_draw_upload; // the upload each draw's buffers came from (srz_ctx::MeshSlot::upload)
  uint32_t n_draws = 0, max_faces = 0;
  uint64_t sdesc_version = 0;
  uint32_t tiles_x = 0, max_tiles = 0;
  bool have_stats = false;
  bool update_failed = false; // an update re-classified the frames but could not get the work lists they need: renders are refused
  // Grid of the side-stream clear (launch_clear).  Its best size depends on what the clear runs beside — about 96 workgroups on configs 2
  // and 3, 256 on config 4, 160 on config 5, with 4 .. 8 % of a step between the best and the worst of them — so a set MEASURES it, on
  // the device (srz_device.h, ClearCtl / k_clear_tune): from render CLEAR_TUNE_SKIP on the clear is launched with CLEAR_GRID_MAX workgroups
  // of which the device-side state says how many take part, and a one-thread kernel ends each of the next <= 18 renders; the decision
  // arrives in a word of mapped host memory, and from the render that finds it there the host launches exactly that grid.  The pixels are
  // the same bits under every grid.  SRZ_CLEAR_WGS fixes the grid.  Every CLEAR_TUNE_AGAIN renders the set measures again (the scene of a sceneset changes under it).  A new set whose shape
  // another set of the ctx has measured (srz_ctx::clear_memo) starts with that set's grid and measures only then.
  static constexpr int CLEAR_TUNE_SKIP = 6, CLEAR_TUNE_AGAIN = 4096;
  struct ClearTune {
    uint32_t wgs = CLEAR_GRID_DEFAULT; // the grid in use outside the measurement
    bool done = false;  // the host has seen the decision of the current measurement
    int renders = 0;    // renders of the set enqueued so far (counted until the measurement's last render)
    int since = 0;      // renders since the last decision
    ClearCtl *d_ctl = nullptr;  // device-side state
    uint32_t *h_wgs = nullptr;  // mapped host memory: 0 until k_clear_tune has decided
  } clear_tune;
  srz_stats stats{};
};

namespace {

// `stream` arguments of the C ABI: NULL = the ctx's own (non-blocking) stream, SRZ_STREAM_NULL = HIP's null stream, else a
// hipStream_t
hipStream_t pick_stream(const srz_ctx *ctx, void *stream) {
  if (!stream) return ctx->stream;
  return stream == SRZ_STREAM_NULL ? (hipStream_t) nullptr : (hipStream_t)stream;
}

int fail(srz_ctx *ctx, int code, const std::string &msg) {
  if (ctx)
    ctx->err = msg;
  else
    g_create_error = msg;
  return code;
}

#define HIP_TRY(ctx, expr)                                                                                             \
  do {                                                                                                                 \
    hipError_t e_ = (expr);                                                                                            \
    if (e_ != hipSuccess)                                                                                              \
      return fail(ctx, e_ == hipErrorOutOfMemory ? SRZ_E_NOMEM : SRZ_E_NODEVICE,                                      \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                                                  \
  } while (0)

void shard_layout(int height, int rank, int world, uint32_t &n_bands, uint32_t &n_local, uint32_t &per_rank,
                  uint32_t &local_rows) {
  n_bands = (uint32_t)((height + BAND - 1) / BAND);
  // (one band of every full group of `world` bands, and of the last, partial group if the rotation puts this rank inside it: band_of)
  n_local = n_bands / (uint32_t)world;
  if ((uint32_t)band_of((int)n_local, rank, world) < n_bands) ++n_local;
  per_rank = (n_bands + (uint32_t)world - 1) / (uint32_t)world;
  local_rows = world == 1 ? (uint32_t)height : per_rank * BAND;
}

// Which frames the FAST builds of k_shade can shade: 1..4 lights (Shader::p is 150 as the reference ships it, src/Shader.cpp:10;
// any light count and exponent are legal there, src/Shader.cpp:192-386) — every shader type qualifies.  An integer exponent
// 0 <= p <= 256 takes the builds with the exact multiplication chains, a non-integer exponent in (0, 4096] the builds whose power
// is pow_fast (FD_GENPOW; not combined with BUMP / DISPLACEMENT batches), every other exponent the generic build.  Sets FD_FAST_SHADE + the
// light count in the host copies of the descriptors.
// (the lights: the set's host copy, fs->h_lights)
void classify_frames(srz_frameset *fs) {
  fs->fast_kinds = 0, fs->any_generic = false;
  for (FrameDesc &d : fs->h_frames) {
    // FD_GREY: three bit-equal channels in ka, ks and every light's intensity (the shaders then compute a PHONG pixel's channel once)
    bool grey = std::memcmp(&d.ka[0], &d.ka[1], 4) == 0 && std::memcmp(&d.ka[1], &d.ka[2], 4) == 0 &&
                std::memcmp(&d.ks[0], &d.ks[1], 4) == 0 && std::memcmp(&d.ks[1], &d.ks[2], 4) == 0;
    for (uint32_t l = 0; grey && l < d.n_lights; ++l) {
      const srz_light &L = fs->h_lights[d.light_off + l];
      grey = std::memcmp(&L.intensity[0], &L.intensity[1], 4) == 0 && std::memcmp(&L.intensity[1], &L.intensity[2], 4) == 0;
    }
    const bool intpow = d.p >= 0.0f && d.p <= 256.0f && d.p == std::trunc(d.p);
    bool bumpy = false;
    for (uint32_t b = 0; b < d.n_batches; ++b) {
      const int sh = fs->h_batches[d.batch_off + b].shader;
      bumpy = bumpy || sh == SRZ_SHADER_BUMP || sh == SRZ_SHADER_DISPLACEMENT;
    }
    const bool fracpow = d.p > 0.0f && d.p <= 4096.0f && d.p != std::trunc(d.p); // (pow_fast's domain)
    // the tolerance mode (SRZ_OPT_APPROX_SHADE): its builds take any finite exponent >= 0 (exp2(p log2 x)) through the plain kinds'
    // work lists; frames they do not cover keep the exact generic build
    const bool approx = fs->approx_shade && d.n_lights >= 1u && d.n_lights <= 4u && !bumpy && d.p >= 0.0f && std::isfinite(d.p);
    const bool fast = approx || (!fs->approx_shade && d.n_lights >= 1u && d.n_lights <= 4u && (intpow || (fracpow && !bumpy)));
    const bool plain = approx || intpow;
    d.flags = (d.flags & ~(FD_FAST_SHADE | FD_BUMPY | FD_GENPOW | FD_PACKED | FD_GREY | (7u << FD_NL_SHIFT))) | (grey ? FD_GREY : 0u) |
              (fast ? (FD_FAST_SHADE | (d.n_lights << FD_NL_SHIFT) | (bumpy ? FD_BUMPY : 0u) | (plain ? 0u : FD_GENPOW)) : 0u) |
              ((d.n_tris < PACK_IDX_MASK && d.n_batches <= PACK_MAX_BATCHES && !fs->no_packed) ? FD_PACKED : 0u);
    if (fast)
      fs->fast_kinds |= 1u << frame_kind(d.flags);
    else
      fs->any_generic = true;
  }
}

// (re)allocates the work-list storage when the set needs a kind that has no slot yet; hipSuccess when nothing had to change.  The
// generic kind always has one (counting runs and the FAST builds' redo tiles go there)
hipError_t ensure_worklists(srz_frameset *fs) {
  const uint32_t need = fs->fast_kinds | 1u << SHADE_KIND_GENERIC | fs->kind_mask;
  if (need == fs->kind_mask && fs->d_worklist) return hipSuccess;
  uint64_t slots = 0;
  uint32_t n = 0;
  for (uint32_t k = 0; k <= SHADE_KIND_GENERIC; ++k)
    if (need & (1u << k)) slots |= (uint64_t)(n++) << (4u * k);
  const size_t cap = (size_t)(fs->n_frames < 8 ? fs->n_frames : (fs->n_frames + 7) / 8) * fs->n_local_bands * fs->tiles_x;
  // the new storage first, the swap only on success: a failed allocation leaves the set exactly as it was (old lists, old slots) —
  // callers that had already re-classified the frames for a kind without a slot roll that back (srz_sceneset_update, srz_draw)
  uint4 *nw = nullptr;
  const hipError_t e = hipMalloc((void **)&nw, std::max<size_t>(sizeof(uint4) * 8u * n * cap, 256));
  if (e != hipSuccess) return e;
  if (fs->d_worklist) { // renders in flight may still be walking the old lists
    (void)hipDeviceSynchronize();
    (void)hipFree(fs->d_worklist);
  }
  fs->d_worklist = nw, fs->kind_mask = need, fs->kind_slots = slots, fs->n_kind_slots = n;
  return hipSuccess;
}

void free_frameset_buffers(srz_frameset *fs) {
  for (int i = 0; i < srz_frameset::STAGE_RING; ++i) {
    if (fs->h_stage[i]) (void)hipHostFree(fs->h_stage[i]);
    if (fs->stage_ev[i]) (void)hipEventDestroy(fs->stage_ev[i]);
  }
  (void)hipFree(fs->d_dyn); // (d_frames / d_lights / d_draws)
  (void)hipFree(fs->d_tris);
  (void)hipFree(fs->d_tri_pos);
  (void)hipFree(fs->d_bbox);
  (void)hipFree(fs->d_tri_batch);
  (void)hipFree(fs->d_pool);
  (void)hipFree(fs->d_pool_heads);
  if (fs->h_pool_heads) (void)hipHostFree(fs->h_pool_heads);
  if (fs->clear_tune.h_wgs) (void)hipHostFree(fs->clear_tune.h_wgs), fs->clear_tune.h_wgs = nullptr;
  if (fs->clear_tune.d_ctl) (void)hipFree(fs->clear_tune.d_ctl), fs->clear_tune.d_ctl = nullptr;
  (void)hipFree(fs->d_tile_info);
  (void)hipFree(fs->d_sparse_rows);
  (void)hipFree(fs->d_slow_list);
  (void)hipFree(fs->d_slow_count);
  (void)hipFree(fs->d_redo_list);
  (void)hipFree(fs->d_vis);
  (void)hipFree(fs->d_worklist);
  (void)hipFree(fs->d_work_count);
  (void)hipFree(fs->d_chunk_rows);
  (void)hipFree(fs->d_band_desc);
  (void)hipFree(fs->d_band_ent);
  (void)hipFree(fs->d_sdesc);
}

// What a render asks for.  VISIBILITY: k_visibility writes the visibility buffer where k_shade would write colour (no texture needed; no
// sample of the clear's grid measurement).  COUNTING: the counters of srz_stats (the reference's ordered walk).  SIZE_ONLY: the creation-
// time pass of srz_frameset_create / srz_sceneset_create — setup + binning of every sub-batch, which size the tile-list pool, nothing else.
// PEEL (srz_frameset_peel_visibility): a VISIBILITY render whose rasteriser is k_peel — the layer behind d_prev instead of the nearest one.
struct Pass {
  enum Kind { COLOUR, VISIBILITY, COUNTING, SIZE_ONLY, PEEL } kind = COLOUR;
  int f_begin = 0, f_count = -1; // only frames [f_begin, f_begin + f_count) of the set (-1: all); d_out is the whole set's buffer either way
  bool one_frame_scratch = false; // a counting run whose pixels nobody reads: every frame writes the SAME one-frame buffer
  const float *d_prev = nullptr;  // PEEL: the previous layer, laid out like d_out
  static Pass colour() { return {}; }
  static Pass colour_frames(int f_begin, int f_count) { return {COLOUR, f_begin, f_count}; }
  static Pass visibility() { return {VISIBILITY}; }
  static Pass counting() { return {COUNTING}; }
  static Pass counting_into_one_frame() { return {COUNTING, 0, -1, true}; }
  static Pass size_only() { return {SIZE_ONLY}; }
  static Pass peel(const float *d_prev) { return {PEEL, 0, -1, false, d_prev}; }
  bool writes_visibility() const { return kind == VISIBILITY || kind == PEEL; } // (k_visibility behind the rasteriser, no clear-grid sample)
};

// the render's flags or some frame's have `bit`
bool any_frame_has(const srz_frameset *fs, uint32_t flags_or, uint32_t bit) {
  return (flags_or & bit) != 0 || std::any_of(fs->h_frames.begin(), fs->h_frames.end(), [bit](const FrameDesc &f) { return (f.flags & bit) != 0; });
}

// the set's positions, for RenderArgs and every pass's Args that reads them: the dense stream of a sceneset, else the triangles themselves
template <class Args> void fill_positions(Args &a, const srz_frameset *fs) {
  a.tri_pos = fs->d_tri_pos ? fs->d_tri_pos : reinterpret_cast<const float *>(fs->d_tris);
  a.pos_stride = fs->d_tri_pos ? TRI_POS_F : TRI_AOS_F;
}

RenderArgs make_args(const srz_ctx *ctx, const srz_frameset *fs, float *d_out, uint32_t flags_or, const Pass &pass) {
  RenderArgs a{};
  a.frames = fs->d_frames;
  a.tris = fs->d_tris;
  fill_positions(a, fs);
  a.bbox = fs->d_bbox;
  a.chunk_rows = fs->d_chunk_rows;
  a.band_desc = fs->d_band_desc;
  a.band_ent = fs->d_band_ent;
  a.tri_batch = fs->d_tri_batch;
  a.lights = fs->d_lights;
  a.pool = fs->d_pool;
  a.pool_heads = fs->d_pool_heads;
  a.pool_demand = fs->h_pool_heads; // (hipHostMallocMapped: the same address on the device)
  a.pool_sub_cap = fs->pool_sub_cap;
  a.pool_sub_mask = fs->pool_n_sub - 1u;
  a.tile_info = fs->d_tile_info;
  a.slow_list = fs->d_slow_list;
  a.slow_count = fs->d_slow_count;
  a.redo_list = fs->d_redo_list;
  a.redo_count = fs->d_slow_count + 1;
  a.force_ordered = a.force_generic = pass.kind == Pass::COUNTING ? 1u : 0u; // (counting: the counters are those of the reference's ordered walk)
  a.any_ordered = any_frame_has(fs, flags_or, SRZ_ORDERED_RASTER) ? 1u : 0u, a.any_generic = fs->any_generic ? 1u : 0u;
  a.sdesc = fs->d_sdesc;
  a.vis = fs->d_vis;
  a.worklist = fs->d_worklist;
  a.kind_slots = fs->kind_slots;
  a.work_count = fs->d_work_count;
  // (a list holds the tiles of every 8th frame; of fewer than 8 frames: any of them)
  a.work_cap = (uint32_t)(fs->n_frames < 8 ? fs->n_frames : (fs->n_frames + 7) / 8) * fs->n_local_bands * fs->tiles_x;
  a.tiles_x = fs->tiles_x;
  a.n_local_bands = fs->n_local_bands;
  a.n_frames = (uint32_t)fs->n_frames;
  a.out = d_out;
  a.local_rows = fs->local_rows;
  a.frame_stride = pass.one_frame_scratch ? 0 : 4ull * fs->local_rows * (uint64_t)fs->width;
  a.shard_rank = fs->shard_rank;
  a.shard_world = fs->shard_world;
  a.flags_or = flags_or;
  a.stats = ctx->d_stats;
  return a;
}

// a timed render's events (from the pool, else new ones), t0 recorded on `s`
int begin_timing(srz_ctx *ctx, EventPair &ep, bool detailed, hipStream_t s) {
  if (ctx->ev_pool.empty())
    for (hipEvent_t *e : {&ep.t0, &ep.t1, &ep.t2, &ep.t3}) HIP_TRY(ctx, hipEventCreate(e));
  else
    ep = ctx->ev_pool.back(), ctx->ev_pool.pop_back();
  ep.detailed = detailed;
  HIP_TRY(ctx, hipEventRecord(ep.t0, s));
  return SRZ_OK;
}

int collect_events(srz_ctx *ctx) {
  for (auto &ep : ctx->ev_used) {
    HIP_TRY(ctx, hipEventSynchronize(ep.t3));
    float b = 0.f, r = 0.f, sh = 0.f, t = 0.f;
    if (ep.detailed) {
      HIP_TRY(ctx, hipEventElapsedTime(&b, ep.t0, ep.t1));
      HIP_TRY(ctx, hipEventElapsedTime(&r, ep.t1, ep.t2));
      HIP_TRY(ctx, hipEventElapsedTime(&sh, ep.t2, ep.t3));
    }
    HIP_TRY(ctx, hipEventElapsedTime(&t, ep.t0, ep.t3));
    ctx->acc_ms[0] += b, ctx->acc_ms[1] += r, ctx->acc_ms[2] += sh, ctx->acc_ms[3] += t;
    ctx->acc_launches++;
    if (ctx->acc_samples.size() < 65536) ctx->acc_samples.push_back(t);
    if (!ctx->span_open) { // keep the first render's start: swap it for the context's spare event
      if (!ctx->span_t0) HIP_TRY(ctx, hipEventCreate(&ctx->span_t0));
      std::swap(ctx->span_t0, ep.t0);
      ctx->span_open = true;
    }
    float sp = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&sp, ctx->span_t0, ep.t3));
    ctx->span_ms = std::max(ctx->span_ms, (double)sp);
    ctx->ev_pool.push_back(ep);
  }
  ctx->ev_used.clear();
  return SRZ_OK;
}

// A side stream (null: none) and its rings of EV_RING events (null: none): destroyed once the stream has drained, or created all or
// nothing — into locals, published only when every call has succeeded.
void destroy_side(hipStream_t stream, hipEvent_t *ring_a, hipEvent_t *ring_b = nullptr) {
  if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
  for (hipEvent_t *ring : {ring_a, ring_b})
    for (int i = 0; ring && i < srz_ctx::EV_RING; ++i)
      if (ring[i]) (void)hipEventDestroy(ring[i]);
}
int create_side(srz_ctx *ctx, const char *what, hipStream_t *stream, bool high_priority, hipEvent_t *ring_a, hipEvent_t *ring_b = nullptr) {
  hipStream_t st = nullptr;
  hipEvent_t ev[2][srz_ctx::EV_RING] = {};
  int prio_least = 0, prio_greatest = 0;
  hipError_t e = high_priority ? hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) : hipSuccess;
  if (e == hipSuccess && stream)
    e = high_priority ? hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio_greatest) : hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  for (int i = 0; i < 2 * srz_ctx::EV_RING && e == hipSuccess; ++i)
    if (i < srz_ctx::EV_RING ? ring_a : ring_b) e = hipEventCreateWithFlags(&ev[i / srz_ctx::EV_RING][i % srz_ctx::EV_RING], hipEventDisableTiming);
  if (e != hipSuccess) {
    destroy_side(st, ev[0], ev[1]);
    return fail(ctx, e == hipErrorOutOfMemory ? SRZ_E_NOMEM : SRZ_E_NODEVICE, std::string(what) + ": " + hipGetErrorString(e));
  }
  if (stream) *stream = st;
  if (ring_a) std::copy(ev[0], ev[0] + srz_ctx::EV_RING, ring_a);
  if (ring_b) std::copy(ev[1], ev[1] + srz_ctx::EV_RING, ring_b);
  return SRZ_OK;
}

// batch → shader / texture, (re)resolved when a texture upload has changed them; SRZ_E_TEXTURE if a batch's slot was never uploaded
int resolve_shading(srz_ctx *ctx, srz_frameset *fs, hipStream_t s) {
  auto needs_tex = [](const BatchDesc &b) { return b.shader == SRZ_SHADER_TEXTURE || b.shader == SRZ_SHADER_DISPLACEMENT || b.shader == SRZ_SHADER_BUMP; };
  for (const BatchDesc &b : fs->h_batches)
    if (needs_tex(b) && (b.tex_id < 0 || b.tex_id >= MAX_TEX || !ctx->h_tex[b.tex_id].bgrx))
      return fail(ctx, SRZ_E_TEXTURE, "batch uses texture slot " + std::to_string(b.tex_id) + " which was never uploaded");
  if (fs->sdesc_version == ctx->tex_version || fs->h_batches.empty()) return SRZ_OK;
  std::vector<ShadeDescG> &h = fs->h_sdesc; // (owned by the set: the asynchronous copy below may read it after we return)
  h.resize(fs->h_batches.size());
  for (size_t i = 0; i < h.size(); ++i) {
    const BatchDesc &b = fs->h_batches[i];
    const TexDesc t = needs_tex(b) ? ctx->h_tex[b.tex_id] : TexDesc{nullptr, 1, 1};
    h[i] = ShadeDescG{b.shader, t.w, t.h, 0, t.bgrx};
  }
  // on the launch stream: ordered after the renders already submitted there, before this one
  HIP_TRY(ctx, hipMemcpyAsync(fs->d_sdesc, h.data(), sizeof(ShadeDescG) * h.size(), hipMemcpyHostToDevice, s));
  fs->sdesc_version = ctx->tex_version;
  return SRZ_OK;
}

// h_pool_heads holds one copy of the allocators' lines (word 0 of each: a sub-pool's demand) per sub-batch of a render: sub-batch `part`'s
// region; the largest demand of the regions of sub-batches [p0, p1); the copy of sub-batch `part`'s demand to the host, on `cs` (no event:
// the next render reads whatever has arrived)
uint32_t *demand_region(const srz_frameset *fs, int part) {
  return fs->h_pool_heads + (size_t)std::min(part, srz_frameset::DEMAND_PARTS - 1) * CNT_STRIDE * 64;
}
uint32_t max_pool_demand(const srz_frameset *fs, int p0, int p1) {
  uint32_t need = 0;
  for (int p = p0; p < p1; ++p)
    for (uint32_t i = 0; i < fs->pool_n_sub; ++i) need = std::max(need, (uint32_t) static_cast<const volatile uint32_t *>(demand_region(fs, p))[i * CNT_STRIDE]);
  return need;
}
hipError_t copy_demand(const srz_frameset *fs, int part, hipStream_t cs) {
  return hipMemcpyAsync(demand_region(fs, part), fs->d_pool_heads, sizeof(uint32_t) * CNT_STRIDE * fs->pool_n_sub, hipMemcpyDeviceToHost, cs);
}
// a new record pool of need + need / slack + 64 records per sub-pool, after the device has stopped reading the old one
int grow_pool(srz_ctx *ctx, srz_frameset *fs, uint32_t need, uint32_t slack) {
  HIP_TRY(ctx, hipDeviceSynchronize());
  const uint64_t cap = (uint64_t)need + need / slack + 64u;
  if (cap * fs->pool_n_sub >= 0xffffffffull) return fail(ctx, SRZ_E_NOMEM, "tile lists exceed 2^32 records; split the batch");
  uint32_t *p = nullptr;
  HIP_TRY(ctx, hipMalloc(&p, sizeof(uint32_t) * cap * fs->pool_n_sub));
  (void)hipFree(fs->d_pool);
  fs->d_pool = p, fs->pool_sub_cap = (uint32_t)cap;
  return SRZ_OK;
}

// Frames per sub-batch.  A LARGE set is rendered as sub-batches of whole frames one after the other on the same stream: what k_raster leaves
// for k_shade (depth, owner ids) and k_bin for k_raster (records) stays in the 256 MiB Infinity Cache only while the frames in flight are few
// (config 2, 1024 frames in pieces of 176 / 208 / 256 / 344 / 512: 0.633 / 0.644 / 0.656 / 0.653 / 0.632 of the roofline: NOTEBOOK r6 §6).
// A sub-batch is a view: every per-frame array from its first frame on; counters, record pool and work lists are shared (k_setup resets
// them, and stream order keeps one sub-batch's kernels behind the previous one's).  Its size is 256 frames' worth of 1024^2 (≈ 262 k tiles)
// in frames of THIS set; frames so large that fewer than 96 make a sub-batch (2048^2 and up) are left alone.  SRZ_SUB_BATCH (tests) fixes it.
int sub_batch_frames(const srz_ctx *ctx, const srz_frameset *fs, int n_all, bool one_piece) {
  const size_t tiles_per_frame = std::max<size_t>((size_t)fs->n_local_bands * fs->tiles_x, 1);
  const int sub = ctx->env_sub_batch > 0 ? ctx->env_sub_batch : (int)std::min<size_t>((256u * 1024u / tiles_per_frame + 7u) / 8u * 8u, 1u << 20);
  if (sub < 96 || n_all < sub + sub / 4 || one_piece) return n_all;
  const int parts = (n_all + sub - 1) / sub;
  return ((n_all + parts - 1) / parts + 7) / 8 * 8;
}

// The side clear of one render (srz_frameset::ClearTune): its grid, RenderArgs::clear_wgs_dev, and how end_clear_plan ends the render
struct ClearPlan {
  uint32_t wgs = CLEAR_GRID_DEFAULT, *dev_wgs = nullptr;
  bool count = false, stamp = false, rebase = false;
};

// The grids sets of this ctx have measured, by the shape of the set as far as the clear's best grid depends on it: frame size, frames,
// bands, triangles, the shading builds in use.  wgs 0: looks the shape up (0: not measured); else files wgs for it.
uint32_t clear_memo(srz_ctx *ctx, const srz_frameset *fs, uint32_t wgs) {
  uint64_t key = 0xcbf29ce484222325ull;
  for (uint64_t v : {(uint64_t)fs->width, (uint64_t)fs->height, (uint64_t)fs->n_frames, (uint64_t)fs->n_local_bands, fs->total_tris,
                     (uint64_t)fs->fast_kinds, (uint64_t)fs->approx_shade})
    key = (key ^ v) * 0x100000001b3ull;
  auto it = std::find_if(ctx->clear_memo.begin(), ctx->clear_memo.end(), [&](const std::pair<uint64_t, uint32_t> &m) { return m.first == key; });
  if (wgs == 0u) return it != ctx->clear_memo.end() ? it->second : 0u;
  if (it != ctx->clear_memo.end()) it->second = wgs;
  else if (ctx->clear_memo.size() < 256) ctx->clear_memo.emplace_back(key, wgs);
  return wgs;
}

// The plan of a render that clears beside k_raster (detailed: the per-kernel timing mode's barriers — not a sample, not counted)
int plan_clear(srz_ctx *ctx, srz_frameset *fs, const Pass &pass, bool detailed, hipStream_t s, ClearPlan &p) {
  srz_frameset::ClearTune &ct = fs->clear_tune;
  p = ClearPlan{ctx->env_clear_wgs ? ctx->env_clear_wgs : ct.wgs};
  if (ctx->env_clear_wgs || !ct.d_ctl) return SRZ_OK;
  p.rebase = pass.writes_visibility() && !ct.done; // (the grid in effect; the next colour render's sample then times itself alone)
  if (pass.kind != Pass::COLOUR || pass.f_count >= 0) return SRZ_OK;
  if (ct.done && !detailed && ++ct.since >= srz_frameset::CLEAR_TUNE_AGAIN) {
    // what the clear runs beside may have changed (srz_sceneset_update): measure again (<= 18 of 4096 renders)
    ct.done = false, ct.since = 0, ct.renders = srz_frameset::CLEAR_TUNE_SKIP;
    *static_cast<volatile uint32_t *>(ct.h_wgs) = 0u; // (no k_clear_tune is in flight: the host stopped launching them when it saw the decision)
    HIP_TRY(ctx, hipMemsetAsync(ct.d_ctl, 0, sizeof(ClearCtl), s));
  }
  if (!ct.done && ct.renders == 0) // (the set's first render: has a set of this shape measured before?)
    if (const uint32_t m = clear_memo(ctx, fs, 0u)) ct.wgs = p.wgs = m, ct.done = true;
  if (ct.done) return SRZ_OK;
  const uint32_t h = *static_cast<volatile uint32_t *>(ct.h_wgs);
  const int j = ct.renders - srz_frameset::CLEAR_TUNE_SKIP;
  if (h != 0u) { // decided: launch that grid from now on
    ct.wgs = p.wgs = h, ct.done = true;
    clear_memo(ctx, fs, h);
  } else if (!detailed && j < 0) { // (the first CLEAR_TUNE_SKIP renders are not measured)
    p.count = true;
  } else if (!detailed) { // measuring (or the decision has not reached the host yet): the device says how many of the grid take part
    p.wgs = CLEAR_GRID_MAX, p.dev_wgs = &ct.d_ctl->wgs;
    p.count = p.stamp = j < CLEAR_TUNE_RENDERS;
  }
  return SRZ_OK;
}

// After the render's last launch: counts it towards the measurement (here: an early error return loses no stamp) and ends it as planned
void end_clear_plan(srz_frameset *fs, const ClearPlan &p, hipStream_t s) {
  if (p.count) ++fs->clear_tune.renders;
  if (p.stamp) launch_clear_tune(fs->clear_tune.d_ctl, fs->clear_tune.h_wgs, s);
  if (p.rebase) launch_clear_rebase(fs->clear_tune.d_ctl, s);
}

struct RenderPlan { // what render_impl decided for the whole render, as each sub-batch needs it
  Pass pass;
  hipStream_t s;
  bool side, turns, vertex_setup;
  ClearPlan clear;
  EventPair *ep; // the per-kernel timing mode: t1 / t2 go around k_raster; else null
};

// setup → bands → raster → shade of frames [f0, f0 + n) of the render (sub-batch `part`).  `a` is the whole render's arguments: the
// first render's growth of the record pool updates them for the sub-batches that follow.
int enqueue_sub_batch(srz_ctx *ctx, srz_frameset *fs, const RenderPlan &r, RenderArgs &a, int f0, int n, int part) {
  const bool stats = r.pass.kind == Pass::COUNTING;
  const hipStream_t s = r.s;
  const size_t tpf = (size_t)fs->n_local_bands * fs->tiles_x;
  RenderArgs v = a;
  if (n != fs->n_frames) {
    const int fa = r.pass.f_begin + f0; // (first frame of this piece in the set)
    v.frames += fa, v.n_frames = (uint32_t)n;
    v.vis += (size_t)fa * tpf * ((size_t)TILE * TILE);
    v.tile_info += (size_t)fa * tpf;
    v.out += (size_t)fa * a.frame_stride;
    v.work_cap = (uint32_t)((size_t)(n < 8 ? n : (n + 7) / 8) * tpf);
  }
  const uint32_t tiles = (uint32_t)((size_t)n * tpf);
  if (r.vertex_setup) launch_chunks(v, n, fs->max_tris, s);
  else launch_setup(v, n, fs->max_tris, stats, s);
  launch_bin(v, n, fs->max_tris, s);
  // The FIRST render of a set sizes the pool by what it needs itself: it waits for k_bin's count, grows the pool if a band
  // did not fit and bins again — a one-shot set (srz_draw_batch, the host layer's per-draw sets) has no second render that
  // could profit from the lazy growth, and would otherwise leave its overflowing bands to the ordered rasteriser.
  if (!fs->pool_sized && !stats) {
    HIP_TRY(ctx, copy_demand(fs, part, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    const uint32_t need = max_pool_demand(fs, part, part + 1);
    if (need > fs->pool_sub_cap) {
      if (int rc = grow_pool(ctx, fs, need, 8u)) return rc; // (earlier sub-batches of this render may still be reading the old pool)
      a.pool = v.pool = fs->d_pool, a.pool_sub_cap = v.pool_sub_cap = fs->pool_sub_cap;
      HIP_TRY(ctx, hipMemsetAsync(fs->d_pool_heads, 0, sizeof(uint32_t) * CNT_STRIDE * fs->pool_n_sub, s));
      launch_bin(v, n, fs->max_tris, s);
    }
  }
  if (r.pass.kind == Pass::SIZE_ONLY) return SRZ_OK; // (the creation-time pass ends with the binning)
  if (r.ep) HIP_TRY(ctx, hipEventRecord(r.ep->t1, s));
  const unsigned ev = r.side ? ctx->ev_next++ % srz_ctx::EV_RING : 0u;
  if (r.side) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fork[ev], s));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_fork[ev], 0));
    launch_clear(v, tiles, ctx->stream2, r.clear.wgs);
    // (in front of the join: whatever follows on the launch stream — the next sub-batch's or render's k_setup zeroes the
    // allocators — is ordered behind this copy; it is 16 words behind a kernel that outlasts k_raster)
    HIP_TRY(ctx, copy_demand(fs, part, ctx->stream2));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_join[ev], ctx->stream2));
  }
  // (a peel: k_peel in k_raster's place, reading the previous layer at the same frame offset as v.out)
  if (r.pass.kind == Pass::PEEL) launch_peel(v, r.pass.d_prev + (v.out - a.out), n, s);
  else launch_raster(v, n, stats, s);
  if (r.turns) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev_raster[ctx->raster_next++ % srz_ctx::EV_RING], s));
    ctx->raster_last_stream = s, ctx->raster_valid = true;
  }
  if (r.ep) HIP_TRY(ctx, hipEventRecord(r.ep->t2, s));
  if (r.pass.writes_visibility()) launch_visibility(v, tiles, s);
  else launch_shade(v, tiles, stats, fs->fast_kinds, fs->any_generic, fs->approx_shade, s);
  if (r.side) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_join[ev], 0));
  else if (r.pass.kind == Pass::PEEL || !raster_four_waves(v)) // (the latency build of k_raster stores the demand itself)
    HIP_TRY(ctx, copy_demand(fs, part, s));
  return SRZ_OK;
}

// a set the ctx can render or shade now: made under the ctx's shard, its last update complete
int check_renderable(srz_ctx *ctx, const srz_frameset *fs) {
  if (fs->shard_rank != ctx->shard_rank || fs->shard_world != ctx->shard_world)
    return fail(ctx, SRZ_E_INVALID, "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)");
  if (fs->update_failed) return fail(ctx, SRZ_E_NOMEM, "the last update of this set failed (out of memory): update it again or destroy it");
  return SRZ_OK;
}

// setup → bands → raster → shade for every frame of the set (or of pass.f_begin.., pass.f_count), asynchronously on `s`
int render_impl(srz_ctx *ctx, srz_frameset *fs, float *d_out, uint32_t flags_or, hipStream_t s, Pass pass) {
  const bool stats = pass.kind == Pass::COUNTING, size_only = pass.kind == Pass::SIZE_ONLY;
  if (int rc = check_renderable(ctx, fs)) return rc;
  if (pass.kind == Pass::COLOUR || stats)
    if (int rc = resolve_shading(ctx, fs, s)) return rc;
  // The record pool follows what the previous renders asked for: growing is rare and the one place where a render waits for the device.
  // (Whatever h_pool_heads holds is a demand some finished or running render of this set really had: a stale value only delays the growth.)
  const uint32_t need = max_pool_demand(fs, 0, srz_frameset::DEMAND_PARTS);
  if (need > fs->pool_sub_cap)
    if (int rc = grow_pool(ctx, fs, need, 4u)) return rc;
  RenderArgs a = make_args(ctx, fs, d_out, flags_or, pass);
  if (!size_only) fs->last_flags = flags_or, fs->rendered = true; // (this render rewrites d_tile_info: srz_frameset_sparse_pack)
  EventPair ep{};
  const bool timed = ctx->timing != 0 && !stats && !size_only && ctx->ev_used.size() < 65536, detailed = timed && ctx->timing >= 2;
  if (timed)
    if (int rc = begin_timing(ctx, ep, detailed, s)) return rc;
  if (stats) HIP_TRY(ctx, hipMemsetAsync(ctx->d_stats, 0, ST_COUNT * sizeof(unsigned long long), s));
  if (fs->max_tris == 0) { // (else: k_setup resets the per-render counters)
    HIP_TRY(ctx, hipMemsetAsync(fs->d_work_count, 0, sizeof(uint32_t) * CNT_STRIDE * N_WORK_LISTS, s));
    HIP_TRY(ctx, hipMemsetAsync(fs->d_pool_heads, 0, sizeof(uint32_t) * CNT_STRIDE * fs->pool_n_sub, s));
    HIP_TRY(ctx, hipMemsetAsync(fs->d_slow_count, 0, 2 * sizeof(uint32_t), s));
  }
  const bool turns = !stats && !size_only && fs->max_tiles >= 8192; // (batches; small jobs are launch-bound and gain nothing)
  if (turns && !ctx->ev_raster[0])
    if (int rc = create_side(ctx, "render: raster events", nullptr, false, ctx->ev_raster)) return rc;
  if (turns && ctx->raster_valid && ctx->raster_last_stream != s) {
    HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_raster[(ctx->raster_next + srz_ctx::EV_RING - 1) % srz_ctx::EV_RING], 0));
    a.other_streams = 1u;
  }
  // vertex stage on the device; outside counting runs it does the triangles' setup too (cull + bounding box from the registers
  // that hold the transformed triangle), and k_chunks replaces k_setup below
  const bool vertex_setup = fs->d_draws != nullptr && !stats;
  if (fs->d_draws) launch_vertex(fs->d_draws, fs->n_draws, fs->max_faces, fs->d_tris, fs->d_tri_pos, fs->d_frames, vertex_setup ? fs->d_bbox : nullptr, s);
  // fused clear of the tiles no bbox reaches: beside k_raster on a second stream (batches), or in the rasteriser (small jobs)
  const bool any_fused = any_frame_has(fs, flags_or, SRZ_FUSED_CLEAR), side = any_fused && fs->max_tiles >= 8192 && !size_only;
  // The clear must run BESIDE the launch stream, so it may not share a hardware queue with it (HIP deals its streams round-robin onto a few:
  // seen, the clear in front of k_raster, +20 % per render).  Streams of another priority live on queues of their own; the clear is throttled
  // by its grid size, not by priority, so the highest one costs the rasteriser nothing.
  if (side && !ctx->stream2)
    if (int rc = create_side(ctx, "render: clear stream", &ctx->stream2, true, ctx->ev_fork, ctx->ev_join)) return rc;
  if (!side && any_fused) a.clear_in_raster = 1u; // (small job: the rasteriser's own waves clear the tiles no bbox reaches)
  RenderPlan r{pass, s, side, turns, vertex_setup, ClearPlan{}, detailed ? &ep : nullptr};
  if (side)
    if (int rc = plan_clear(ctx, fs, pass, detailed, s, r.clear)) return rc;
  a.clear_wgs_dev = r.clear.dev_wgs;
  const int n_all = pass.f_count < 0 ? fs->n_frames : pass.f_count;
  const int chunk = sub_batch_frames(ctx, fs, n_all, stats || detailed);
  for (int f0 = 0, part = 0; f0 < n_all; f0 += chunk, ++part)
    if (int rc = enqueue_sub_batch(ctx, fs, r, a, f0, std::min(chunk, n_all - f0), part)) return rc;
  if (!stats) fs->pool_sized = true;
  end_clear_plan(fs, r.clear, s);
  if (timed) {
    HIP_TRY(ctx, hipEventRecord(ep.t3, s));
    ctx->ev_used.push_back(ep);
  }
  HIP_TRY(ctx, hipGetLastError());
  return SRZ_OK;
}

// srz_frameset_render / _render_visibility
int render_entry(const char *name, srz_ctx *ctx, srz_frameset *fs, void *d_out, size_t out_bytes, uint32_t flags, void *stream, Pass pass) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn(name);
  if (!fs || !d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / output");
  if (out_bytes < srz_frameset_out_bytes(ctx, fs)) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (((uintptr_t)d_out & 15u) != 0) return fail(ctx, SRZ_E_INVALID, fn + ": output must be 16-byte aligned");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return render_impl(ctx, fs, (float *)d_out, flags & FRAME_FLAGS, pick_stream(ctx, stream), pass);
}

int read_stats(srz_ctx *ctx, hipStream_t s, srz_stats *st) {
  unsigned long long h[ST_COUNT];
  HIP_TRY(ctx, hipMemcpyAsync(h, ctx->d_stats, sizeof h, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  st->n_tris = h[ST_TRIS], st->n_culled = h[ST_CULLED], st->pixel_tests = h[ST_PIXEL_TESTS];
  st->fragments = h[ST_FRAGMENTS], st->shaded = h[ST_SHADED], st->visible = h[ST_VISIBLE];
  st->visible_textured = h[ST_VISIBLE_TEX];
  std::memcpy(ctx->dbg, h, sizeof h);
  return SRZ_OK;
}

// The counters of srz_stats are those of the reference's ORDERED walk ("shaded" = fragments that pass the z-test when
// their triangle is drawn), which the order-independent rasteriser does not produce.  A draw that asks for them runs the
// counting kernels (ordered rasteriser) once more on a scratch copy of the framebuffer the draw starts from.
int stats_pass(srz_ctx *ctx, srz_frameset *fs, const float *d_start, uint32_t flags_or, hipStream_t s, srz_stats *st) {
  const size_t bytes = (size_t)fs->n_frames * 4u * fs->local_rows * (size_t)fs->width * sizeof(float);
  float *d_tmp = nullptr;
  HIP_TRY(ctx, hipMalloc(&d_tmp, bytes));
  hipError_t e = d_start ? hipMemcpyAsync(d_tmp, d_start, bytes, hipMemcpyDeviceToDevice, s) : hipSuccess;
  int rc = e == hipSuccess ? render_impl(ctx, fs, d_tmp, flags_or, s, Pass::counting()) : fail(ctx, SRZ_E_NODEVICE, hipGetErrorString(e));
  if (rc == SRZ_OK) rc = read_stats(ctx, s, st); // (synchronises s)
  else (void)hipStreamSynchronize(s);
  (void)hipFree(d_tmp);
  return rc;
}

} // namespace

// The passes over a visibility buffer (srz_frameset_shade_visibility .. srz_frameset_normal_map_grad): what their entry points share.
// Each entry point is its own argument rules, these checks, its own Args fields, the launch.
namespace {

int check_pass_flags(srz_ctx *ctx, const std::string &fn, uint32_t flags) {
  if ((flags & ~(uint32_t)SRZ_FUSED_CLEAR) != 0u) return fail(ctx, SRZ_E_INVALID, fn + ": only SRZ_FUSED_CLEAR is accepted in flags");
  return SRZ_OK;
}
// `n` (the caller's `name`: attr_tris, pos_tris) is what a per-triangle array of the caller holds per frame
int check_tri_count(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, const char *name, uint32_t n) {
  for (const FrameDesc &d : fs->h_frames)
    if (d.n_tris > n) return fail(ctx, SRZ_E_INVALID, fn + ": " + name + " is below a frame's triangle count");
  return SRZ_OK;
}
// the plane buffers (16 bytes: the kernels move them four words at a time) and the per-triangle arrays (4 bytes); a null pointer,
// where an entry point lets one through, counts as aligned
template <uintptr_t BYTES> bool aligned(std::initializer_list<const void *> ptrs) {
  uintptr_t bits = 0;
  for (const void *p : ptrs) bits |= (uintptr_t)p;
  return (bits & (BYTES - 1u)) == 0;
}
struct Range { // (a null pointer overlaps nothing)
  const void *p;
  size_t bytes;
};
bool ranges_overlap(Range x, Range y) {
  const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
  return x.p && y.p && a < b + y.bytes && b < a + x.bytes;
}
// the gradient passes: no output overlaps an input (any number of them), and the two outputs do not overlap each other
template <size_t N_IN> int check_grad_overlap(srz_ctx *ctx, const std::string &fn, const Range (&outs)[2], const Range (&ins)[N_IN]) {
  for (const Range &o : outs)
    for (const Range &i : ins)
      if (ranges_overlap(o, i)) return fail(ctx, SRZ_E_INVALID, fn + ": an output overlaps an input");
  if (ranges_overlap(outs[0], outs[1])) return fail(ctx, SRZ_E_INVALID, fn + ": the two outputs overlap");
  return SRZ_OK;
}
// What a pass does once its arguments are accepted: the set is renderable, the device current, the stream picked (*s).  Then, as
// `steps` asks: the shading state resolved (textures uploaded, batch → shader / texture), and a sceneset's vertex stage run again —
// its triangles are that stage's output, computed as a render computes them (no setup: nothing is rasterised).
enum : unsigned { PASS_SHADING = 1u, PASS_VERTEX = 2u };
int begin_pass(srz_ctx *ctx, srz_frameset *fs, void *stream, unsigned steps, hipStream_t *s) {
  if (int rc = check_renderable(ctx, fs)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  *s = pick_stream(ctx, stream);
  if (steps & PASS_SHADING)
    if (int rc = resolve_shading(ctx, fs, *s)) return rc;
  if ((steps & PASS_VERTEX) && fs->d_draws)
    launch_vertex(fs->d_draws, fs->n_draws, fs->max_faces, fs->d_tris, fs->d_tri_pos, fs->d_frames, nullptr, *s);
  return SRZ_OK;
}
int end_pass(srz_ctx *ctx) {
  HIP_TRY(ctx, hipGetLastError());
  return SRZ_OK;
}

uint64_t plane_words(const srz_frameset *fs) { return fs->local_rows * (uint64_t)fs->width; }
// the fields every pass's Args names alike: the frames, the two buffers, and what the walk over the set's tiles reads
template <class Args> void fill_walk(Args &a, const srz_frameset *fs, const void *d_vis, void *d_out) {
  a.frames = fs->d_frames, a.vis = (const float *)d_vis, a.out = (float *)d_out;
  a.local_rows = fs->local_rows, a.tiles_x = fs->tiles_x, a.n_local_bands = fs->n_local_bands, a.n_frames = (uint32_t)fs->n_frames;
  a.shard_rank = fs->shard_rank, a.shard_world = fs->shard_world;
}
// what srz_frameset_interpolate and _interpolate_grad check alike; the attribute array's bytes in *attr_bytes
int check_interp(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, uint32_t n_ch, uint32_t attr_frames, uint32_t attr_tris,
                 uint32_t flags, size_t *attr_bytes) {
  if (n_ch == 0u || n_ch > SRZ_ATTR_MAX_CH) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. SRZ_ATTR_MAX_CH");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  if (attr_frames != 1u && attr_frames != (uint32_t)fs->n_frames)
    return fail(ctx, SRZ_E_INVALID, fn + ": attr_frames must be 1 or the set's frame count");
  if (int rc = check_tri_count(ctx, fs, fn, "attr_tris", attr_tris)) return rc;
  *attr_bytes = (size_t)attr_frames * attr_tris * 3u * n_ch * sizeof(float);
  return SRZ_OK;
}
InterpArgs interp_args(const srz_frameset *fs, const void *d_vis, const float *d_attr, uint32_t n_ch, uint32_t attr_frames, uint32_t attr_tris,
                       uint32_t out_planes, void *d_out, uint32_t flags) {
  InterpArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.attr = d_attr;
  a.vis_stride = 4ull * plane, a.frame_stride = out_planes * plane, a.gout_stride = n_ch * plane;
  a.attr_frame_stride = attr_frames == 1u ? 0ull : (uint64_t)attr_tris * 3u * n_ch;
  a.n_ch = n_ch;
  a.flags_or = flags;
  return a;
}
// what srz_frameset_antialias and _antialias_grad check alike
int check_antialias(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, uint32_t n_ch, uint32_t flags) {
  if (n_ch == 0u || n_ch > SRZ_ATTR_MAX_CH) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. SRZ_ATTR_MAX_CH");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  if (fs->shard_world > 1)
    return fail(ctx, SRZ_E_INVALID, fn + ": needs the whole frame on this ctx (a vertical pair across a band edge needs another rank's rows)");
  return SRZ_OK;
}
AntialiasArgs antialias_args(const srz_frameset *fs, const void *d_vis, const void *d_in, uint32_t n_ch, void *d_out) {
  AntialiasArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  fill_positions(a, fs);
  a.in = (const float *)d_in;
  a.vis_stride = 4ull * plane, a.frame_stride = n_ch * plane;
  a.n_ch = n_ch;
  return a;
}
// what srz_frameset_texture and _texture_grad check alike; the texture's bytes in *tex_bytes
int check_texture(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, uint32_t tex_w, uint32_t tex_h, uint32_t n_ch,
                  uint32_t tex_frames, uint32_t mode, uint32_t flags, size_t *tex_bytes) {
  if (n_ch == 0u || n_ch > SRZ_ATTR_MAX_CH) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. SRZ_ATTR_MAX_CH");
  if (tex_w == 0u || tex_w > SRZ_TEX_MAX_SIZE || tex_h == 0u || tex_h > SRZ_TEX_MAX_SIZE)
    return fail(ctx, SRZ_E_INVALID, fn + ": tex_w and tex_h must be 1 .. SRZ_TEX_MAX_SIZE");
  if (mode != SRZ_TEX_CLAMP && mode != SRZ_TEX_WRAP) return fail(ctx, SRZ_E_INVALID, fn + ": mode must be SRZ_TEX_CLAMP or SRZ_TEX_WRAP");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  if (tex_frames != 1u && tex_frames != (uint32_t)fs->n_frames)
    return fail(ctx, SRZ_E_INVALID, fn + ": tex_frames must be 1 or the set's frame count");
  *tex_bytes = (size_t)tex_frames * tex_h * tex_w * n_ch * sizeof(float);
  return SRZ_OK;
}
TexArgs texture_args(const srz_frameset *fs, const void *d_vis, const void *d_uv, const float *d_tex, uint32_t tex_w, uint32_t tex_h,
                     uint32_t n_ch, uint32_t tex_frames, uint32_t mode, uint32_t out_planes, void *d_out, uint32_t flags) {
  TexArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.uv = (const float *)d_uv, a.tex = d_tex;
  a.vis_stride = 4ull * plane, a.frame_stride = out_planes * plane, a.uv_stride = 2ull * plane, a.gout_stride = n_ch * plane;
  a.tex_frame_stride = tex_frames == 1u ? 0ull : (uint64_t)tex_h * tex_w * n_ch;
  a.tex_w = tex_w, a.tex_h = tex_h, a.n_ch = n_ch, a.mode = mode;
  a.flags_or = flags;
  return a;
}
// what srz_frameset_texture_cube and _texture_cube_grad check alike; the cube's bytes in *tex_bytes
int check_cube(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t flags,
               size_t *tex_bytes) {
  if (n_ch == 0u || n_ch > SRZ_ATTR_MAX_CH) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. SRZ_ATTR_MAX_CH");
  if (n == 0u || n > SRZ_TEX_MAX_SIZE) return fail(ctx, SRZ_E_INVALID, fn + ": n must be 1 .. SRZ_TEX_MAX_SIZE");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  if (tex_frames != 1u && tex_frames != (uint32_t)fs->n_frames)
    return fail(ctx, SRZ_E_INVALID, fn + ": tex_frames must be 1 or the set's frame count");
  *tex_bytes = (size_t)tex_frames * 6u * n * n * n_ch * sizeof(float);
  return SRZ_OK;
}
CubeArgs cube_args(const srz_frameset *fs, const void *d_vis, const void *d_dir, const float *d_tex, uint32_t n, uint32_t n_ch,
                   uint32_t tex_frames, uint32_t out_planes, void *d_out, uint32_t flags) {
  CubeArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.dir = (const float *)d_dir, a.tex = d_tex;
  a.vis_stride = 4ull * plane, a.frame_stride = out_planes * plane, a.dir_stride = 3ull * plane, a.gout_stride = n_ch * plane;
  a.tex_frame_stride = tex_frames == 1u ? 0ull : 6ull * n * n * n_ch;
  a.n = n, a.n_ch = n_ch;
  a.flags_or = flags;
  return a;
}
// the mip passes: any number of outputs against any number of inputs, and the outputs against each other
int check_overlaps(srz_ctx *ctx, const std::string &fn, std::initializer_list<Range> outs, std::initializer_list<Range> ins) {
  for (const Range *o = outs.begin(); o != outs.end(); ++o) {
    for (const Range &i : ins)
      if (ranges_overlap(*o, i)) return fail(ctx, SRZ_E_INVALID, fn + ": an output overlaps an input");
    for (const Range *p = o + 1; p != outs.end(); ++p)
      if (ranges_overlap(*o, *p)) return fail(ctx, SRZ_E_INVALID, fn + ": two outputs overlap");
  }
  return SRZ_OK;
}
// what srz_frameset_light and _light_grad check alike (check_cube's shape); the parameter block's bytes in *par_bytes
int check_light(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, uint32_t n_lights, uint32_t par_frames, uint32_t p, uint32_t flags,
                size_t *par_bytes) {
  if (n_lights == 0u || n_lights > SRZ_LIGHT_MAX) return fail(ctx, SRZ_E_INVALID, fn + ": n_lights must be 1 .. SRZ_LIGHT_MAX");
  if (p == 0u || p > 256u) return fail(ctx, SRZ_E_INVALID, fn + ": p must be 1 .. 256");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  if (par_frames != 1u && par_frames != (uint32_t)fs->n_frames)
    return fail(ctx, SRZ_E_INVALID, fn + ": par_frames must be 1 or the set's frame count");
  *par_bytes = (size_t)par_frames * SRZ_LIGHT_PAR(n_lights) * sizeof(float);
  return SRZ_OK;
}
LightArgs light_args(const srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const void *d_kd, const float *d_par,
                     uint32_t n_lights, uint32_t par_frames, uint32_t p, void *d_out, uint32_t flags) {
  LightArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.nrm = (const float *)d_nrm, a.pos = (const float *)d_pos, a.kd = (const float *)d_kd, a.par = d_par;
  a.vis_stride = 4ull * plane, a.frame_stride = 3ull * plane;
  a.par_stride = par_frames == 1u ? 0ull : (uint64_t)SRZ_LIGHT_PAR(n_lights);
  a.n_lights = n_lights, a.p = p;
  a.flags_or = flags;
  return a;
}
// what srz_frameset_shadow and _shadow_grad check alike (check_cube's shape); the map's bytes in *map_bytes
int check_shadow(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, uint32_t map_w, uint32_t map_h, uint32_t map_frames, float bias,
                 float width, uint32_t flags, size_t *map_bytes) {
  if (map_w == 0u || map_w > SRZ_TEX_MAX_SIZE || map_h == 0u || map_h > SRZ_TEX_MAX_SIZE)
    return fail(ctx, SRZ_E_INVALID, fn + ": map_w and map_h must be 1 .. SRZ_TEX_MAX_SIZE");
  if (!std::isfinite(bias) || !std::isfinite(width)) return fail(ctx, SRZ_E_INVALID, fn + ": bias and width must be finite");
  if (width < 0.0f) return fail(ctx, SRZ_E_INVALID, fn + ": width must be >= 0 (0: the hard test)");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  if (map_frames != 1u && map_frames != (uint32_t)fs->n_frames)
    return fail(ctx, SRZ_E_INVALID, fn + ": map_frames must be 1 or the set's frame count");
  *map_bytes = (size_t)map_frames * map_h * map_w * sizeof(float);
  return SRZ_OK;
}
ShadowArgs shadow_args(const srz_frameset *fs, const void *d_vis, const void *d_sc, const float *d_map, uint32_t map_w, uint32_t map_h,
                       uint32_t map_frames, float bias, float width, uint32_t out_planes, void *d_out, uint32_t flags) {
  ShadowArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.sc = (const float *)d_sc, a.map = d_map;
  a.vis_stride = 4ull * plane, a.frame_stride = out_planes * plane, a.sc_stride = 3ull * plane, a.gout_stride = plane;
  a.map_frame_stride = map_frames == 1u ? 0ull : (uint64_t)map_h * map_w;
  a.map_w = map_w, a.map_h = map_h, a.bias = bias, a.width = width;
  a.flags_or = flags;
  return a;
}
constexpr uint32_t MIP_MAX_FRAMES = 65536u;
// what srz_texture_mip_build and _mip_fold check alike (no set: tex_frames is any count up to MIP_MAX_FRAMES)
int check_mip(srz_ctx *ctx, const std::string &fn, uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels,
              size_t mip_bytes, const void *tex, const void *mip) {
  if (!tex) return fail(ctx, SRZ_E_INVALID, fn + ": null texture");
  if (n_ch == 0u || n_ch > SRZ_ATTR_MAX_CH) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. SRZ_ATTR_MAX_CH");
  if (tex_w == 0u || tex_w > SRZ_TEX_MAX_SIZE || tex_h == 0u || tex_h > SRZ_TEX_MAX_SIZE)
    return fail(ctx, SRZ_E_INVALID, fn + ": tex_w and tex_h must be 1 .. SRZ_TEX_MAX_SIZE");
  if (tex_frames == 0u || tex_frames > MIP_MAX_FRAMES) return fail(ctx, SRZ_E_INVALID, fn + ": tex_frames must be 1 .. 65536");
  if (n_levels == 0u || n_levels > srz_texture_mip_levels(tex_w, tex_h))
    return fail(ctx, SRZ_E_INVALID, fn + ": n_levels must be 1 .. srz_texture_mip_levels(tex_w, tex_h)");
  if (!mip && n_levels > 1u) return fail(ctx, SRZ_E_INVALID, fn + ": null pyramid"); // (one level: there is none)
  const size_t need = srz_texture_mip_bytes(tex_w, tex_h, n_ch, tex_frames, n_levels);
  if (mip_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": mip_bytes is below srz_texture_mip_bytes");
  if (!aligned<4>({tex, mip})) return fail(ctx, SRZ_E_INVALID, fn + ": the texture and the pyramid must be 4-byte aligned");
  if (ranges_overlap({tex, (size_t)tex_frames * tex_h * tex_w * n_ch * sizeof(float)}, {mip, need}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the pyramid overlaps the texture");
  return SRZ_OK;
}
// what srz_frameset_texture_mip and _texture_mip_grad check alike behind check_texture; the pyramid's bytes in *mip_bytes
int check_tex_mip(srz_ctx *ctx, const std::string &fn, uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels,
                  const void *d_uvd, size_t *mip_bytes) {
  if (n_levels == 0u || n_levels > srz_texture_mip_levels(tex_w, tex_h))
    return fail(ctx, SRZ_E_INVALID, fn + ": n_levels must be 1 .. srz_texture_mip_levels(tex_w, tex_h)");
  if (n_levels > 1u && !d_uvd) return fail(ctx, SRZ_E_INVALID, fn + ": n_levels > 1 needs the derivative planes");
  *mip_bytes = srz_texture_mip_bytes(tex_w, tex_h, n_ch, tex_frames, n_levels);
  return SRZ_OK;
}
TexMipArgs texture_mip_args(const srz_frameset *fs, const void *d_vis, const void *d_uv, const void *d_uvd, const float *d_tex,
                            const float *d_mip, uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t mode,
                            uint32_t n_levels, uint32_t out_planes, void *d_out, uint32_t flags) {
  TexMipArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.uv = (const float *)d_uv, a.uvd = (const float *)d_uvd, a.tex = d_tex, a.mip = d_mip;
  a.vis_stride = 4ull * plane, a.frame_stride = out_planes * plane, a.uv_stride = 2ull * plane, a.gout_stride = n_ch * plane;
  a.tex_w = tex_w, a.tex_h = tex_h, a.n_ch = n_ch, a.mode = mode, a.tex_frames = tex_frames, a.n_levels = n_levels;
  a.flags_or = flags;
  return a;
}
// what srz_frameset_texture_cube_mip and _texture_cube_mip_grad check alike behind check_cube; the pyramid's bytes in *mip_bytes
int check_cube_mip(srz_ctx *ctx, const std::string &fn, uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels, const void *d_lam,
                   size_t *mip_bytes) {
  if (n_levels == 0u || n_levels > srz_cube_mip_levels(n)) return fail(ctx, SRZ_E_INVALID, fn + ": n_levels must be 1 .. srz_cube_mip_levels(n)");
  if (n_levels > 1u && tex_frames > MIP_MAX_FRAMES / 6u) return fail(ctx, SRZ_E_INVALID, fn + ": 6 * tex_frames must not exceed 65536 with a pyramid");
  if (n_levels > 1u && !d_lam) return fail(ctx, SRZ_E_INVALID, fn + ": n_levels > 1 needs the level plane");
  *mip_bytes = srz_cube_mip_bytes(n, n_ch, tex_frames, n_levels);
  return SRZ_OK;
}
CubeMipArgs cube_mip_args(const srz_frameset *fs, const void *d_vis, const void *d_dir, const void *d_lam, const float *d_tex, const float *d_mip,
                          uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels, uint32_t out_planes, void *d_out, uint32_t flags) {
  CubeMipArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.dir = (const float *)d_dir, a.lam = (const float *)d_lam, a.tex = d_tex, a.mip = d_mip;
  a.vis_stride = 4ull * plane, a.frame_stride = out_planes * plane, a.dir_stride = 3ull * plane, a.gout_stride = n_ch * plane, a.lam_stride = plane;
  a.n = n, a.n_ch = n_ch, a.tex_frames = tex_frames, a.n_levels = n_levels;
  a.flags_or = flags;
  return a;
}

} // namespace

extern "C" {

int srz_abi_version(void) { return SRZ_ABI_VERSION; }

int srz_create(srz_ctx **out, int device_id) {
  if (!out) return fail(nullptr, SRZ_E_INVALID, "srz_create: out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, SRZ_E_NODEVICE,
                std::string("srz_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count=0") +
                    "); this library has no CPU fallback");
  if (device_id < 0 || device_id >= n) return fail(nullptr, SRZ_E_INVALID, "srz_create: device_id out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) != hipSuccess)
    return fail(nullptr, SRZ_E_NODEVICE, "srz_create: hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, SRZ_E_NODEVICE, std::string("srz_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
  srz_ctx *ctx = new (std::nothrow) srz_ctx();
  if (!ctx) return fail(nullptr, SRZ_E_NOMEM, "srz_create: out of host memory");
  ctx->device = device_id;
  ctx->env_sub_batch = getenv("SRZ_SUB_BATCH") ? atoi(getenv("SRZ_SUB_BATCH")) : 0;
  ctx->env_no_packed = getenv("SRZ_NO_PACKED") != nullptr;
  ctx->env_clear_wgs = getenv("SRZ_CLEAR_WGS") ? (uint32_t)std::max(atoi(getenv("SRZ_CLEAR_WGS")), 0) : 0u;
  ctx->opt_pool_lazy = getenv("SRZ_POOL_LAZY") != nullptr;
  for (int i = 0; i < MAX_TEX; ++i) ctx->h_tex[i] = TexDesc{nullptr, 0, 0}, ctx->d_texmem[i] = nullptr;
  auto bail = [&](const char *what, hipError_t err) {
    g_create_error = std::string(what) + ": " + hipGetErrorString(err);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    (void)hipFree(ctx->d_stats);
    delete ctx;
    return SRZ_E_NODEVICE;
  };
  if ((e = hipSetDevice(device_id)) != hipSuccess) return bail("hipSetDevice", e);
  if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
  if ((e = hipMalloc(&ctx->d_stats, sizeof(unsigned long long) * ST_COUNT)) != hipSuccess) return bail("hipMalloc(stats)", e);
  *out = ctx;
  return SRZ_OK;
}

void srz_destroy(srz_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->draw_fs) srz_frameset_destroy(ctx, ctx->draw_fs);
  (void)hipFree(ctx->draw_out);
  (void)hipFree(ctx->batch_out);
  if (ctx->span_t0) (void)hipEventDestroy(ctx->span_t0);
  for (auto &ep : ctx->ev_used) ctx->ev_pool.push_back(ep);
  for (auto &ep : ctx->ev_pool) (void)hipEventDestroy(ep.t0), (void)hipEventDestroy(ep.t1), (void)hipEventDestroy(ep.t2), (void)hipEventDestroy(ep.t3);
  for (int i = 0; i < MAX_TEX; ++i) (void)hipFree(ctx->d_texmem[i]);
  for (int i = 0; i < MAX_MESH; ++i) (void)hipFree(ctx->mesh[i].d_verts), (void)hipFree(ctx->mesh[i].d_faces), (void)hipFree(ctx->mesh[i].d_corner_off);
  (void)hipFree(ctx->d_stats);
  destroy_side(ctx->stream2, ctx->ev_fork, ctx->ev_join);
  destroy_side(ctx->stream3, ctx->ev_piece);
  destroy_side(nullptr, ctx->ev_raster);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char *srz_last_error(const srz_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int srz_set_option(srz_ctx *ctx, int option, int value) {
  if (!ctx) return SRZ_E_INVALID;
  if (option == SRZ_OPT_POOL_LAZY)
    ctx->opt_pool_lazy = value != 0;
  else if (option == SRZ_OPT_APPROX_SHADE)
    ctx->opt_approx_shade = value != 0;
  else
    return fail(ctx, SRZ_E_INVALID, "srz_set_option: unknown option " + std::to_string(option));
  return SRZ_OK;
}

int srz_set_shard(srz_ctx *ctx, int rank, int world) {
  if (!ctx) return SRZ_E_INVALID;
  if (world < 1 || rank < 0 || rank >= world) return fail(ctx, SRZ_E_INVALID, "srz_set_shard: need 0 <= rank < world");
  ctx->shard_rank = rank, ctx->shard_world = world;
  return SRZ_OK;
}

int srz_texture_upload(srz_ctx *ctx, int tex_id, const uint8_t *bgr, int w, int h, int row_stride) {
  if (!ctx) return SRZ_E_INVALID;
  if (tex_id < 0 || tex_id >= MAX_TEX || !bgr || w <= 0 || h <= 0 || row_stride < 3 * w || w > 32768 || h > 32768)
    return fail(ctx, SRZ_E_INVALID, "srz_texture_upload: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint8_t *d_raw = nullptr;
  uint32_t *d_px = nullptr;
  size_t raw = (size_t)row_stride * h;
  HIP_TRY(ctx, hipMalloc(&d_raw, raw));
  hipError_t e = hipMalloc(&d_px, (size_t)w * h * 4);
  if (e != hipSuccess) {
    (void)hipFree(d_raw);
    return fail(ctx, SRZ_E_NOMEM, "srz_texture_upload: hipMalloc failed");
  }
  e = hipMemcpyAsync(d_raw, bgr, raw, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    launch_tex_convert(d_raw, w, h, row_stride, d_px, ctx->stream);
    e = hipStreamSynchronize(ctx->stream);
  }
  (void)hipFree(d_raw);
  if (e != hipSuccess) {
    (void)hipFree(d_px);
    return fail(ctx, SRZ_E_NODEVICE, std::string("srz_texture_upload: ") + hipGetErrorString(e));
  }
  (void)hipFree(ctx->d_texmem[tex_id]);
  ctx->d_texmem[tex_id] = d_px;
  ctx->h_tex[tex_id] = TexDesc{d_px, w, h};
  ctx->tex_version++;
  return SRZ_OK;
}

// the one writer of a frame's shading data: eye, ka, ks, p, kh, kn and the flags the device sees (classify_frames adds its own)
static void set_shading(FrameDesc &d, const srz_frame &fr) {
  std::memcpy(d.eye, fr.eye, sizeof d.eye), std::memcpy(d.ka, fr.ka, sizeof d.ka), std::memcpy(d.ks, fr.ks, sizeof d.ks);
  d.p = fr.p, d.kh = fr.kh, d.kn = fr.kn;
  d.flags = fr.flags & FRAME_FLAGS;
}

// the set's block [FrameDesc x n | lights | DrawDesc x draws] from its host copies into `st`, laid out as d_dyn
static void stage_dyn(const srz_frameset *fs, uint8_t *st) {
  std::memcpy(st, fs->h_frames.data(), sizeof(FrameDesc) * fs->h_frames.size());
  if (!fs->h_lights.empty()) std::memcpy(st + fs->dyn_lights_off, fs->h_lights.data(), sizeof(srz_light) * fs->h_lights.size());
  if (!fs->h_draws.empty()) std::memcpy(st + fs->dyn_draws_off, fs->h_draws.data(), sizeof(DrawDesc) * fs->h_draws.size());
}

// The set's staging ring, made at its first update, all or nothing: out of memory leaves the set as it was
static int ensure_stage_ring(srz_ctx *ctx, srz_frameset *fs, const char *who) {
  if (fs->h_stage[0]) return SRZ_OK;
  for (int i = 0; i < srz_frameset::STAGE_RING; ++i) {
    hipError_t e = hipHostMalloc((void **)&fs->h_stage[i], fs->dyn_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&fs->stage_ev[i], hipEventDisableTiming);
    if (e != hipSuccess) {
      for (int j = 0; j <= i; ++j) {
        if (fs->h_stage[j]) (void)hipHostFree(fs->h_stage[j]);
        if (fs->stage_ev[j]) (void)hipEventDestroy(fs->stage_ev[j]);
        fs->h_stage[j] = nullptr, fs->stage_ev[j] = nullptr;
      }
      return fail(ctx, e == hipErrorOutOfMemory ? SRZ_E_NOMEM : SRZ_E_NODEVICE, std::string(who) + ": staging buffers: " + hipGetErrorString(e));
    }
  }
  return SRZ_OK;
}

// The block's upload: ONE asynchronous copy on the context's stream from the next slot of the ring, ordered after every render already
// submitted there (which may still be reading the block) and before the next one.  Renders submitted on OTHER streams are the caller's
// to order.
static int upload_dyn(srz_ctx *ctx, srz_frameset *fs) {
  const unsigned slot = fs->stage_next++ % srz_frameset::STAGE_RING;
  if (fs->stage_busy[slot]) HIP_TRY(ctx, hipEventSynchronize(fs->stage_ev[slot])); // its copy of 4 updates ago
  stage_dyn(fs, fs->h_stage[slot]);
  HIP_TRY(ctx, hipMemcpyAsync(fs->d_dyn, fs->h_stage[slot], fs->dyn_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(fs->stage_ev[slot], ctx->stream));
  fs->stage_busy[slot] = true;
  return SRZ_OK;
}

// draws: the DrawDescs of a sceneset (their tri_off in the set's triangle order), null for a frameset
static int build_frameset(srz_ctx *ctx, const srz_frame *frames, int n_frames, srz_frameset **out, bool copy_tris, bool tris_aos = false,
                          const std::vector<DrawDesc> *draws = nullptr) {
  if (!ctx) return SRZ_E_INVALID;
  if (!out) return fail(ctx, SRZ_E_INVALID, "srz_frameset_create: out is NULL");
  *out = nullptr;
  if (!frames || n_frames <= 0) return fail(ctx, SRZ_E_INVALID, "srz_frameset_create: no frames");
  const int W = frames[0].width, H = frames[0].height;
  if (W <= 0 || H <= 0 || W > 32767 || H > 32767) return fail(ctx, SRZ_E_INVALID, "srz_frameset_create: width/height must be in 1..32767");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  srz_frameset *fs = new (std::nothrow) srz_frameset();
  if (!fs) return fail(ctx, SRZ_E_NOMEM, "srz_frameset_create: out of host memory");
  fs->n_frames = n_frames, fs->width = W, fs->height = H;
  fs->shard_rank = ctx->shard_rank, fs->shard_world = ctx->shard_world;
  shard_layout(H, fs->shard_rank, fs->shard_world, fs->n_bands, fs->n_local_bands, fs->bands_per_rank, fs->local_rows);
  fs->tiles_x = (uint32_t)((W + TILE - 1) / TILE);
  if ((uint64_t)((n_frames + 7) / 8 * 8) * fs->n_local_bands * fs->tiles_x >= 0x7fffffffull) {
    delete fs;
    return fail(ctx, SRZ_E_INVALID, "srz_frameset_create: frames x tiles exceeds the launch grid limit; split the batch");
  }
  uint64_t tri_off = 0, light_off = 0, batch_off = 0, group_off = 0;
  for (int f = 0; f < n_frames; ++f) {
    const srz_frame &fr = frames[f];
    auto bad = [&](const char *m) {
      delete fs;
      return fail(ctx, SRZ_E_INVALID, std::string("srz_frameset_create: frame ") + std::to_string(f) + ": " + m);
    };
    if (fr.width != W || fr.height != H) return bad("all frames of a set must share width/height");
    if ((fr.n_lights && !fr.lights) || (fr.n_batches && !fr.batches)) return bad("null lights/batches");
    if (fr.n_batches > 65535) return bad("more than 65535 batches");
    FrameDesc d{};
    d.width = W, d.height = H;
    set_shading(d, fr);
    d.n_lights = fr.n_lights, d.light_off = (uint32_t)light_off;
    d.tri_off = (uint32_t)tri_off, d.n_batches = fr.n_batches, d.batch_off = (uint32_t)batch_off;
    uint64_t nt = 0;
    for (uint32_t b = 0; b < fr.n_batches; ++b) {
      const srz_batch &sb = fr.batches[b];
      if (copy_tris && sb.n_tris && !sb.tris) return bad("batch with null triangle pointer");
      if (sb.shader < SRZ_SHADER_NORMAL || sb.shader > SRZ_SHADER_BUMP) return bad("unknown shader type");
      fs->h_batches.push_back(BatchDesc{sb.shader, sb.tex_id, (uint32_t)nt, sb.n_tris});
      nt += sb.n_tris;
    }
    if (tri_off + nt > 0xfffffff0ull || nt >= 0x7fffffffull) return bad("too many triangles");
    d.n_tris = (uint32_t)nt;
    d.n_local_bands = fs->n_local_bands;
    d.chunk_off = (uint32_t)(tri_off / 64u) + (uint32_t)f; // (every frame's chunk words start on a word of their own)
    d.group_off = (uint32_t)group_off;
    group_off += (nt + GROUP_TRIS - 1u) / GROUP_TRIS;
    fs->h_frames.push_back(d);
    fs->max_tris = std::max(fs->max_tris, d.n_tris);
    tri_off += nt, light_off += fr.n_lights, batch_off += fr.n_batches;
  }
  fs->total_tris = tri_off, fs->total_lights = light_off, fs->total_groups = group_off;
  fs->no_packed = ctx->env_no_packed;
  fs->approx_shade = ctx->opt_approx_shade;
  fs->pool_sized = ctx->opt_pool_lazy; // (SRZ_OPT_POOL_LAZY: no first-render sizing — the pool only follows the previous renders' demand)

  // stage host copies (pinned not needed: one-time upload)
  fs->tris_aos = tris_aos && copy_tris;
  std::vector<srz_tri> h_tris(copy_tris ? (size_t)tri_off : 0);
  std::vector<float> h_pos(copy_tris && !fs->tris_aos ? (size_t)tri_off * TRI_POS_F : 0); // the dense copy of the positions
  std::vector<uint16_t> h_tb((size_t)tri_off);
  fs->h_lights.resize((size_t)light_off);
  for (int f = 0; f < n_frames; ++f) {
    const srz_frame &fr = frames[f];
    const FrameDesc &d = fs->h_frames[f];
    size_t o = d.tri_off;
    for (uint32_t b = 0; b < fr.n_batches; ++b) {
      const srz_batch &sb = fr.batches[b];
      if (copy_tris && sb.n_tris) {
        std::memcpy(&h_tris[o], sb.tris, sizeof(srz_tri) * sb.n_tris);
        if (!h_pos.empty())
          for (size_t t = 0; t < sb.n_tris; ++t) std::memcpy(&h_pos[(o + t) * TRI_POS_F], &sb.tris[t].pos[0][0], sizeof(float) * TRI_POS_F);
      }
      std::fill(h_tb.begin() + o, h_tb.begin() + o + sb.n_tris, (uint16_t)b);
      o += sb.n_tris;
    }
    if (fr.n_lights) std::memcpy(&fs->h_lights[d.light_off], fr.lights, sizeof(srz_light) * fr.n_lights);
  }
  classify_frames(fs);
  if (draws) {
    fs->h_draws = *draws, fs->n_draws = (uint32_t)draws->size();
    for (const DrawDesc &dd : *draws) fs->max_faces = std::max(fs->max_faces, dd.n_faces);
  }
  // [FrameDesc x n | lights | DrawDesc x draws], 16-byte aligned parts
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  fs->dyn_lights_off = up16(sizeof(FrameDesc) * (size_t)n_frames);
  fs->dyn_draws_off = up16(fs->dyn_lights_off + sizeof(srz_light) * (size_t)light_off);
  fs->dyn_bytes = fs->dyn_draws_off + sizeof(DrawDesc) * fs->h_draws.size();
  auto dev_alloc = [&](void **p, size_t bytes) { return hipMalloc(p, std::max<size_t>(bytes, 256)); };
  hipError_t e = hipSuccess;
#define FS_TRY(expr)                                                                                                   \
  if (e == hipSuccess) e = (expr)
  FS_TRY(dev_alloc((void **)&fs->d_dyn, fs->dyn_bytes));
  if (e == hipSuccess) {
    fs->d_frames = reinterpret_cast<FrameDesc *>(fs->d_dyn);
    fs->d_lights = reinterpret_cast<srz_light *>(fs->d_dyn + fs->dyn_lights_off);
    if (draws) fs->d_draws = reinterpret_cast<DrawDesc *>(fs->d_dyn + fs->dyn_draws_off);
  }
  FS_TRY(dev_alloc((void **)&fs->d_tris, sizeof(srz_tri) * tri_off));
  if (!fs->tris_aos) FS_TRY(dev_alloc((void **)&fs->d_tri_pos, sizeof(float) * TRI_POS_F * tri_off + 16)); // (+16: slack behind the last triangle's 9 floats, which are read as three 12-byte pieces)
  FS_TRY(dev_alloc((void **)&fs->d_bbox, sizeof(BBox) * tri_off));
  FS_TRY(dev_alloc((void **)&fs->d_chunk_rows, sizeof(uint32_t) * (tri_off / 64 + (size_t)n_frames + 1)));
  FS_TRY(dev_alloc((void **)&fs->d_band_desc, sizeof(uint32_t) * group_off * fs->n_local_bands));
  FS_TRY(dev_alloc((void **)&fs->d_band_ent, sizeof(uint2) * group_off * ENT_PER_GROUP));
  FS_TRY(dev_alloc((void **)&fs->d_tri_batch, sizeof(uint16_t) * tri_off));
  fs->max_tiles = (uint32_t)n_frames * fs->n_local_bands * fs->tiles_x;
  {  // record pool: one sub-pool per ~128 binning workgroups (their bump allocators are single addresses); first guess
     // 4 records per triangle — the renders' own demand corrects it (render_impl)
    const uint64_t n_wgs = (uint64_t)((n_frames + 7) / 8 * 8) * fs->n_local_bands;
    uint32_t n_sub = 1;
    while (n_sub < 64u && (uint64_t)n_sub * 256u <= n_wgs) n_sub *= 2u;
    fs->pool_n_sub = n_sub;
    const uint64_t cap = std::min<uint64_t>((4ull * tri_off + 4096u) / n_sub + 64u, 0xfffffff0ull / n_sub);
    fs->pool_sub_cap = (uint32_t)cap;
    FS_TRY(dev_alloc((void **)&fs->d_pool, sizeof(uint32_t) * cap * n_sub));
    FS_TRY(dev_alloc((void **)&fs->d_pool_heads, sizeof(uint32_t) * CNT_STRIDE * 64)); // (one cache line per allocator)
    // what a render asked of each sub-pool comes back through pinned, device-mapped host memory: small jobs store it from
    // k_raster's first workgroup (no copy, no event, no query on the launch path), batches copy it on the clear's side stream
    FS_TRY(hipHostMalloc((void **)&fs->h_pool_heads, sizeof(uint32_t) * CNT_STRIDE * 64 * srz_frameset::DEMAND_PARTS, hipHostMallocMapped | hipHostMallocCoherent));
    if (e == hipSuccess) std::memset(fs->h_pool_heads, 0, sizeof(uint32_t) * CNT_STRIDE * 64 * srz_frameset::DEMAND_PARTS);
    // the measurement of the side clear's grid (srz_frameset::ClearTune): device-side state, and the word its decision arrives in
    FS_TRY(dev_alloc((void **)&fs->clear_tune.d_ctl, sizeof(ClearCtl)));
    if (e == hipSuccess) FS_TRY(hipMemset(fs->clear_tune.d_ctl, 0, sizeof(ClearCtl)));
    FS_TRY(hipHostMalloc((void **)&fs->clear_tune.h_wgs, 64, hipHostMallocMapped | hipHostMallocCoherent));
    if (e == hipSuccess) *fs->clear_tune.h_wgs = 0u;
    FS_TRY(dev_alloc((void **)&fs->d_tile_info, sizeof(uint2) * fs->max_tiles));
    FS_TRY(dev_alloc((void **)&fs->d_slow_list, sizeof(uint32_t) * fs->max_tiles));
    FS_TRY(dev_alloc((void **)&fs->d_slow_count, 2 * sizeof(uint32_t)));
    FS_TRY(dev_alloc((void **)&fs->d_redo_list, sizeof(uint4) * fs->max_tiles));
  }
  FS_TRY(dev_alloc((void **)&fs->d_vis, sizeof(uint32_t) * (size_t)fs->max_tiles * ((size_t)TILE * TILE)));
  FS_TRY(ensure_worklists(fs)); // (8 lists per build kind the classified frames need: not all 104)
  FS_TRY(dev_alloc((void **)&fs->d_work_count, sizeof(uint32_t) * CNT_STRIDE * N_WORK_LISTS));
  FS_TRY(dev_alloc((void **)&fs->d_sdesc, sizeof(ShadeDescG) * fs->h_batches.size()));
  std::vector<uint8_t> h_dyn(fs->dyn_bytes);
  stage_dyn(fs, h_dyn.data());
  FS_TRY(hipMemcpy(fs->d_dyn, h_dyn.data(), fs->dyn_bytes, hipMemcpyHostToDevice));
  if (tri_off) {
    if (copy_tris) FS_TRY(hipMemcpy(fs->d_tris, h_tris.data(), sizeof(srz_tri) * tri_off, hipMemcpyHostToDevice));
    if (!h_pos.empty()) FS_TRY(hipMemcpy(fs->d_tri_pos, h_pos.data(), sizeof(float) * h_pos.size(), hipMemcpyHostToDevice));
    FS_TRY(hipMemcpy(fs->d_tri_batch, h_tb.data(), sizeof(uint16_t) * tri_off, hipMemcpyHostToDevice));
  }
#undef FS_TRY
  if (e != hipSuccess) {
    free_frameset_buffers(fs);
    delete fs;
    return fail(ctx, e == hipErrorOutOfMemory ? SRZ_E_NOMEM : SRZ_E_NODEVICE,
                std::string("srz_frameset_create: ") + hipGetErrorString(e));
  }
  *out = fs;
  return SRZ_OK;
}

// A set made through the public entry points sizes its tile-list pool NOW (creation is synchronous anyway: it uploads), by a binning
// pass of its own, so that every srz_frameset_render — the first included — is asynchronous on its stream.  (The ctx's internal
// one-frame sets of srz_draw / srz_draw_scene are rendered at once: their first render does the sizing.)
static int size_pool_at_create(srz_ctx *ctx, srz_frameset **out) {
  srz_frameset *fs = *out;
  if (fs->pool_sized) return SRZ_OK; // SRZ_OPT_POOL_LAZY
  int rc = render_impl(ctx, fs, nullptr, 0, ctx->stream, Pass::size_only());
  if (rc == SRZ_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, SRZ_E_NODEVICE, "srz_frameset_create: the binning pass failed");
  if (rc != SRZ_OK) {
    srz_frameset_destroy(ctx, fs);
    *out = nullptr;
  }
  return rc;
}

int srz_frameset_create(srz_ctx *ctx, const srz_frame *frames, int n_frames, srz_frameset **out) {
  int rc = build_frameset(ctx, frames, n_frames, out, true);
  return rc == SRZ_OK ? size_pool_at_create(ctx, out) : rc;
}

int srz_mesh_upload(srz_ctx *ctx, int mesh_id, const srz_vertex *verts, uint32_t n_verts, const uint32_t *faces, uint32_t n_faces) {
  if (!ctx) return SRZ_E_INVALID;
  if (mesh_id < 0 || mesh_id >= MAX_MESH || !verts || !faces || n_verts == 0) return fail(ctx, SRZ_E_INVALID, "srz_mesh_upload: bad arguments");
  for (uint32_t i = 0; i < 3u * n_faces; ++i)
    if (faces[i] >= n_verts) return fail(ctx, SRZ_E_INVALID, "srz_mesh_upload: face index out of range");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the corner lists, by a counting sort on the vertex: stable, so a vertex's corners come in increasing order of 3 * face + k
  std::vector<uint32_t> lists((size_t)n_verts + 1 + 3 * (size_t)n_faces, 0u);
  uint32_t *off = lists.data(), *corners = off + n_verts + 1;
  for (uint32_t i = 0; i < 3u * n_faces; ++i) ++off[faces[i] + 1];
  for (uint32_t v = 0; v < n_verts; ++v) off[v + 1] += off[v];
  {
    std::vector<uint32_t> at(off, off + n_verts);
    for (uint32_t i = 0; i < 3u * n_faces; ++i) corners[at[faces[i]]++] = i;
  }
  srz_ctx::MeshSlot m;
  HIP_TRY(ctx, hipMalloc(&m.d_verts, sizeof(srz_vertex) * n_verts));
  hipError_t e = hipMalloc(&m.d_faces, sizeof(uint32_t) * 3 * (n_faces ? n_faces : 1));
  if (e == hipSuccess) e = hipMalloc(&m.d_corner_off, sizeof(uint32_t) * lists.size());
  if (e == hipSuccess) e = hipMemcpy(m.d_verts, verts, sizeof(srz_vertex) * n_verts, hipMemcpyHostToDevice);
  if (e == hipSuccess && n_faces) e = hipMemcpy(m.d_faces, faces, sizeof(uint32_t) * 3 * n_faces, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m.d_corner_off, lists.data(), sizeof(uint32_t) * lists.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(m.d_verts), (void)hipFree(m.d_faces), (void)hipFree(m.d_corner_off);
    return fail(ctx, SRZ_E_NOMEM, std::string("srz_mesh_upload: ") + hipGetErrorString(e));
  }
  m.n_verts = n_verts, m.n_faces = n_faces, m.upload = ++ctx->mesh_uploads;
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(ctx->mesh[mesh_id].d_verts), (void)hipFree(ctx->mesh[mesh_id].d_faces), (void)hipFree(ctx->mesh[mesh_id].d_corner_off);
  ctx->mesh[mesh_id] = m;
  return SRZ_OK;
}

int srz_mesh_update(srz_ctx *ctx, int mesh_id, const srz_vertex *d_verts, uint32_t n_verts, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_mesh_update");
  if (mesh_id < 0 || mesh_id >= MAX_MESH || !ctx->mesh[mesh_id].d_verts) return fail(ctx, SRZ_E_INVALID, fn + ": no mesh in that slot");
  if (!d_verts) return fail(ctx, SRZ_E_INVALID, fn + ": null vertices");
  const srz_ctx::MeshSlot &m = ctx->mesh[mesh_id];
  if (n_verts != m.n_verts) return fail(ctx, SRZ_E_INVALID, fn + ": n_verts is not the slot's vertex count");
  if (!aligned<4>({d_verts})) return fail(ctx, SRZ_E_INVALID, fn + ": the vertices must be 4-byte aligned");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // (the slot's own buffer, its address, the faces, the corner lists and the upload counter stay: every sceneset that draws the slot
  // remains valid and transforms the new vertices at its next vertex stage)
  HIP_TRY(ctx, hipMemcpyAsync(m.d_verts, d_verts, sizeof(srz_vertex) * n_verts, hipMemcpyDeviceToDevice, pick_stream(ctx, stream)));
  return SRZ_OK;
}

// What srz_mesh_normals and srz_mesh_normals_grad check alike; on success the slot's lists and the resolved positions are in `a`
// (a null d_pos: the slot's own records) and *pos_span is the bytes the positions reach over.
static int check_mesh_normals(srz_ctx *ctx, const std::string &fn, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets,
                              MeshNormalsArgs &a, size_t *pos_span) {
  if (mesh_id < 0 || mesh_id >= MAX_MESH || !ctx->mesh[mesh_id].d_verts) return fail(ctx, SRZ_E_INVALID, fn + ": no mesh in that slot");
  const srz_ctx::MeshSlot &m = ctx->mesh[mesh_id];
  if (n_sets == 0u || n_sets > 65535u) return fail(ctx, SRZ_E_INVALID, fn + ": n_sets must be 1 .. 65535");
  if (!d_pos && n_sets != 1u) return fail(ctx, SRZ_E_INVALID, fn + ": the slot's own vertices are one set (n_sets must be 1)");
  if (d_pos && pos_stride < 3u) return fail(ctx, SRZ_E_INVALID, fn + ": pos_stride must be at least 3");
  a.pos = d_pos ? d_pos : reinterpret_cast<const float *>(m.d_verts), a.pos_stride = d_pos ? pos_stride : 8u;
  a.faces = m.d_faces, a.corner_off = m.d_corner_off, a.corners = m.d_corner_off + m.n_verts + 1;
  a.n_verts = m.n_verts, a.n_sets = n_sets;
  *pos_span = (((size_t)n_sets * m.n_verts - 1u) * a.pos_stride + 3u) * sizeof(float);
  return SRZ_OK;
}

int srz_mesh_normals(srz_ctx *ctx, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, float *d_nrm, uint32_t nrm_stride,
                     void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_mesh_normals");
  MeshNormalsArgs a{};
  size_t pos_span = 0;
  if (int rc = check_mesh_normals(ctx, fn, mesh_id, d_pos, pos_stride, n_sets, a, &pos_span)) return rc;
  if (!d_nrm && n_sets != 1u) return fail(ctx, SRZ_E_INVALID, fn + ": the slot's own normals are one set (n_sets must be 1)");
  if (d_nrm && nrm_stride < 3u) return fail(ctx, SRZ_E_INVALID, fn + ": nrm_stride must be at least 3");
  if (!aligned<4>({d_pos, d_nrm})) return fail(ctx, SRZ_E_INVALID, fn + ": the buffers must be 4-byte aligned");
  a.nrm = d_nrm ? d_nrm : reinterpret_cast<float *>(ctx->mesh[mesh_id].d_verts) + 3, a.nrm_stride = d_nrm ? nrm_stride : 8u;
  const size_t nrm_span = (((size_t)n_sets * a.n_verts - 1u) * a.nrm_stride + 3u) * sizeof(float);
  // (the one overlap that is none: records whose floats 3..5 are the normals of their floats 0..2 — the slot's own layout)
  const bool records = a.nrm == a.pos + 3 && a.nrm_stride == a.pos_stride && a.pos_stride >= 6u;
  if (!records && ranges_overlap({a.nrm, nrm_span}, {a.pos, pos_span})) return fail(ctx, SRZ_E_INVALID, fn + ": the normals overlap the positions");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  launch_mesh_normals(a, pick_stream(ctx, stream));
  HIP_TRY(ctx, hipGetLastError());
  return SRZ_OK;
}

int srz_mesh_normals_grad(srz_ctx *ctx, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, const float *d_gnrm,
                          uint32_t gnrm_stride, float *d_work, float *d_gpos, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_mesh_normals_grad");
  MeshNormalsArgs a{};
  size_t pos_span = 0;
  if (int rc = check_mesh_normals(ctx, fn, mesh_id, d_pos, pos_stride, n_sets, a, &pos_span)) return rc;
  if (!d_gnrm || !d_work || !d_gpos) return fail(ctx, SRZ_E_INVALID, fn + ": null normal gradient / workspace / output");
  if (gnrm_stride < 3u) return fail(ctx, SRZ_E_INVALID, fn + ": gnrm_stride must be at least 3");
  if (!aligned<4>({d_pos, d_gnrm, d_work, d_gpos})) return fail(ctx, SRZ_E_INVALID, fn + ": the buffers must be 4-byte aligned");
  const size_t packed = (size_t)n_sets * a.n_verts * 3u * sizeof(float);
  const size_t gnrm_span = (((size_t)n_sets * a.n_verts - 1u) * gnrm_stride + 3u) * sizeof(float);
  if (int rc = check_grad_overlap(ctx, fn, {{d_work, packed}, {d_gpos, packed}}, {{a.pos, pos_span}, {d_gnrm, gnrm_span}})) return rc;
  a.gnrm = d_gnrm, a.gnrm_stride = gnrm_stride, a.work = d_work, a.gpos = d_gpos;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  launch_mesh_normals_grad(a, pick_stream(ctx, stream));
  HIP_TRY(ctx, hipGetLastError());
  return SRZ_OK;
}

// What srz_mesh_tangents and srz_mesh_tangents_grad check alike (check_mesh_normals, and the uv set); on success the slot's lists and
// the resolved positions and uv are in `a`, *pos_span and *uv_span the bytes they reach over.
static int check_mesh_tangents(srz_ctx *ctx, const std::string &fn, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets,
                               const float *d_uv, uint32_t uv_stride, MeshTangentsArgs &a, size_t *pos_span, size_t *uv_span) {
  MeshNormalsArgs n{};
  if (int rc = check_mesh_normals(ctx, fn, mesh_id, d_pos, pos_stride, n_sets, n, pos_span)) return rc;
  if (d_uv && uv_stride < 2u) return fail(ctx, SRZ_E_INVALID, fn + ": uv_stride must be at least 2");
  a.pos = n.pos, a.pos_stride = n.pos_stride, a.faces = n.faces, a.corner_off = n.corner_off, a.corners = n.corners;
  a.n_verts = n.n_verts, a.n_sets = n.n_sets;
  a.uv = d_uv ? d_uv : reinterpret_cast<const float *>(ctx->mesh[mesh_id].d_verts) + 6, a.uv_stride = d_uv ? uv_stride : 8u;
  *uv_span = (((size_t)a.n_verts - 1u) * a.uv_stride + 2u) * sizeof(float);
  return SRZ_OK;
}

int srz_mesh_tangents(srz_ctx *ctx, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, const float *d_uv,
                      uint32_t uv_stride, float *d_tan, uint32_t tan_stride, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_mesh_tangents");
  MeshTangentsArgs a{};
  size_t pos_span = 0, uv_span = 0;
  if (int rc = check_mesh_tangents(ctx, fn, mesh_id, d_pos, pos_stride, n_sets, d_uv, uv_stride, a, &pos_span, &uv_span)) return rc;
  if (!d_tan) return fail(ctx, SRZ_E_INVALID, fn + ": null d_tan (a vertex record has no tangent field)");
  if (tan_stride < 4u) return fail(ctx, SRZ_E_INVALID, fn + ": tan_stride must be at least 4");
  if (!aligned<4>({d_pos, d_uv, d_tan})) return fail(ctx, SRZ_E_INVALID, fn + ": the buffers must be 4-byte aligned");
  const size_t tan_span = (((size_t)n_sets * a.n_verts - 1u) * tan_stride + 4u) * sizeof(float);
  if (ranges_overlap({d_tan, tan_span}, {a.pos, pos_span}) || ranges_overlap({d_tan, tan_span}, {a.uv, uv_span}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the tangents overlap the positions or the uv");
  a.tan = d_tan, a.tan_stride = tan_stride;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  launch_mesh_tangents(a, pick_stream(ctx, stream));
  HIP_TRY(ctx, hipGetLastError());
  return SRZ_OK;
}

int srz_mesh_tangents_grad(srz_ctx *ctx, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, const float *d_uv,
                           uint32_t uv_stride, const float *d_gtan, uint32_t gtan_stride, float *d_work, float *d_gpos, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_mesh_tangents_grad");
  MeshTangentsArgs a{};
  size_t pos_span = 0, uv_span = 0;
  if (int rc = check_mesh_tangents(ctx, fn, mesh_id, d_pos, pos_stride, n_sets, d_uv, uv_stride, a, &pos_span, &uv_span)) return rc;
  if (!d_gtan || !d_work || !d_gpos) return fail(ctx, SRZ_E_INVALID, fn + ": null tangent gradient / workspace / output");
  if (gtan_stride < 4u) return fail(ctx, SRZ_E_INVALID, fn + ": gtan_stride must be at least 4");
  if (!aligned<4>({d_pos, d_uv, d_gtan, d_work, d_gpos})) return fail(ctx, SRZ_E_INVALID, fn + ": the buffers must be 4-byte aligned");
  const size_t packed = (size_t)n_sets * a.n_verts * 3u * sizeof(float);
  const size_t gtan_span = (((size_t)n_sets * a.n_verts - 1u) * gtan_stride + 4u) * sizeof(float);
  if (int rc = check_overlaps(ctx, fn, {{d_work, packed}, {d_gpos, packed}}, {{a.pos, pos_span}, {a.uv, uv_span}, {d_gtan, gtan_span}}))
    return rc;
  a.gtan = d_gtan, a.gtan_stride = gtan_stride, a.work = d_work, a.gpos = d_gpos;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  launch_mesh_tangents_grad(a, pick_stream(ctx, stream));
  HIP_TRY(ctx, hipGetLastError());
  return SRZ_OK;
}

// srz_mesh_laplacian and srz_mesh_laplacian_grad: one set of checks and one launch — the backward is the operator's transpose over
// d_gout, laid out like the forward's d_x (only the forward has the null form: the slot's own positions).
static int mesh_laplacian(srz_ctx *ctx, const std::string &fn, bool grad, int mesh_id, const float *d_x, uint32_t x_stride, uint32_t n_ch,
                          uint32_t n_sets, int kind, const float *d_wpos, uint32_t wpos_stride, float *d_out, uint32_t out_stride, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  if (mesh_id < 0 || mesh_id >= MAX_MESH || !ctx->mesh[mesh_id].d_verts) return fail(ctx, SRZ_E_INVALID, fn + ": no mesh in that slot");
  const srz_ctx::MeshSlot &m = ctx->mesh[mesh_id];
  if (n_sets == 0u || n_sets > 65535u) return fail(ctx, SRZ_E_INVALID, fn + ": n_sets must be 1 .. 65535");
  if (n_ch == 0u || n_ch > 64u) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. 64");
  if (kind != SRZ_LAP_UMBRELLA && kind != SRZ_LAP_GRAPH && kind != SRZ_LAP_COTAN) return fail(ctx, SRZ_E_INVALID, fn + ": unknown kind");
  if (!d_x && grad) return fail(ctx, SRZ_E_INVALID, fn + ": null d_gout");
  if (!d_x && (n_ch != 3u || n_sets != 1u))
    return fail(ctx, SRZ_E_INVALID, fn + ": the slot's own positions are one set of three channels (n_ch must be 3, n_sets 1)");
  if (!d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null output");
  if ((d_x && x_stride < n_ch) || out_stride < n_ch) return fail(ctx, SRZ_E_INVALID, fn + ": a stride is below n_ch");
  if (d_wpos && wpos_stride < 3u) return fail(ctx, SRZ_E_INVALID, fn + ": wpos_stride must be at least 3");
  if (!aligned<4>({d_x, d_wpos, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": the buffers must be 4-byte aligned");
  MeshLaplacianArgs a{};
  const float *own = reinterpret_cast<const float *>(m.d_verts);
  a.x = d_x ? d_x : own, a.x_stride = d_x ? x_stride : 8u;
  a.wpos = d_wpos ? d_wpos : own, a.wpos_stride = d_wpos ? wpos_stride : 8u;
  a.faces = m.d_faces, a.corner_off = m.d_corner_off, a.corners = m.d_corner_off + m.n_verts + 1;
  a.out = d_out, a.out_stride = out_stride, a.n_ch = n_ch, a.n_verts = m.n_verts, a.n_sets = n_sets;
  const size_t last = (size_t)n_sets * m.n_verts - 1u;
  const Range x_span{a.x, (last * a.x_stride + n_ch) * sizeof(float)}, out_span{d_out, (last * out_stride + n_ch) * sizeof(float)};
  const Range wpos_span{a.wpos, (((size_t)m.n_verts - 1u) * a.wpos_stride + 3u) * sizeof(float)};
  // (no in-place record form: the pass reads its neighbours' inputs, so an output inside the input's span is a race)
  if (ranges_overlap(out_span, x_span)) return fail(ctx, SRZ_E_INVALID, fn + ": the output overlaps the input");
  if (kind == SRZ_LAP_COTAN && ranges_overlap(out_span, wpos_span)) return fail(ctx, SRZ_E_INVALID, fn + ": the output overlaps the weight positions");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  launch_mesh_laplacian(a, kind, grad, pick_stream(ctx, stream));
  HIP_TRY(ctx, hipGetLastError());
  return SRZ_OK;
}

int srz_mesh_laplacian(srz_ctx *ctx, int mesh_id, const float *d_x, uint32_t x_stride, uint32_t n_ch, uint32_t n_sets, int kind,
                       const float *d_wpos, uint32_t wpos_stride, float *d_out, uint32_t out_stride, void *stream) {
  return mesh_laplacian(ctx, "srz_mesh_laplacian", false, mesh_id, d_x, x_stride, n_ch, n_sets, kind, d_wpos, wpos_stride, d_out, out_stride, stream);
}

int srz_mesh_laplacian_grad(srz_ctx *ctx, int mesh_id, const float *d_gout, uint32_t gout_stride, uint32_t n_ch, uint32_t n_sets, int kind,
                            const float *d_wpos, uint32_t wpos_stride, float *d_gx, uint32_t gx_stride, void *stream) {
  return mesh_laplacian(ctx, "srz_mesh_laplacian_grad", true, mesh_id, d_gout, gout_stride, n_ch, n_sets, kind, d_wpos, wpos_stride, d_gx, gx_stride,
                        stream);
}

// srz_mesh_edges and srz_mesh_edges_grad: check_mesh_normals for the slot and the positions, then the pass's own buffers.  A face
// field of a slot with no faces reaches over nothing (a null Range overlaps nothing).
static int mesh_edges(srz_ctx *ctx, const std::string &fn, bool grad, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, int kind,
                      const float *d_gout, float *d_out, uint32_t stride, float *d_work, float *d_gpos, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  MeshNormalsArgs n{};
  size_t pos_span = 0;
  if (int rc = check_mesh_normals(ctx, fn, mesh_id, d_pos, pos_stride, n_sets, n, &pos_span)) return rc;
  const uint32_t n_faces = ctx->mesh[mesh_id].n_faces;
  if (kind != SRZ_EDGE_COUNT && kind != SRZ_EDGE_LENGTH && kind != SRZ_EDGE_DIHEDRAL) return fail(ctx, SRZ_E_INVALID, fn + ": unknown kind");
  if (grad && kind == SRZ_EDGE_COUNT) return fail(ctx, SRZ_E_INVALID, fn + ": SRZ_EDGE_COUNT has no backward");
  if (kind == SRZ_EDGE_COUNT && n_sets != 1u) return fail(ctx, SRZ_E_INVALID, fn + ": SRZ_EDGE_COUNT reads no positions (n_sets must be 1)");
  if (grad ? !d_gout || !d_gpos : !d_out) return fail(ctx, SRZ_E_INVALID, fn + (grad ? ": null output gradient / output" : ": null output"));
  if (grad && kind == SRZ_EDGE_DIHEDRAL && !d_work) return fail(ctx, SRZ_E_INVALID, fn + ": SRZ_EDGE_DIHEDRAL needs a workspace");
  if (stride < 3u) return fail(ctx, SRZ_E_INVALID, fn + (grad ? ": gout_stride must be at least 3" : ": out_stride must be at least 3"));
  if (!aligned<4>({d_pos, d_gout, d_out, d_work, d_gpos})) return fail(ctx, SRZ_E_INVALID, fn + ": the buffers must be 4-byte aligned");
  const size_t field_span = n_faces ? (((size_t)n_sets * n_faces - 1u) * stride + 3u) * sizeof(float) : 0u;
  const Range pos{n.pos, pos_span}, field{n_faces ? (grad ? (const void *)d_gout : (const void *)d_out) : nullptr, field_span};
  if (!grad) {
    if (ranges_overlap(field, pos)) return fail(ctx, SRZ_E_INVALID, fn + ": the output overlaps the positions");
  } else {
    const bool dihedral = kind == SRZ_EDGE_DIHEDRAL; // (LENGTH neither reads nor writes d_work)
    const Range work{dihedral && n_faces ? d_work : nullptr, (size_t)n_sets * n_faces * 3u * sizeof(float)};
    if (int rc = check_grad_overlap(ctx, fn, {work, {d_gpos, (size_t)n_sets * n.n_verts * 3u * sizeof(float)}}, {pos, field})) return rc;
  }
  MeshEdgesArgs a{};
  a.pos = n.pos, a.pos_stride = n.pos_stride, a.faces = n.faces, a.corner_off = n.corner_off, a.corners = n.corners;
  a.out = d_out, a.out_stride = stride, a.gout = d_gout, a.gout_stride = stride, a.work = d_work, a.gpos = d_gpos;
  a.n_verts = n.n_verts, a.n_faces = n_faces, a.n_sets = n_sets;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (grad) launch_mesh_edges_grad(a, kind, pick_stream(ctx, stream));
  else launch_mesh_edges(a, kind, pick_stream(ctx, stream));
  HIP_TRY(ctx, hipGetLastError());
  return SRZ_OK;
}

int srz_mesh_edges(srz_ctx *ctx, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, int kind, float *d_out,
                   uint32_t out_stride, void *stream) {
  return mesh_edges(ctx, "srz_mesh_edges", false, mesh_id, d_pos, pos_stride, n_sets, kind, nullptr, d_out, out_stride, nullptr, nullptr, stream);
}

int srz_mesh_edges_grad(srz_ctx *ctx, int mesh_id, const float *d_pos, uint32_t pos_stride, uint32_t n_sets, int kind,
                        const float *d_gout, uint32_t gout_stride, float *d_work, float *d_gpos, void *stream) {
  return mesh_edges(ctx, "srz_mesh_edges_grad", true, mesh_id, d_pos, pos_stride, n_sets, kind, d_gout, nullptr, gout_stride, d_work, d_gpos, stream);
}

// A sceneset's frames as srz_frames whose batches carry sizes only (k_vertex makes the triangles): fr[f], its batches in `batches`.
// Every draw names an uploaded mesh (the callers have checked).
static void scene_frames(const srz_ctx *ctx, const srz_scene_frame *frames, int n_frames, std::vector<srz_frame> &fr, std::vector<srz_batch> &batches) {
  size_t n = 0;
  for (int f = 0; f < n_frames; ++f) n += frames[f].n_draws;
  fr.assign((size_t)n_frames, srz_frame{}), batches.assign(n, srz_batch{});
  srz_batch *b = batches.data();
  for (int f = 0; f < n_frames; ++f) {
    const srz_scene_frame &sf = frames[f];
    srz_frame &o = fr[f];
    o.width = sf.width, o.height = sf.height;
    std::memcpy(o.eye, sf.eye, sizeof o.eye), std::memcpy(o.ka, sf.ka, sizeof o.ka), std::memcpy(o.ks, sf.ks, sizeof o.ks);
    o.p = sf.p, o.kh = sf.kh, o.kn = sf.kn;
    o.n_lights = sf.n_lights, o.lights = sf.lights;
    o.n_batches = sf.n_draws, o.batches = b;
    o.flags = sf.flags;
    for (uint32_t d = 0; d < sf.n_draws; ++d, ++b)
      b->shader = sf.draws[d].shader, b->tex_id = sf.draws[d].tex_id, b->n_tris = ctx->mesh[sf.draws[d].mesh_id].n_faces;
  }
}
// what a draw's vertex stage takes of the call: the frame's depth mapping and the draw's matrices
static void set_draw(DrawDesc &dd, const srz_scene_frame &sf, const srz_mesh_draw &dr) {
  dd.zscale = sf.zscale, dd.zoffset = sf.zoffset;
  std::memcpy(dd.ndc_mvp, dr.ndc_mvp, sizeof dd.ndc_mvp), std::memcpy(dd.normal_m, dr.normal_m, sizeof dd.normal_m);
}

static int refresh_frames(srz_ctx *ctx, srz_frameset *fs, const srz_frame *frames, int n_frames, const char *who, bool copy_tris);
static int sceneset_create_impl(srz_ctx *ctx, const srz_scene_frame *frames, int n_frames, srz_frameset **out, bool size_pool);
int srz_sceneset_create(srz_ctx *ctx, const srz_scene_frame *frames, int n_frames, srz_frameset **out) {
  return sceneset_create_impl(ctx, frames, n_frames, out, /*size_pool=*/true);
}
// (size_pool = false: srz_draw_scene's internal one-frame set — rendered at once, its first render sizes the pool: no second binning
// pass, no extra synchronisation per signature change)
static int sceneset_create_impl(srz_ctx *ctx, const srz_scene_frame *frames, int n_frames, srz_frameset **out, bool size_pool) {
  if (!ctx) return SRZ_E_INVALID;
  if (!out) return fail(ctx, SRZ_E_INVALID, "srz_sceneset_create: out is NULL");
  *out = nullptr;
  if (!frames || n_frames <= 0) return fail(ctx, SRZ_E_INVALID, "srz_sceneset_create: no frames");
  std::vector<DrawDesc> draws;
  std::vector<int> draw_mesh;
  std::vector<uint64_t> draw_upload;
  uint32_t first = 0; // (a draw's first triangle: the set's triangles are its frames' draws in order)
  for (int f = 0; f < n_frames; ++f) {
    const srz_scene_frame &sf = frames[f];
    if (sf.n_draws && !sf.draws) return fail(ctx, SRZ_E_INVALID, "srz_sceneset_create: null draws");
    for (uint32_t d = 0; d < sf.n_draws; ++d) {
      const srz_mesh_draw &dr = sf.draws[d];
      if (dr.mesh_id < 0 || dr.mesh_id >= MAX_MESH || !ctx->mesh[dr.mesh_id].d_verts)
        return fail(ctx, SRZ_E_INVALID, "srz_sceneset_create: draw names a mesh slot that was never uploaded");
      const srz_ctx::MeshSlot &m = ctx->mesh[dr.mesh_id];
      DrawDesc dd{};
      dd.verts = m.d_verts, dd.faces = m.d_faces, dd.n_faces = m.n_faces, dd.tri_off = first, dd.frame = (uint32_t)f;
      set_draw(dd, sf, dr);
      draws.push_back(dd), draw_mesh.push_back(dr.mesh_id), draw_upload.push_back(m.upload);
      first += m.n_faces;
    }
  }
  std::vector<srz_frame> fr;
  std::vector<srz_batch> batches;
  scene_frames(ctx, frames, n_frames, fr, batches);
  srz_frameset *fs = nullptr;
  int rc = build_frameset(ctx, fr.data(), n_frames, &fs, false, false, &draws);
  if (rc) return rc;
  fs->h_draw_mesh = draw_mesh, fs->h_draw_upload = draw_upload;
  *out = fs;
  return size_pool ? size_pool_at_create(ctx, out) : SRZ_OK; // (with the matrices of creation: a later srz_sceneset_update is followed by the lazy growth)
}

int srz_sceneset_update(srz_ctx *ctx, srz_frameset *fs, const srz_scene_frame *frames, int n_frames) {
  if (!ctx) return SRZ_E_INVALID;
  if (!fs || !frames || !fs->d_draws) return fail(ctx, SRZ_E_INVALID, "srz_sceneset_update: not a sceneset");
  if (n_frames != fs->n_frames) return fail(ctx, SRZ_E_INVALID, "srz_sceneset_update: frame count changed");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (int f = 0, di = 0; f < n_frames; ++f) { // the mesh bindings (the frame path checks the rest)
    const srz_scene_frame &sf = frames[f];
    const FrameDesc &d = fs->h_frames[f];
    if (sf.width != fs->width || sf.height != fs->height || sf.n_lights != d.n_lights || sf.n_draws != d.n_batches ||
        (sf.n_lights && !sf.lights) || (sf.n_draws && !sf.draws))
      return fail(ctx, SRZ_E_INVALID, "srz_sceneset_update: structure changed");
    for (uint32_t k = 0; k < sf.n_draws; ++k, ++di) {
      const srz_mesh_draw &dr = sf.draws[k];
      // (the slot must still hold the upload the set's draws point into: comparing the buffers' addresses would accept a slot
      // uploaded twice since, whose new vertex buffer got the old one's address back while the face buffer did not)
      if (dr.mesh_id != fs->h_draw_mesh[di] || dr.mesh_id < 0 || dr.mesh_id >= MAX_MESH ||
          ctx->mesh[dr.mesh_id].n_faces != fs->h_draws[di].n_faces || ctx->mesh[dr.mesh_id].upload != fs->h_draw_upload[di])
        return fail(ctx, SRZ_E_INVALID, "srz_sceneset_update: mesh binding changed");
    }
  }
  for (int f = 0, di = 0; f < n_frames; ++f)
    for (uint32_t k = 0; k < frames[f].n_draws; ++k) set_draw(fs->h_draws[di++], frames[f], frames[f].draws[k]);
  std::vector<srz_frame> fr;
  std::vector<srz_batch> batches;
  scene_frames(ctx, frames, n_frames, fr, batches);
  return refresh_frames(ctx, fs, fr.data(), n_frames, "srz_sceneset_update", /*copy_tris=*/false);
}

int srz_target_create(srz_ctx *ctx, int width, int height, srz_target **out) {
  if (!ctx) return SRZ_E_INVALID;
  if (!out || width <= 0 || height <= 0 || width > 32767 || height > 32767) return fail(ctx, SRZ_E_INVALID, "srz_target_create: bad size");
  *out = nullptr;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  srz_target *t = new (std::nothrow) srz_target();
  if (!t) return fail(ctx, SRZ_E_NOMEM, "srz_target_create: out of host memory");
  t->width = width, t->height = height;
  const size_t plane = (size_t)width * height;
  hipError_t e = hipMalloc(&t->d_planes, plane * 16);
  if (e == hipSuccess) e = hipMalloc(&t->d_bgr8, plane * 3 + 16);
  if (e != hipSuccess) {
    (void)hipFree(t->d_planes), (void)hipFree(t->d_bgr8);
    delete t;
    return fail(ctx, SRZ_E_NOMEM, "srz_target_create: hipMalloc failed");
  }
  *out = t;
  return srz_target_clear(ctx, t, 1, 1);
}

void srz_target_destroy(srz_ctx *ctx, srz_target *t) {
  if (!t) return;
  if (ctx) (void)hipSetDevice(ctx->device), (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(t->d_planes), (void)hipFree(t->d_bgr8);
  delete t;
}

static int target_materialize_clear(srz_ctx *ctx, srz_target *t) {
  if (!t->pending_clear) return SRZ_OK;
  const size_t plane = (size_t)t->width * t->height;
  HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)t->d_planes, 0x7f800000, plane, ctx->stream)); // +inf
  HIP_TRY(ctx, hipMemsetAsync(t->d_planes + plane, 0, plane * 12, ctx->stream));
  t->pending_clear = false;
  return SRZ_OK;
}

int srz_target_clear(srz_ctx *ctx, srz_target *t, int color, int depth) {
  if (!ctx || !t) return SRZ_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t plane = (size_t)t->width * t->height;
  if (color && depth) {
    t->pending_clear = true; // free if a draw follows; materialised by the next read / partial clear otherwise
    return SRZ_OK;
  }
  if (!color && !depth) return SRZ_OK;
  int rc = target_materialize_clear(ctx, t);
  if (rc) return rc;
  if (depth) HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)t->d_planes, 0x7f800000, plane, ctx->stream));
  if (color) HIP_TRY(ctx, hipMemsetAsync(t->d_planes + plane, 0, plane * 12, ctx->stream));
  return SRZ_OK;
}

int srz_target_draw(srz_ctx *ctx, srz_target *t, int primitive, srz_frameset *fs, srz_stats *stats) {
  if (!ctx) return SRZ_E_INVALID;
  if (primitive != SRZ_PRIMITIVE_LINES && primitive != SRZ_PRIMITIVE_TRIANGLES)
    return fail(ctx, SRZ_E_PRIMITIVE, "Primitive Type is not supported!");
  if (!t || !fs) return fail(ctx, SRZ_E_INVALID, "srz_target_draw: null argument");
  if (fs->n_frames != 1 || fs->width != t->width || fs->height != t->height || fs->shard_world != 1)
    return fail(ctx, SRZ_E_INVALID, "srz_target_draw: needs an unsharded 1-frame set of the target's size");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t flags = t->pending_clear ? SRZ_FUSED_CLEAR : 0u;
  int rc = SRZ_OK;
  if (stats) rc = stats_pass(ctx, fs, t->pending_clear ? nullptr : t->d_planes, flags, ctx->stream, stats);
  if (rc == SRZ_OK) rc = render_impl(ctx, fs, t->d_planes, flags, ctx->stream, Pass::colour());
  if (rc == SRZ_OK) t->pending_clear = false; // (a failed draw leaves the pending clear(Color|Depth) in place)
  return rc;
}

int srz_target_read(srz_ctx *ctx, srz_target *t, float *z, float *c0, float *c1, float *c2) {
  if (!ctx || !t) return SRZ_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = target_materialize_clear(ctx, t);
  if (rc) return rc;
  const size_t plane = (size_t)t->width * t->height;
  float *host[4] = {z, c0, c1, c2};
  for (int p = 0; p < 4; ++p)
    if (host[p]) HIP_TRY(ctx, hipMemcpyAsync(host[p], t->d_planes + p * plane, plane * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return SRZ_OK;
}

int srz_target_read_bgr8(srz_ctx *ctx, srz_target *t, uint8_t *bgr8) {
  if (!ctx || !t || !bgr8) return SRZ_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = target_materialize_clear(ctx, t);
  if (rc) return rc;
  const size_t plane = (size_t)t->width * t->height;
  launch_resolve8(t->d_planes, t->d_bgr8, 1, (uint32_t)t->height, (uint32_t)t->width, 4ull * plane, ctx->stream);
  HIP_TRY(ctx, hipMemcpyAsync(bgr8, t->d_bgr8, plane * 3, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return SRZ_OK;
}

void srz_frameset_destroy(srz_ctx *ctx, srz_frameset *fs) {
  if (!fs) return;
  if (ctx) {
    // renders of this set may still be running on the ctx's stream, on the clear's side stream or on a stream the caller
    // passed to srz_frameset_render: wait for the whole device before its buffers (and the pinned demand words) go
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
  }
  free_frameset_buffers(fs);
  delete fs;
}

int srz_frameset_local_rows(const srz_ctx *ctx, const srz_frameset *fs) { return fs ? (int)fs->local_rows : SRZ_E_INVALID; }

size_t srz_frameset_out_bytes(const srz_ctx *ctx, const srz_frameset *fs) {
  return fs ? (size_t)fs->n_frames * 4u * fs->local_rows * (size_t)fs->width * sizeof(float) : 0;
}

int srz_frameset_render(srz_ctx *ctx, srz_frameset *fs, void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  return render_entry("srz_frameset_render", ctx, fs, d_out, out_bytes, flags, stream, Pass::colour());
}

int srz_frameset_render_visibility(srz_ctx *ctx, srz_frameset *fs, void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  return render_entry("srz_frameset_render_visibility", ctx, fs, d_out, out_bytes, flags, stream, Pass::visibility());
}

int srz_frameset_peel_visibility(srz_ctx *ctx, srz_frameset *fs, const void *d_prev, void *d_out, size_t out_bytes, uint32_t flags,
                                 void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_peel_visibility");
  if (!fs || !d_prev || !d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / previous layer / output");
  const size_t bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < bytes) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (!aligned<16>({d_prev, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": buffers must be 16-byte aligned");
  // (a tile's wave writes its pixels of d_out while other tiles' still read theirs of d_prev, and k_clear writes beside both)
  if (ranges_overlap({d_prev, bytes}, {d_out, bytes})) return fail(ctx, SRZ_E_INVALID, fn + ": the previous layer and the output overlap");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // every pixel's four words are written: a fused-clear render with k_peel in k_raster's place
  return render_impl(ctx, fs, (float *)d_out, (flags & FRAME_FLAGS) | SRZ_FUSED_CLEAR, pick_stream(ctx, stream),
                     Pass::peel(static_cast<const float *>(d_prev)));
}

int srz_frameset_shade_visibility(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, void *d_out, size_t out_bytes, uint32_t flags,
                                  void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_shade_visibility");
  if (!fs || !d_vis || !d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / output");
  const size_t bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < bytes) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (!aligned<16>({d_vis, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": buffers must be 16-byte aligned");
  // (this pass alone may run in place: a pixel's colour is written after its own visibility words were read, and nobody else's are)
  if (d_vis != d_out && ranges_overlap({d_vis, bytes}, {d_out, bytes}))
    return fail(ctx, SRZ_E_INVALID, fn + ": visibility buffer and output overlap partly");
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, PASS_SHADING | PASS_VERTEX, &s)) return rc;
  ShadeVisArgs a{};
  fill_walk(a, fs, d_vis, d_out);
  a.tris = fs->d_tris, a.tri_batch = fs->d_tri_batch, a.lights = fs->d_lights, a.sdesc = fs->d_sdesc;
  a.frame_stride = 4ull * plane_words(fs);
  a.flags_or = flags & FRAME_FLAGS, a.in_place = d_vis == d_out ? 1u : 0u;
  a.any_generic = fs->any_generic ? 1u : 0u;
  a.redo_list = reinterpret_cast<uint32_t *>(fs->d_redo_list), a.redo_count = fs->d_slow_count + 1; // (k_shade's: a render zeroes them itself)
  HIP_TRY(ctx, hipMemsetAsync(a.redo_count, 0, sizeof(uint32_t), s));
  launch_shade_vis(a, fs->fast_kinds, fs->any_generic, fs->approx_shade, s);
  // no sample of the side clear's grid measurement: while the set measures, its clock restarts here, so the next colour render times
  // only itself (as after a visibility render)
  const srz_frameset::ClearTune &ct = fs->clear_tune;
  if (!ctx->env_clear_wgs && ct.d_ctl && !ct.done && fs->max_tiles >= 8192) launch_clear_rebase(ct.d_ctl, s);
  return end_pass(ctx);
}

size_t srz_frameset_gbuffer_bytes(const srz_ctx *ctx, const srz_frameset *fs, uint32_t what) {
  if (!fs || what == 0u || (what & ~GB_GROUPS) != 0u) return 0;
  return (size_t)fs->n_frames * gbuf_planes(what) * fs->local_rows * (size_t)fs->width * sizeof(float);
}

int srz_frameset_gbuffer(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, void *d_out, size_t out_bytes, uint32_t what, uint32_t flags,
                         void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_gbuffer");
  if (!fs || !d_vis || !d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / output");
  if (what == 0u || (what & ~GB_GROUPS) != 0u) return fail(ctx, SRZ_E_INVALID, fn + ": `what` names no group or an unknown one");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  const size_t need = srz_frameset_gbuffer_bytes(ctx, fs, what), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (!aligned<16>({d_vis, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": buffers must be 16-byte aligned");
  if (ranges_overlap({d_out, need}, {d_vis, vis_bytes})) return fail(ctx, SRZ_E_INVALID, fn + ": the output overlaps the visibility buffer");
  hipStream_t s; // (the shading state: nothing but the albedo reads it)
  if (int rc = begin_pass(ctx, fs, stream, ((what & SRZ_GB_ALBEDO) ? PASS_SHADING : 0u) | PASS_VERTEX, &s)) return rc;
  GbufArgs a{};
  fill_walk(a, fs, d_vis, d_out);
  a.tris = fs->d_tris, a.tri_batch = fs->d_tri_batch, a.sdesc = fs->d_sdesc;
  a.vis_stride = 4ull * plane_words(fs), a.frame_stride = gbuf_planes(what) * plane_words(fs);
  a.flags_or = flags, a.what = what;
  launch_gbuffer(a, s);
  return end_pass(ctx);
}

size_t srz_frameset_motion_bytes(const srz_ctx *ctx, const srz_frameset *fs, uint32_t what) {
  if (!fs || what == 0u || (what & ~MV_GROUPS) != 0u) return 0;
  return (size_t)fs->n_frames * motion_planes(what) * fs->local_rows * (size_t)fs->width * sizeof(float);
}

int srz_frameset_motion(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, void *d_out, size_t out_bytes, uint32_t what, int delta,
                        uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_motion");
  if (!fs || !d_vis || !d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / output");
  if (what == 0u || (what & ~MV_GROUPS) != 0u) return fail(ctx, SRZ_E_INVALID, fn + ": `what` names no group or an unknown one");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  if ((what & SRZ_MV_TARGET) && fs->shard_world > 1)
    return fail(ctx, SRZ_E_INVALID, fn + ": SRZ_MV_TARGET needs the whole frame on this ctx (the target row may belong to another rank)");
  const size_t need = srz_frameset_motion_bytes(ctx, fs, what), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (!aligned<16>({d_vis, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": buffers must be 16-byte aligned");
  if (ranges_overlap({d_out, need}, {d_vis, vis_bytes})) return fail(ctx, SRZ_E_INVALID, fn + ": the output overlaps the visibility buffer");
  // triangle t of frame f + delta stands for triangle t of frame f: every pair inside the set must have one triangle count
  const int n = fs->n_frames, d = std::max(-n, std::min(n, delta)); // (beyond +-n no frame has a target: the same result)
  for (int f = 0; f < n; ++f) {
    const int g = f + d;
    if (g >= 0 && g < n && fs->h_frames[f].n_tris != fs->h_frames[g].n_tris)
      return fail(ctx, SRZ_E_INVALID, fn + ": frames " + std::to_string(f) + " and " + std::to_string(g) + " differ in triangle count");
  }
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, PASS_VERTEX, &s)) return rc;
  MotionArgs a{};
  fill_walk(a, fs, d_vis, d_out);
  fill_positions(a, fs);
  a.delta = d;
  a.vis_stride = 4ull * plane_words(fs), a.frame_stride = motion_planes(what) * plane_words(fs);
  a.flags_or = flags, a.what = what;
  launch_motion(a, s);
  return end_pass(ctx);
}

size_t srz_frameset_interpolate_bytes(const srz_ctx *ctx, const srz_frameset *fs, uint32_t n_ch) {
  if (!fs || n_ch == 0u || n_ch > SRZ_ATTR_MAX_CH) return 0;
  return (size_t)fs->n_frames * n_ch * fs->local_rows * (size_t)fs->width * sizeof(float);
}

int srz_frameset_interpolate(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_attr, uint32_t n_ch, uint32_t attr_frames,
                             uint32_t attr_tris, void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_interpolate");
  if (!fs || !d_vis || !d_attr || !d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / attributes / output");
  size_t attr_bytes = 0;
  if (int rc = check_interp(ctx, fs, fn, n_ch, attr_frames, attr_tris, flags, &attr_bytes)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, n_ch), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (!aligned<16>({d_vis, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": buffers must be 16-byte aligned");
  if (!aligned<4>({d_attr})) return fail(ctx, SRZ_E_INVALID, fn + ": the attributes must be 4-byte aligned");
  if (ranges_overlap({d_out, need}, {d_vis, vis_bytes}) || ranges_overlap({d_out, need}, {d_attr, attr_bytes}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the output overlaps the visibility buffer or the attributes");
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (the caller's attributes, not the set's triangles: no vertex stage)
  launch_interp(interp_args(fs, d_vis, d_attr, n_ch, attr_frames, attr_tris, n_ch, d_out, flags), s);
  return end_pass(ctx);
}

int srz_frameset_interpolate_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_gout, const float *d_attr, uint32_t n_ch,
                                  uint32_t attr_frames, uint32_t attr_tris, float *d_gattr, void *d_gbary, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_interpolate_grad");
  if (!fs || !d_vis || !d_gout) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / output gradient");
  if (!d_gattr && !d_gbary) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gattr nor d_gbary is asked for");
  if (d_gbary && !d_attr) return fail(ctx, SRZ_E_INVALID, fn + ": d_gbary needs the attributes");
  size_t attr_bytes = 0;
  if (int rc = check_interp(ctx, fs, fn, n_ch, attr_frames, attr_tris, flags, &attr_bytes)) return rc;
  const size_t gout_bytes = srz_frameset_interpolate_bytes(ctx, fs, n_ch), gbary_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u);
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (!aligned<16>({d_vis, d_gout, d_gbary})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers must be 16-byte aligned");
  if (!aligned<4>({d_attr, d_gattr})) return fail(ctx, SRZ_E_INVALID, fn + ": attributes and their gradient must be 4-byte aligned");
  if (int rc = check_grad_overlap(ctx, fn, {{d_gattr, attr_bytes}, {d_gbary, gbary_bytes}},
                                  {{d_vis, vis_bytes}, {d_gout, gout_bytes}, {d_attr, attr_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_interpolate)
  InterpArgs a = interp_args(fs, d_vis, d_attr, n_ch, attr_frames, attr_tris, 2u, d_gbary, flags);
  a.gout = (const float *)d_gout, a.gattr = d_gattr;
  launch_interp_grad(a, s);
  return end_pass(ctx);
}

int srz_frameset_position_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_gbary, const void *d_gz, uint32_t pos_tris,
                               float *d_gpos, void *d_gpix, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_position_grad");
  if (!fs || !d_vis) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer");
  if (!d_gbary && !d_gz) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gbary nor d_gz is given");
  if (!d_gpos && !d_gpix) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gpos nor d_gpix is asked for");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  if (int rc = check_tri_count(ctx, fs, fn, "pos_tris", pos_tris)) return rc;
  const size_t two_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u), one_bytes = srz_frameset_interpolate_bytes(ctx, fs, 1u);
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs), gpos_bytes = (size_t)fs->n_frames * pos_tris * TRI_POS_F * sizeof(float);
  if (!aligned<16>({d_vis, d_gbary, d_gz, d_gpix})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers must be 16-byte aligned");
  if (!aligned<4>({d_gpos})) return fail(ctx, SRZ_E_INVALID, fn + ": the position gradient must be 4-byte aligned");
  if (int rc = check_grad_overlap(ctx, fn, {{d_gpos, gpos_bytes}, {d_gpix, two_bytes}},
                                  {{d_vis, vis_bytes}, {d_gbary, two_bytes}, {d_gz, one_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, PASS_VERTEX, &s)) return rc;
  PosGradArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_gpix);
  fill_positions(a, fs);
  a.gbary = (const float *)d_gbary, a.gz = (const float *)d_gz, a.gpos = d_gpos;
  a.vis_stride = 4ull * plane, a.frame_stride = 2ull * plane, a.gz_stride = plane, a.gpos_stride = (uint64_t)pos_tris * TRI_POS_F;
  a.flags_or = flags;
  launch_pos_grad(a, s);
  return end_pass(ctx);
}

int srz_frameset_positions(srz_ctx *ctx, srz_frameset *fs, uint32_t pos_tris, float *d_pos, size_t pos_bytes, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_positions");
  if (!fs || !d_pos) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / output");
  if (int rc = check_tri_count(ctx, fs, fn, "pos_tris", pos_tris)) return rc;
  if (pos_bytes < (size_t)fs->n_frames * pos_tris * TRI_POS_F * sizeof(float)) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (!aligned<4>({d_pos})) return fail(ctx, SRZ_E_INVALID, fn + ": the positions must be 4-byte aligned");
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, PASS_VERTEX, &s)) return rc;
  struct {
    const float *tri_pos;
    uint32_t pos_stride;
  } p;
  fill_positions(p, fs);
  launch_positions(fs->d_frames, (uint32_t)fs->n_frames, p.tri_pos, p.pos_stride, d_pos, pos_tris, s);
  return end_pass(ctx);
}

// what the passes over ONE mesh slot of a sceneset check alike (srz_sceneset_vertex_grad, srz_sceneset_corner_attr / _grad): the slot
// holds a mesh, the set draws it, and the slot still holds the upload the set's draws point into
static int check_drawn_slot(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, int mesh_id) {
  if (mesh_id < 0 || mesh_id >= MAX_MESH || !ctx->mesh[mesh_id].d_verts) return fail(ctx, SRZ_E_INVALID, fn + ": no mesh in that slot");
  bool drawn = false;
  for (size_t di = 0; di < fs->h_draw_mesh.size(); ++di) {
    if (fs->h_draw_mesh[di] != mesh_id) continue;
    drawn = true;
    // (as srz_sceneset_update)
    if (ctx->mesh[mesh_id].upload != fs->h_draw_upload[di]) return fail(ctx, SRZ_E_INVALID, fn + ": the slot was uploaded anew since the set was created");
  }
  if (!drawn) return fail(ctx, SRZ_E_INVALID, fn + ": the set draws no mesh of that slot");
  return SRZ_OK;
}

int srz_sceneset_vertex_grad(srz_ctx *ctx, srz_frameset *fs, int mesh_id, const float *d_gpos, uint32_t pos_tris, float *d_gverts,
                             float *d_gdraw, uint32_t draw_stride, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_sceneset_vertex_grad");
  if (!fs || !fs->d_draws) return fail(ctx, SRZ_E_INVALID, fn + ": not a sceneset");
  if (!d_gpos) return fail(ctx, SRZ_E_INVALID, fn + ": null position gradient");
  if (!d_gverts && !d_gdraw) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gverts nor d_gdraw is asked for");
  if (int rc = check_drawn_slot(ctx, fs, fn, mesh_id)) return rc;
  const srz_ctx::MeshSlot &m = ctx->mesh[mesh_id];
  if (int rc = check_tri_count(ctx, fs, fn, "pos_tris", pos_tris)) return rc;
  if (d_gdraw)
    for (const FrameDesc &d : fs->h_frames)
      if (d.n_batches > draw_stride) return fail(ctx, SRZ_E_INVALID, fn + ": draw_stride is below a frame's draw count");
  if (!aligned<4>({d_gpos, d_gverts, d_gdraw})) return fail(ctx, SRZ_E_INVALID, fn + ": the buffers must be 4-byte aligned");
  const size_t gpos_bytes = (size_t)fs->n_frames * pos_tris * TRI_POS_F * sizeof(float);
  const size_t gverts_bytes = (size_t)fs->n_frames * m.n_verts * 3u * sizeof(float);
  const size_t gdraw_bytes = (size_t)fs->n_frames * draw_stride * VG_VALS * sizeof(float);
  if (int rc = check_grad_overlap(ctx, fn, {{d_gverts, gverts_bytes}, {d_gdraw, gdraw_bytes}}, {{d_gpos, gpos_bytes}})) return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (the pass reads vertices, matrices and d_gpos: no triangle of the set)
  VertexGradArgs a{};
  a.frames = fs->d_frames, a.draws = fs->d_draws;
  a.verts = m.d_verts, a.corner_off = m.d_corner_off, a.corners = m.d_corner_off + m.n_verts + 1;
  a.gpos = d_gpos, a.gverts = d_gverts, a.gdraw = d_gdraw;
  a.gpos_stride = (uint64_t)pos_tris * TRI_POS_F;
  a.n_verts = m.n_verts, a.n_frames = (uint32_t)fs->n_frames, a.draw_stride = draw_stride;
  launch_vertex_grad(a, s);
  return end_pass(ctx);
}

// what srz_sceneset_corner_attr and _corner_attr_grad check alike, and the fields of `a` they fill alike
static int check_corner_attr(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, int mesh_id, uint32_t n_ch, uint32_t pos_tris,
                             CornerAttrArgs &a) {
  if (!fs || !fs->d_draws) return fail(ctx, SRZ_E_INVALID, fn + ": not a sceneset");
  if (int rc = check_drawn_slot(ctx, fs, fn, mesh_id)) return rc;
  if (n_ch == 0u || n_ch > SRZ_ATTR_MAX_CH) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. SRZ_ATTR_MAX_CH");
  if (int rc = check_tri_count(ctx, fs, fn, "pos_tris", pos_tris)) return rc;
  const srz_ctx::MeshSlot &m = ctx->mesh[mesh_id];
  a.frames = fs->d_frames, a.draws = fs->d_draws;
  a.verts = m.d_verts, a.corner_off = m.d_corner_off, a.corners = m.d_corner_off + m.n_verts + 1;
  a.n_verts = m.n_verts, a.n_ch = n_ch, a.pos_tris = pos_tris, a.n_frames = (uint32_t)fs->n_frames;
  return SRZ_OK;
}

int srz_sceneset_corner_attr(srz_ctx *ctx, srz_frameset *fs, int mesh_id, const float *d_attr, uint32_t n_ch, uint32_t attr_frames,
                             float *d_out, uint32_t pos_tris, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_sceneset_corner_attr");
  CornerAttrArgs a{};
  if (int rc = check_corner_attr(ctx, fs, fn, mesh_id, n_ch, pos_tris, a)) return rc;
  if (!d_attr || !d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null attributes / output");
  if (attr_frames != 1u && attr_frames != (uint32_t)fs->n_frames) return fail(ctx, SRZ_E_INVALID, fn + ": attr_frames must be 1 or the set's frame count");
  if (!aligned<4>({d_attr, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": the buffers must be 4-byte aligned");
  const size_t per_frame = (size_t)a.n_verts * n_ch;
  if (ranges_overlap({d_out, (size_t)fs->n_frames * pos_tris * 3u * n_ch * sizeof(float)}, {d_attr, attr_frames * per_frame * sizeof(float)}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the output overlaps the attributes");
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (the pass reads the draws' offsets and the slot's lists: no triangle of the set)
  a.attr = d_attr, a.out = d_out, a.attr_frame_stride = attr_frames == 1u ? 0u : per_frame;
  launch_corner_attr(a, s);
  return end_pass(ctx);
}

int srz_sceneset_corner_attr_grad(srz_ctx *ctx, srz_frameset *fs, int mesh_id, const float *d_gout, uint32_t n_ch, float *d_gattr,
                                  uint32_t pos_tris, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_sceneset_corner_attr_grad");
  CornerAttrArgs a{};
  if (int rc = check_corner_attr(ctx, fs, fn, mesh_id, n_ch, pos_tris, a)) return rc;
  if (!d_gout || !d_gattr) return fail(ctx, SRZ_E_INVALID, fn + ": null output gradient / attribute gradient");
  if (!aligned<4>({d_gout, d_gattr})) return fail(ctx, SRZ_E_INVALID, fn + ": the buffers must be 4-byte aligned");
  if (ranges_overlap({d_gattr, (size_t)fs->n_frames * a.n_verts * n_ch * sizeof(float)},
                     {d_gout, (size_t)fs->n_frames * pos_tris * 3u * n_ch * sizeof(float)}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the attribute gradient overlaps the output gradient");
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc;
  a.gout = d_gout, a.gattr = d_gattr;
  launch_corner_attr_grad(a, s);
  return end_pass(ctx);
}

int srz_frameset_antialias(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_in, uint32_t n_ch, void *d_out, size_t out_bytes,
                           uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_antialias");
  if (!fs || !d_vis || !d_in || !d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / input / output");
  if (int rc = check_antialias(ctx, fs, fn, n_ch, flags)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, n_ch), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (!aligned<16>({d_vis, d_in, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": buffers must be 16-byte aligned");
  if (ranges_overlap({d_out, need}, {d_vis, vis_bytes}) || ranges_overlap({d_out, need}, {d_in, need}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the output overlaps the visibility buffer or the input (the pass reads neighbours: not in place)");
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, PASS_VERTEX, &s)) return rc;
  launch_antialias(antialias_args(fs, d_vis, d_in, n_ch, d_out), s);
  return end_pass(ctx);
}

int srz_frameset_antialias_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_in, const void *d_gout, uint32_t n_ch,
                                void *d_gin, uint32_t pos_tris, float *d_gpos, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_antialias_grad");
  if (!fs || !d_vis || !d_in || !d_gout) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / input / output gradient");
  if (!d_gin && !d_gpos) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gin nor d_gpos is asked for");
  if (int rc = check_antialias(ctx, fs, fn, n_ch, flags)) return rc;
  if (d_gpos)
    if (int rc = check_tri_count(ctx, fs, fn, "pos_tris", pos_tris)) return rc;
  const size_t planes_bytes = srz_frameset_interpolate_bytes(ctx, fs, n_ch), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  const size_t gpos_bytes = (size_t)fs->n_frames * pos_tris * TRI_POS_F * sizeof(float);
  if (!aligned<16>({d_vis, d_in, d_gout, d_gin})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers must be 16-byte aligned");
  if (!aligned<4>({d_gpos})) return fail(ctx, SRZ_E_INVALID, fn + ": the position gradient must be 4-byte aligned");
  if (int rc = check_grad_overlap(ctx, fn, {{d_gin, planes_bytes}, {d_gpos, gpos_bytes}},
                                  {{d_vis, vis_bytes}, {d_in, planes_bytes}, {d_gout, planes_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, PASS_VERTEX, &s)) return rc;
  AntialiasArgs a = antialias_args(fs, d_vis, d_in, n_ch, d_gin);
  a.gout = (const float *)d_gout, a.gpos = d_gpos, a.gpos_stride = (uint64_t)pos_tris * TRI_POS_F;
  launch_antialias_grad(a, s);
  return end_pass(ctx);
}

int srz_frameset_texture(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_uv, const float *d_tex, uint32_t tex_w,
                         uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t mode, void *d_out, size_t out_bytes, uint32_t flags,
                         void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_texture");
  if (!fs || !d_vis || !d_uv || !d_tex || !d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / uv / texture / output");
  size_t tex_bytes = 0;
  if (int rc = check_texture(ctx, fs, fn, tex_w, tex_h, n_ch, tex_frames, mode, flags, &tex_bytes)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, n_ch), uv_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u);
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (!aligned<16>({d_vis, d_uv, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers must be 16-byte aligned");
  if (!aligned<4>({d_tex})) return fail(ctx, SRZ_E_INVALID, fn + ": the texture must be 4-byte aligned");
  if (ranges_overlap({d_out, need}, {d_vis, vis_bytes}) || ranges_overlap({d_out, need}, {d_uv, uv_bytes}) ||
      ranges_overlap({d_out, need}, {d_tex, tex_bytes}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the output overlaps the visibility buffer, uv or the texture");
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (the caller's uv and texture, not the set's: no shading state, no vertex stage)
  launch_tex(texture_args(fs, d_vis, d_uv, d_tex, tex_w, tex_h, n_ch, tex_frames, mode, n_ch, d_out, flags), s);
  return end_pass(ctx);
}

int srz_frameset_texture_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_uv, const void *d_gout, const float *d_tex,
                              uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t mode, float *d_gtex, void *d_guv,
                              uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_texture_grad");
  if (!fs || !d_vis || !d_uv || !d_gout) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / uv / output gradient");
  if (!d_gtex && !d_guv) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gtex nor d_guv is asked for");
  if (d_guv && !d_tex) return fail(ctx, SRZ_E_INVALID, fn + ": d_guv needs the texture");
  size_t tex_bytes = 0;
  if (int rc = check_texture(ctx, fs, fn, tex_w, tex_h, n_ch, tex_frames, mode, flags, &tex_bytes)) return rc;
  const size_t gout_bytes = srz_frameset_interpolate_bytes(ctx, fs, n_ch), uv_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u);
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (!aligned<16>({d_vis, d_uv, d_gout, d_guv})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers must be 16-byte aligned");
  if (!aligned<4>({d_tex, d_gtex})) return fail(ctx, SRZ_E_INVALID, fn + ": the texture and its gradient must be 4-byte aligned");
  if (int rc = check_grad_overlap(ctx, fn, {{d_gtex, tex_bytes}, {d_guv, uv_bytes}},
                                  {{d_vis, vis_bytes}, {d_uv, uv_bytes}, {d_gout, gout_bytes}, {d_tex, tex_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture)
  TexArgs a = texture_args(fs, d_vis, d_uv, d_tex, tex_w, tex_h, n_ch, tex_frames, mode, 2u, d_guv, flags);
  a.gout = (const float *)d_gout, a.gtex = d_gtex;
  launch_tex_grad(a, s);
  return end_pass(ctx);
}

int srz_frameset_texture_cube(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_dir, const float *d_tex, uint32_t n,
                              uint32_t n_ch, uint32_t tex_frames, void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_texture_cube");
  if (!fs || !d_vis || !d_dir || !d_tex || !d_out)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_dir ? "d_dir" : !d_tex ? "d_tex" : "d_out"));
  size_t tex_bytes = 0;
  if (int rc = check_cube(ctx, fs, fn, n, n_ch, tex_frames, flags, &tex_bytes)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, n_ch), dir_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u);
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_vis, d_dir, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_dir, d_out) must be 16-byte aligned");
  if (!aligned<4>({d_tex})) return fail(ctx, SRZ_E_INVALID, fn + ": d_tex must be 4-byte aligned");
  if (ranges_overlap({d_out, need}, {d_vis, vis_bytes}) || ranges_overlap({d_out, need}, {d_dir, dir_bytes}) ||
      ranges_overlap({d_out, need}, {d_tex, tex_bytes}))
    return fail(ctx, SRZ_E_INVALID, fn + ": d_out overlaps d_vis, d_dir or d_tex");
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture)
  launch_cube(cube_args(fs, d_vis, d_dir, d_tex, n, n_ch, tex_frames, n_ch, d_out, flags), s);
  return end_pass(ctx);
}

int srz_frameset_texture_cube_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_dir, const void *d_gout,
                                   const float *d_tex, uint32_t n, uint32_t n_ch, uint32_t tex_frames, float *d_gtex, void *d_gdir,
                                   uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_texture_cube_grad");
  if (!fs || !d_vis || !d_dir || !d_gout)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_dir ? "d_dir" : "d_gout"));
  if (!d_gtex && !d_gdir) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gtex nor d_gdir is asked for");
  if (d_gdir && !d_tex) return fail(ctx, SRZ_E_INVALID, fn + ": d_gdir needs d_tex");
  size_t tex_bytes = 0;
  if (int rc = check_cube(ctx, fs, fn, n, n_ch, tex_frames, flags, &tex_bytes)) return rc;
  const size_t gout_bytes = srz_frameset_interpolate_bytes(ctx, fs, n_ch), dir_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u);
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (!aligned<16>({d_vis, d_dir, d_gout, d_gdir}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_dir, d_gout, d_gdir) must be 16-byte aligned");
  if (!aligned<4>({d_tex, d_gtex})) return fail(ctx, SRZ_E_INVALID, fn + ": d_tex and d_gtex must be 4-byte aligned");
  if (int rc = check_grad_overlap(ctx, fn + " (d_gtex, d_gdir against d_vis, d_dir, d_gout, d_tex)", {{d_gtex, tex_bytes}, {d_gdir, dir_bytes}},
                                  {{d_vis, vis_bytes}, {d_dir, dir_bytes}, {d_gout, gout_bytes}, {d_tex, tex_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture)
  CubeArgs a = cube_args(fs, d_vis, d_dir, d_tex, n, n_ch, tex_frames, 3u, d_gdir, flags);
  a.gout = (const float *)d_gout, a.gtex = d_gtex;
  launch_cube_grad(a, s);
  return end_pass(ctx);
}

namespace {
// what srz_frameset_background and _background_grad check alike behind their null pointers (check_cube, then the block and `where`);
// the cube's bytes in *tex_bytes, the block's in *ray_bytes
int check_background(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, uint32_t ray_frames, uint32_t n, uint32_t n_ch,
                     uint32_t tex_frames, uint32_t where, uint32_t flags, size_t *tex_bytes, size_t *ray_bytes) {
  if (int rc = check_cube(ctx, fs, fn, n, n_ch, tex_frames, flags, tex_bytes)) return rc;
  if (ray_frames != 1u && ray_frames != (uint32_t)fs->n_frames)
    return fail(ctx, SRZ_E_INVALID, fn + ": ray_frames must be 1 or the set's frame count");
  if (where > SRZ_BG_ALL) return fail(ctx, SRZ_E_INVALID, fn + ": where must be SRZ_BG_NOBODY or SRZ_BG_ALL");
  *ray_bytes = (size_t)ray_frames * 9u * sizeof(float);
  return SRZ_OK;
}
BgArgs background_args(const srz_frameset *fs, const void *d_vis, const float *d_ray, uint32_t ray_frames, const float *d_tex, uint32_t n,
                       uint32_t n_ch, uint32_t tex_frames, uint32_t where, void *d_out, uint32_t flags) {
  BgArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.ray = d_ray, a.tex = d_tex;
  a.vis_stride = 4ull * plane, a.frame_stride = n_ch * plane, a.gout_stride = n_ch * plane;
  a.tex_frame_stride = tex_frames == 1u ? 0ull : 6ull * n * n * n_ch;
  a.ray_stride = ray_frames == 1u ? 0ull : 9ull;
  a.n = n, a.n_ch = n_ch, a.where = where;
  a.flags_or = flags;
  return a;
}
} // namespace

int srz_frameset_background(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_ray, uint32_t ray_frames, const float *d_tex,
                            uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t where, void *d_out, size_t out_bytes, uint32_t flags,
                            void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_background");
  if (where == SRZ_BG_ALL) d_vis = nullptr; // (not read: it may be anything)
  if (!fs || (!d_vis && where == SRZ_BG_NOBODY) || !d_ray || !d_tex || !d_out)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_ray ? "d_ray" : !d_tex ? "d_tex" : !d_out ? "d_out" : "d_vis"));
  size_t tex_bytes = 0, ray_bytes = 0;
  if (int rc = check_background(ctx, fs, fn, ray_frames, n, n_ch, tex_frames, where, flags, &tex_bytes, &ray_bytes)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, n_ch), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_vis, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_out) must be 16-byte aligned");
  if (!aligned<4>({d_ray, d_tex})) return fail(ctx, SRZ_E_INVALID, fn + ": d_ray and d_tex must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn + " (d_out against d_vis, d_ray, d_tex)", {{d_out, need}},
                              {{d_vis, vis_bytes}, {d_ray, ray_bytes}, {d_tex, tex_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture_cube: caller data only)
  launch_background(background_args(fs, d_vis, d_ray, ray_frames, d_tex, n, n_ch, tex_frames, where, d_out, flags), s);
  return end_pass(ctx);
}

size_t srz_frameset_background_work_bytes(srz_ctx *ctx, srz_frameset *fs) {
  if (!ctx || !fs) return 0;
  // [frame][tile][9] partial sums, and [frame][9] rows for the fold of a shared ray block
  return (size_t)fs->n_frames * ((size_t)fs->n_local_bands * fs->tiles_x + 1u) * 9u * sizeof(float);
}

int srz_frameset_background_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_ray, uint32_t ray_frames,
                                 const void *d_gout, const float *d_tex, uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t where,
                                 float *d_gtex, float *d_gray, void *d_work, size_t work_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_background_grad");
  if (where == SRZ_BG_ALL) d_vis = nullptr; // (not read: it may be anything)
  if (!fs || (!d_vis && where == SRZ_BG_NOBODY) || !d_ray || !d_gout)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_ray ? "d_ray" : !d_gout ? "d_gout" : "d_vis"));
  if (!d_gtex && !d_gray) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gtex nor d_gray is asked for");
  if (d_gray && !d_tex) return fail(ctx, SRZ_E_INVALID, fn + ": d_gray needs d_tex");
  if (d_gray && !d_work) return fail(ctx, SRZ_E_INVALID, fn + ": d_gray needs d_work");
  size_t tex_bytes = 0, ray_bytes = 0;
  if (int rc = check_background(ctx, fs, fn, ray_frames, n, n_ch, tex_frames, where, flags, &tex_bytes, &ray_bytes)) return rc;
  const size_t gout_bytes = srz_frameset_interpolate_bytes(ctx, fs, n_ch), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  const size_t need_work = d_gray ? srz_frameset_background_work_bytes(ctx, fs) : 0;
  if (work_bytes < need_work) return fail(ctx, SRZ_E_INVALID, fn + ": work_bytes is below srz_frameset_background_work_bytes");
  if (!aligned<16>({d_vis, d_gout})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_gout) must be 16-byte aligned");
  if (!aligned<4>({d_ray, d_tex, d_gtex, d_gray, d_gray ? d_work : nullptr}))
    return fail(ctx, SRZ_E_INVALID, fn + ": d_ray, d_tex, d_gtex, d_gray and d_work must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn + " (d_gtex, d_gray, d_work against d_vis, d_ray, d_gout, d_tex)",
                              {{d_gtex, tex_bytes}, {d_gray, ray_bytes}, {d_gray ? d_work : nullptr, need_work}},
                              {{d_vis, vis_bytes}, {d_ray, ray_bytes}, {d_gout, gout_bytes}, {d_tex, tex_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture_cube: caller data only)
  BgArgs a = background_args(fs, d_vis, d_ray, ray_frames, d_tex, n, n_ch, tex_frames, where, nullptr, flags);
  a.gout = (const float *)d_gout, a.gtex = d_gtex;
  a.work = d_gray ? (float *)d_work : nullptr;
  launch_background_grad(a, d_gray, s);
  return end_pass(ctx);
}

int srz_frameset_shadow(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_sc, const float *d_map, uint32_t map_w,
                        uint32_t map_h, uint32_t map_frames, float bias, float width, void *d_out, size_t out_bytes, uint32_t flags,
                        void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_shadow");
  if (!fs || !d_vis || !d_sc || !d_map || !d_out)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_sc ? "d_sc" : !d_map ? "d_map" : "d_out"));
  size_t map_bytes = 0;
  if (int rc = check_shadow(ctx, fs, fn, map_w, map_h, map_frames, bias, width, flags, &map_bytes)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, 1u), sc_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u);
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_vis, d_sc, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_sc, d_out) must be 16-byte aligned");
  if (!aligned<4>({d_map})) return fail(ctx, SRZ_E_INVALID, fn + ": d_map must be 4-byte aligned");
  if (ranges_overlap({d_out, need}, {d_vis, vis_bytes}) || ranges_overlap({d_out, need}, {d_sc, sc_bytes}) ||
      ranges_overlap({d_out, need}, {d_map, map_bytes}))
    return fail(ctx, SRZ_E_INVALID, fn + ": d_out overlaps d_vis, d_sc or d_map");
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture)
  launch_shadow(shadow_args(fs, d_vis, d_sc, d_map, map_w, map_h, map_frames, bias, width, 1u, d_out, flags), s);
  return end_pass(ctx);
}

int srz_frameset_shadow_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_sc, const void *d_gout, const float *d_map,
                             uint32_t map_w, uint32_t map_h, uint32_t map_frames, float bias, float width, float *d_gmap, void *d_gsc,
                             uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_shadow_grad");
  if (!fs || !d_vis || !d_sc || !d_gout || !d_map)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_sc ? "d_sc" : !d_gout ? "d_gout" : "d_map"));
  if (!d_gmap && !d_gsc) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gmap nor d_gsc is asked for");
  size_t map_bytes = 0;
  if (int rc = check_shadow(ctx, fs, fn, map_w, map_h, map_frames, bias, width, flags, &map_bytes)) return rc;
  const size_t gout_bytes = srz_frameset_interpolate_bytes(ctx, fs, 1u), sc_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u);
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (!aligned<16>({d_vis, d_sc, d_gout, d_gsc}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_sc, d_gout, d_gsc) must be 16-byte aligned");
  if (!aligned<4>({d_map, d_gmap})) return fail(ctx, SRZ_E_INVALID, fn + ": d_map and d_gmap must be 4-byte aligned");
  if (int rc = check_grad_overlap(ctx, fn + " (d_gmap, d_gsc against d_vis, d_sc, d_gout, d_map)", {{d_gmap, map_bytes}, {d_gsc, sc_bytes}},
                                  {{d_vis, vis_bytes}, {d_sc, sc_bytes}, {d_gout, gout_bytes}, {d_map, map_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture)
  ShadowArgs a = shadow_args(fs, d_vis, d_sc, d_map, map_w, map_h, map_frames, bias, width, 3u, d_gsc, flags);
  a.gout = (const float *)d_gout, a.gmap = d_gmap;
  launch_shadow_grad(a, s);
  return end_pass(ctx);
}

int srz_frameset_light(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const void *d_kd,
                       const float *d_par, uint32_t n_lights, uint32_t par_frames, uint32_t p, void *d_out, size_t out_bytes, uint32_t flags,
                       void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_light");
  if (!fs || !d_vis || !d_nrm || !d_pos || !d_par || !d_out)
    return fail(ctx, SRZ_E_INVALID,
                fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_nrm ? "d_nrm" : !d_pos ? "d_pos" : !d_par ? "d_par" : "d_out"));
  size_t par_bytes = 0;
  if (int rc = check_light(ctx, fs, fn, n_lights, par_frames, p, flags, &par_bytes)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, 3u), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_vis, d_nrm, d_pos, d_kd, d_out}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_nrm, d_pos, d_kd, d_out) must be 16-byte aligned");
  if (!aligned<4>({d_par})) return fail(ctx, SRZ_E_INVALID, fn + ": d_par must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn + " (d_out against d_vis, d_nrm, d_pos, d_kd, d_par)", {{d_out, need}},
                              {{d_vis, vis_bytes}, {d_nrm, need}, {d_pos, need}, {d_kd, need}, {d_par, par_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture: caller data only)
  launch_light(light_args(fs, d_vis, d_nrm, d_pos, d_kd, d_par, n_lights, par_frames, p, d_out, flags), s);
  return end_pass(ctx);
}

size_t srz_frameset_light_work_bytes(srz_ctx *ctx, srz_frameset *fs, uint32_t n_lights) {
  if (!ctx || !fs || n_lights == 0u || n_lights > SRZ_LIGHT_MAX) return 0;
  // [frame][tile][K] partial sums, and [frame][K] rows for the fold of a shared parameter frame
  return (size_t)fs->n_frames * ((size_t)fs->n_local_bands * fs->tiles_x + 1u) * SRZ_LIGHT_PAR(n_lights) * sizeof(float);
}

int srz_frameset_light_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const void *d_kd,
                            const float *d_par, uint32_t n_lights, uint32_t par_frames, uint32_t p, const void *d_gout, void *d_gnrm,
                            void *d_gpos, void *d_gkd, float *d_gpar, void *d_work, size_t work_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_light_grad");
  if (!fs || !d_vis || !d_nrm || !d_pos || !d_par || !d_gout)
    return fail(ctx, SRZ_E_INVALID,
                fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_nrm ? "d_nrm" : !d_pos ? "d_pos" : !d_par ? "d_par" : "d_gout"));
  if (!d_gnrm && !d_gpos && !d_gkd && !d_gpar) return fail(ctx, SRZ_E_INVALID, fn + ": none of d_gnrm, d_gpos, d_gkd, d_gpar is asked for");
  if (d_gkd && !d_kd) return fail(ctx, SRZ_E_INVALID, fn + ": d_gkd needs d_kd");
  if (d_gpar && !d_work) return fail(ctx, SRZ_E_INVALID, fn + ": d_gpar needs d_work");
  size_t par_bytes = 0;
  if (int rc = check_light(ctx, fs, fn, n_lights, par_frames, p, flags, &par_bytes)) return rc;
  const size_t plane_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  const size_t need_work = d_gpar ? srz_frameset_light_work_bytes(ctx, fs, n_lights) : 0;
  if (work_bytes < need_work) return fail(ctx, SRZ_E_INVALID, fn + ": work_bytes is below srz_frameset_light_work_bytes");
  if (!aligned<16>({d_vis, d_nrm, d_pos, d_kd, d_gout, d_gnrm, d_gpos, d_gkd}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_nrm, d_pos, d_kd, d_gout, d_gnrm, d_gpos, d_gkd) must be 16-byte aligned");
  if (!aligned<4>({d_par, d_gpar, d_gpar ? d_work : nullptr})) return fail(ctx, SRZ_E_INVALID, fn + ": d_par, d_gpar and d_work must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn + " (d_gnrm, d_gpos, d_gkd, d_gpar, d_work against d_vis, d_nrm, d_pos, d_kd, d_par, d_gout)",
                              {{d_gnrm, plane_bytes}, {d_gpos, plane_bytes}, {d_gkd, plane_bytes}, {d_gpar, par_bytes},
                               {d_gpar ? d_work : nullptr, need_work}},
                              {{d_vis, vis_bytes}, {d_nrm, plane_bytes}, {d_pos, plane_bytes}, {d_kd, plane_bytes}, {d_par, par_bytes},
                               {d_gout, plane_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc;
  LightArgs a = light_args(fs, d_vis, d_nrm, d_pos, d_kd, d_par, n_lights, par_frames, p, nullptr, flags);
  a.gout = (const float *)d_gout, a.gnrm = (float *)d_gnrm, a.gpos = (float *)d_gpos, a.gkd = (float *)d_gkd;
  a.work = d_gpar ? (float *)d_work : nullptr;
  launch_light_grad(a, d_gpar, s);
  return end_pass(ctx);
}

namespace {
// what srz_frameset_microfacet and _microfacet_grad check alike (check_light without the exponent, in its words); the parameter
// block's bytes in *par_bytes
int check_microfacet(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, uint32_t n_lights, uint32_t par_frames, uint32_t flags,
                     size_t *par_bytes) {
  if (n_lights == 0u || n_lights > SRZ_LIGHT_MAX) return fail(ctx, SRZ_E_INVALID, fn + ": n_lights must be 1 .. SRZ_LIGHT_MAX");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  if (par_frames != 1u && par_frames != (uint32_t)fs->n_frames)
    return fail(ctx, SRZ_E_INVALID, fn + ": par_frames must be 1 or the set's frame count");
  *par_bytes = (size_t)par_frames * SRZ_MICROFACET_PAR(n_lights) * sizeof(float);
  return SRZ_OK;
}
MicrofacetArgs microfacet_args(const srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const void *d_base,
                               const void *d_mat, const float *d_par, uint32_t n_lights, uint32_t par_frames, void *d_out, uint32_t flags) {
  MicrofacetArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.nrm = (const float *)d_nrm, a.pos = (const float *)d_pos, a.base = (const float *)d_base, a.mat = (const float *)d_mat, a.par = d_par;
  a.vis_stride = 4ull * plane, a.frame_stride = 3ull * plane, a.mat_stride = 2ull * plane;
  a.par_stride = par_frames == 1u ? 0ull : (uint64_t)SRZ_MICROFACET_PAR(n_lights);
  a.n_lights = n_lights;
  a.flags_or = flags;
  return a;
}
} // namespace

int srz_frameset_microfacet(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const void *d_base,
                            const void *d_mat, const float *d_par, uint32_t n_lights, uint32_t par_frames, void *d_out, size_t out_bytes,
                            uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_microfacet");
  if (!fs || !d_vis || !d_nrm || !d_pos || !d_mat || !d_par || !d_out)
    return fail(ctx, SRZ_E_INVALID,
                fn + ": null " +
                    (!fs ? "frameset" : !d_vis ? "d_vis" : !d_nrm ? "d_nrm" : !d_pos ? "d_pos" : !d_mat ? "d_mat" : !d_par ? "d_par" : "d_out"));
  size_t par_bytes = 0;
  if (int rc = check_microfacet(ctx, fs, fn, n_lights, par_frames, flags, &par_bytes)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, 3u), mat_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u),
               vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_vis, d_nrm, d_pos, d_base, d_mat, d_out}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_nrm, d_pos, d_base, d_mat, d_out) must be 16-byte aligned");
  if (!aligned<4>({d_par})) return fail(ctx, SRZ_E_INVALID, fn + ": d_par must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn + " (d_out against d_vis, d_nrm, d_pos, d_base, d_mat, d_par)", {{d_out, need}},
                              {{d_vis, vis_bytes}, {d_nrm, need}, {d_pos, need}, {d_base, need}, {d_mat, mat_bytes}, {d_par, par_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_light: caller data only)
  launch_microfacet(microfacet_args(fs, d_vis, d_nrm, d_pos, d_base, d_mat, d_par, n_lights, par_frames, d_out, flags), s);
  return end_pass(ctx);
}

size_t srz_frameset_microfacet_work_bytes(srz_ctx *ctx, srz_frameset *fs, uint32_t n_lights) {
  if (!ctx || !fs || n_lights == 0u || n_lights > SRZ_LIGHT_MAX) return 0;
  // [frame][tile][K] partial sums, and [frame][K] rows for the fold of a shared parameter frame
  return (size_t)fs->n_frames * ((size_t)fs->n_local_bands * fs->tiles_x + 1u) * SRZ_MICROFACET_PAR(n_lights) * sizeof(float);
}

int srz_frameset_microfacet_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos,
                                 const void *d_base, const void *d_mat, const float *d_par, uint32_t n_lights, uint32_t par_frames,
                                 const void *d_gout, void *d_gnrm, void *d_gpos, void *d_gbase, void *d_gmat, float *d_gpar, void *d_work,
                                 size_t work_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_microfacet_grad");
  if (!fs || !d_vis || !d_nrm || !d_pos || !d_mat || !d_par || !d_gout)
    return fail(ctx, SRZ_E_INVALID,
                fn + ": null " +
                    (!fs ? "frameset" : !d_vis ? "d_vis" : !d_nrm ? "d_nrm" : !d_pos ? "d_pos" : !d_mat ? "d_mat" : !d_par ? "d_par" : "d_gout"));
  if (!d_gnrm && !d_gpos && !d_gbase && !d_gmat && !d_gpar)
    return fail(ctx, SRZ_E_INVALID, fn + ": none of d_gnrm, d_gpos, d_gbase, d_gmat, d_gpar is asked for");
  if (d_gbase && !d_base) return fail(ctx, SRZ_E_INVALID, fn + ": d_gbase needs d_base");
  if (d_gpar && !d_work) return fail(ctx, SRZ_E_INVALID, fn + ": d_gpar needs d_work");
  size_t par_bytes = 0;
  if (int rc = check_microfacet(ctx, fs, fn, n_lights, par_frames, flags, &par_bytes)) return rc;
  const size_t plane_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u), mat_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u),
               vis_bytes = srz_frameset_out_bytes(ctx, fs);
  const size_t need_work = d_gpar ? srz_frameset_microfacet_work_bytes(ctx, fs, n_lights) : 0;
  if (work_bytes < need_work) return fail(ctx, SRZ_E_INVALID, fn + ": work_bytes is below srz_frameset_microfacet_work_bytes");
  if (!aligned<16>({d_vis, d_nrm, d_pos, d_base, d_mat, d_gout, d_gnrm, d_gpos, d_gbase, d_gmat}))
    return fail(ctx, SRZ_E_INVALID,
                fn + ": the plane buffers (d_vis, d_nrm, d_pos, d_base, d_mat, d_gout, d_gnrm, d_gpos, d_gbase, d_gmat) must be 16-byte aligned");
  if (!aligned<4>({d_par, d_gpar, d_gpar ? d_work : nullptr})) return fail(ctx, SRZ_E_INVALID, fn + ": d_par, d_gpar and d_work must be 4-byte aligned");
  if (int rc = check_overlaps(
          ctx, fn + " (d_gnrm, d_gpos, d_gbase, d_gmat, d_gpar, d_work against d_vis, d_nrm, d_pos, d_base, d_mat, d_par, d_gout)",
          {{d_gnrm, plane_bytes}, {d_gpos, plane_bytes}, {d_gbase, plane_bytes}, {d_gmat, mat_bytes}, {d_gpar, par_bytes},
           {d_gpar ? d_work : nullptr, need_work}},
          {{d_vis, vis_bytes}, {d_nrm, plane_bytes}, {d_pos, plane_bytes}, {d_base, plane_bytes}, {d_mat, mat_bytes}, {d_par, par_bytes},
           {d_gout, plane_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc;
  MicrofacetArgs a = microfacet_args(fs, d_vis, d_nrm, d_pos, d_base, d_mat, d_par, n_lights, par_frames, nullptr, flags);
  a.gout = (const float *)d_gout, a.gnrm = (float *)d_gnrm, a.gpos = (float *)d_gpos, a.gbase = (float *)d_gbase, a.gmat = (float *)d_gmat;
  a.work = d_gpar ? (float *)d_work : nullptr;
  launch_microfacet_grad(a, d_gpar, s);
  return end_pass(ctx);
}

// ---- image-based lighting: the reflection vector, the split-sum table, the combine
namespace {
ReflectArgs reflect_args(const srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const float *d_eye,
                         uint32_t par_frames, void *d_out, uint32_t flags) {
  ReflectArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.nrm = (const float *)d_nrm, a.pos = (const float *)d_pos, a.eye = d_eye;
  a.vis_stride = 4ull * plane, a.frame_stride = 4ull * plane, a.nrm_stride = 3ull * plane;
  a.eye_stride = par_frames == 1u ? 0ull : 3ull;
  a.flags_or = flags;
  return a;
}
// what srz_frameset_reflect and _reflect_grad check alike
int check_reflect(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, uint32_t par_frames, uint32_t flags) {
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  if (par_frames != 1u && par_frames != (uint32_t)fs->n_frames)
    return fail(ctx, SRZ_E_INVALID, fn + ": par_frames must be 1 or the set's frame count");
  return SRZ_OK;
}
IblArgs ibl_args(const srz_frameset *fs, const void *d_vis, const void *d_base, const void *d_mat, const void *d_nv, const void *d_irr,
                 const void *d_spec, const float *d_tab, uint32_t n, void *d_out, uint32_t flags) {
  IblArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.base = (const float *)d_base, a.mat = (const float *)d_mat, a.nv = (const float *)d_nv, a.irr = (const float *)d_irr;
  a.spec = (const float *)d_spec, a.tab = d_tab;
  a.vis_stride = 4ull * plane, a.frame_stride = 3ull * plane, a.mat_stride = 2ull * plane, a.nv_stride = plane;
  a.n = n;
  a.flags_or = flags;
  return a;
}
// what srz_frameset_ibl and _ibl_grad check alike
int check_ibl(srz_ctx *ctx, const std::string &fn, uint32_t n, uint32_t flags) {
  if (n < 2u || n > SRZ_BRDF_TABLE_MAX) return fail(ctx, SRZ_E_INVALID, fn + ": n must be 2 .. SRZ_BRDF_TABLE_MAX");
  return check_pass_flags(ctx, fn, flags);
}
} // namespace

int srz_frameset_reflect(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const float *d_eye,
                         uint32_t par_frames, void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_reflect");
  if (!fs || !d_vis || !d_nrm || !d_pos || !d_eye || !d_out)
    return fail(ctx, SRZ_E_INVALID,
                fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_nrm ? "d_nrm" : !d_pos ? "d_pos" : !d_eye ? "d_eye" : "d_out"));
  if (int rc = check_reflect(ctx, fs, fn, par_frames, flags)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, 4u), plane_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u),
               vis_bytes = srz_frameset_out_bytes(ctx, fs), eye_bytes = (size_t)par_frames * 3u * sizeof(float);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_vis, d_nrm, d_pos, d_out}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_nrm, d_pos, d_out) must be 16-byte aligned");
  if (!aligned<4>({d_eye})) return fail(ctx, SRZ_E_INVALID, fn + ": d_eye must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn + " (d_out against d_vis, d_nrm, d_pos, d_eye)", {{d_out, need}},
                              {{d_vis, vis_bytes}, {d_nrm, plane_bytes}, {d_pos, plane_bytes}, {d_eye, eye_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_light: caller data only)
  launch_reflect(reflect_args(fs, d_vis, d_nrm, d_pos, d_eye, par_frames, d_out, flags), s);
  return end_pass(ctx);
}

int srz_frameset_reflect_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_pos, const float *d_eye,
                              uint32_t par_frames, const void *d_gout, void *d_gnrm, void *d_gpos, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_reflect_grad");
  if (!fs || !d_vis || !d_nrm || !d_pos || !d_eye || !d_gout)
    return fail(ctx, SRZ_E_INVALID,
                fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_nrm ? "d_nrm" : !d_pos ? "d_pos" : !d_eye ? "d_eye" : "d_gout"));
  if (!d_gnrm && !d_gpos) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gnrm nor d_gpos is asked for");
  if (int rc = check_reflect(ctx, fs, fn, par_frames, flags)) return rc;
  const size_t gout_bytes = srz_frameset_interpolate_bytes(ctx, fs, 4u), plane_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u),
               vis_bytes = srz_frameset_out_bytes(ctx, fs), eye_bytes = (size_t)par_frames * 3u * sizeof(float);
  if (!aligned<16>({d_vis, d_nrm, d_pos, d_gout, d_gnrm, d_gpos}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_nrm, d_pos, d_gout, d_gnrm, d_gpos) must be 16-byte aligned");
  if (!aligned<4>({d_eye})) return fail(ctx, SRZ_E_INVALID, fn + ": d_eye must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn + " (d_gnrm, d_gpos against d_vis, d_nrm, d_pos, d_eye, d_gout)",
                              {{d_gnrm, plane_bytes}, {d_gpos, plane_bytes}},
                              {{d_vis, vis_bytes}, {d_nrm, plane_bytes}, {d_pos, plane_bytes}, {d_eye, eye_bytes}, {d_gout, gout_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc;
  ReflectArgs a = reflect_args(fs, d_vis, d_nrm, d_pos, d_eye, par_frames, nullptr, flags);
  a.gout = (const float *)d_gout, a.gnrm = (float *)d_gnrm, a.gpos = (float *)d_gpos;
  launch_reflect_grad(a, s);
  return end_pass(ctx);
}

int srz_brdf_table(srz_ctx *ctx, float *d_tab, size_t tab_bytes, uint32_t n, uint32_t m, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_brdf_table");
  if (!d_tab) return fail(ctx, SRZ_E_INVALID, fn + ": null d_tab");
  if (n < 2u || n > SRZ_BRDF_TABLE_MAX) return fail(ctx, SRZ_E_INVALID, fn + ": n must be 2 .. SRZ_BRDF_TABLE_MAX");
  if (m == 0u || m > 256u) return fail(ctx, SRZ_E_INVALID, fn + ": m must be 1 .. 256");
  if (tab_bytes < (size_t)n * n * 2u * sizeof(float)) return fail(ctx, SRZ_E_INVALID, fn + ": tab_bytes is too small for d_tab");
  if (!aligned<4>({d_tab})) return fail(ctx, SRZ_E_INVALID, fn + ": d_tab must be 4-byte aligned");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  launch_brdf_table(d_tab, n, m, pick_stream(ctx, stream));
  return end_pass(ctx);
}

int srz_frameset_ibl(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_base, const void *d_mat, const void *d_nv,
                     const void *d_irr, const void *d_spec, const float *d_tab, uint32_t n, void *d_out, size_t out_bytes, uint32_t flags,
                     void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_ibl");
  if (!fs || !d_vis || !d_mat || !d_nv || !d_irr || !d_spec || !d_tab || !d_out)
    return fail(ctx, SRZ_E_INVALID,
                fn + ": null " +
                    (!fs ? "frameset" : !d_vis ? "d_vis" : !d_mat ? "d_mat" : !d_nv ? "d_nv" : !d_irr ? "d_irr" : !d_spec ? "d_spec" : !d_tab ? "d_tab" : "d_out"));
  if (int rc = check_ibl(ctx, fn, n, flags)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, 3u), mat_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u),
               nv_bytes = srz_frameset_interpolate_bytes(ctx, fs, 1u), vis_bytes = srz_frameset_out_bytes(ctx, fs),
               tab_bytes = (size_t)n * n * 2u * sizeof(float);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_vis, d_base, d_mat, d_nv, d_irr, d_spec, d_out}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_base, d_mat, d_nv, d_irr, d_spec, d_out) must be 16-byte aligned");
  if (!aligned<4>({d_tab})) return fail(ctx, SRZ_E_INVALID, fn + ": d_tab must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn + " (d_out against d_vis, d_base, d_mat, d_nv, d_irr, d_spec, d_tab)", {{d_out, need}},
                              {{d_vis, vis_bytes}, {d_base, need}, {d_mat, mat_bytes}, {d_nv, nv_bytes}, {d_irr, need}, {d_spec, need},
                               {d_tab, tab_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_light: caller data only)
  launch_ibl(ibl_args(fs, d_vis, d_base, d_mat, d_nv, d_irr, d_spec, d_tab, n, d_out, flags), s);
  return end_pass(ctx);
}

int srz_frameset_ibl_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_base, const void *d_mat, const void *d_nv,
                          const void *d_irr, const void *d_spec, const float *d_tab, uint32_t n, const void *d_gout, void *d_gbase,
                          void *d_gmat, void *d_gnv, void *d_girr, void *d_gspec, float *d_gtab, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_ibl_grad");
  if (!fs || !d_vis || !d_mat || !d_nv || !d_irr || !d_spec || !d_tab || !d_gout)
    return fail(ctx, SRZ_E_INVALID,
                fn + ": null " +
                    (!fs ? "frameset" : !d_vis ? "d_vis" : !d_mat ? "d_mat" : !d_nv ? "d_nv" : !d_irr ? "d_irr" : !d_spec ? "d_spec" : !d_tab ? "d_tab" : "d_gout"));
  if (!d_gbase && !d_gmat && !d_gnv && !d_girr && !d_gspec && !d_gtab)
    return fail(ctx, SRZ_E_INVALID, fn + ": none of d_gbase, d_gmat, d_gnv, d_girr, d_gspec, d_gtab is asked for");
  if (d_gbase && !d_base) return fail(ctx, SRZ_E_INVALID, fn + ": d_gbase needs d_base");
  if (int rc = check_ibl(ctx, fn, n, flags)) return rc;
  const size_t plane_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u), mat_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u),
               nv_bytes = srz_frameset_interpolate_bytes(ctx, fs, 1u), vis_bytes = srz_frameset_out_bytes(ctx, fs),
               tab_bytes = (size_t)n * n * 2u * sizeof(float);
  if (!aligned<16>({d_vis, d_base, d_mat, d_nv, d_irr, d_spec, d_gout, d_gbase, d_gmat, d_gnv, d_girr, d_gspec}))
    return fail(ctx, SRZ_E_INVALID,
                fn + ": the plane buffers (d_vis, d_base, d_mat, d_nv, d_irr, d_spec, d_gout, d_gbase, d_gmat, d_gnv, d_girr, d_gspec) must be "
                     "16-byte aligned");
  if (!aligned<4>({d_tab, d_gtab})) return fail(ctx, SRZ_E_INVALID, fn + ": d_tab and d_gtab must be 4-byte aligned");
  if (int rc = check_overlaps(
          ctx, fn + " (d_gbase, d_gmat, d_gnv, d_girr, d_gspec, d_gtab against d_vis, d_base, d_mat, d_nv, d_irr, d_spec, d_tab, d_gout)",
          {{d_gbase, plane_bytes}, {d_gmat, mat_bytes}, {d_gnv, nv_bytes}, {d_girr, plane_bytes}, {d_gspec, plane_bytes}, {d_gtab, tab_bytes}},
          {{d_vis, vis_bytes}, {d_base, plane_bytes}, {d_mat, mat_bytes}, {d_nv, nv_bytes}, {d_irr, plane_bytes}, {d_spec, plane_bytes},
           {d_tab, tab_bytes}, {d_gout, plane_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc;
  IblArgs a = ibl_args(fs, d_vis, d_base, d_mat, d_nv, d_irr, d_spec, d_tab, n, nullptr, flags);
  a.gout = (const float *)d_gout, a.gbase = (float *)d_gbase, a.gmat = (float *)d_gmat, a.gnv = (float *)d_gnv;
  a.girr = (float *)d_girr, a.gspec = (float *)d_gspec, a.gtab = d_gtab;
  launch_ibl_grad(a, s);
  return end_pass(ctx);
}

namespace {
NormalMapArgs normal_map_args(const srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_tan, const void *d_m, void *d_out,
                              uint32_t flags) {
  NormalMapArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.nrm = (const float *)d_nrm, a.tan = (const float *)d_tan, a.m = (const float *)d_m;
  a.vis_stride = 4ull * plane, a.frame_stride = 3ull * plane, a.tan_stride = 4ull * plane;
  a.flags_or = flags;
  return a;
}
} // namespace

int srz_frameset_normal_map(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_tan, const void *d_m,
                            void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_normal_map");
  if (!fs || !d_vis || !d_nrm || !d_tan || !d_m || !d_out)
    return fail(ctx, SRZ_E_INVALID,
                fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_nrm ? "d_nrm" : !d_tan ? "d_tan" : !d_m ? "d_m" : "d_out"));
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, 3u), tan_bytes = srz_frameset_interpolate_bytes(ctx, fs, 4u),
               vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_vis, d_nrm, d_tan, d_m, d_out}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_nrm, d_tan, d_m, d_out) must be 16-byte aligned");
  if (int rc = check_overlaps(ctx, fn + " (d_out against d_vis, d_nrm, d_tan, d_m)", {{d_out, need}},
                              {{d_vis, vis_bytes}, {d_nrm, need}, {d_tan, tan_bytes}, {d_m, need}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_light: caller data only)
  launch_normal_map(normal_map_args(fs, d_vis, d_nrm, d_tan, d_m, d_out, flags), s);
  return end_pass(ctx);
}

int srz_frameset_normal_map_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const void *d_tan, const void *d_m,
                                 const void *d_gout, void *d_gnrm, void *d_gtan, void *d_gm, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_normal_map_grad");
  if (!fs || !d_vis || !d_nrm || !d_tan || !d_m || !d_gout)
    return fail(ctx, SRZ_E_INVALID,
                fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_nrm ? "d_nrm" : !d_tan ? "d_tan" : !d_m ? "d_m" : "d_gout"));
  if (!d_gnrm && !d_gtan && !d_gm) return fail(ctx, SRZ_E_INVALID, fn + ": none of d_gnrm, d_gtan, d_gm is asked for");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  const size_t b3 = srz_frameset_interpolate_bytes(ctx, fs, 3u), b4 = srz_frameset_interpolate_bytes(ctx, fs, 4u),
               vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (!aligned<16>({d_vis, d_nrm, d_tan, d_m, d_gout, d_gnrm, d_gtan, d_gm}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_nrm, d_tan, d_m, d_gout, d_gnrm, d_gtan, d_gm) must be 16-byte aligned");
  if (int rc = check_overlaps(ctx, fn + " (d_gnrm, d_gtan, d_gm against d_vis, d_nrm, d_tan, d_m, d_gout)",
                              {{d_gnrm, b3}, {d_gtan, b4}, {d_gm, b3}}, {{d_vis, vis_bytes}, {d_nrm, b3}, {d_tan, b4}, {d_m, b3}, {d_gout, b3}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc;
  NormalMapArgs a = normal_map_args(fs, d_vis, d_nrm, d_tan, d_m, nullptr, flags);
  a.gout = (const float *)d_gout, a.gnrm = (float *)d_gnrm, a.gtan = (float *)d_gtan, a.gm = (float *)d_gm;
  launch_normal_map_grad(a, s);
  return end_pass(ctx);
}

namespace {
// check_overlaps for a number of buffers known at run time (the composite's layers): the same rule, the same messages
int check_overlaps_n(srz_ctx *ctx, const std::string &fn, const std::vector<Range> &outs, const std::vector<Range> &ins) {
  for (size_t o = 0; o < outs.size(); ++o) {
    for (const Range &i : ins)
      if (ranges_overlap(outs[o], i)) return fail(ctx, SRZ_E_INVALID, fn + ": an output overlaps an input");
    for (size_t p = o + 1; p < outs.size(); ++p)
      if (ranges_overlap(outs[o], outs[p])) return fail(ctx, SRZ_E_INVALID, fn + ": two outputs overlap");
  }
  return SRZ_OK;
}
// what srz_frameset_composite and _composite_grad check alike behind their null ctx, and the Args they share.  *ins: every input's
// range, for the caller's overlap check
int check_composite(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, const srz_composite_layer *layers, uint32_t n_layers,
                    uint32_t n_ch, const void *d_bg, uint32_t want_through, uint32_t flags, std::vector<Range> *ins) {
  if (!fs || !layers) return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : "layers"));
  if (n_layers == 0u || n_layers > (uint32_t)SRZ_COMPOSITE_MAX) return fail(ctx, SRZ_E_INVALID, fn + ": n_layers must be 1 .. SRZ_COMPOSITE_MAX");
  if (n_ch == 0u || n_ch > SRZ_ATTR_MAX_CH) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. SRZ_ATTR_MAX_CH");
  if (want_through > 1u) return fail(ctx, SRZ_E_INVALID, fn + ": want_through must be 0 or 1");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, const_cast<srz_frameset *>(fs));
  const size_t col_bytes = srz_frameset_interpolate_bytes(ctx, const_cast<srz_frameset *>(fs), n_ch);
  const size_t one_bytes = srz_frameset_interpolate_bytes(ctx, const_cast<srz_frameset *>(fs), 1u);
  for (uint32_t k = 0; k < n_layers; ++k) {
    const srz_composite_layer &l = layers[k];
    if (!l.vis || !l.color) return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!l.vis ? "vis" : "color") + " in layer " + std::to_string(k));
    if (!aligned<16>({l.vis, l.color, l.alpha}))
      return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (every layer's vis, color, alpha) must be 16-byte aligned");
    ins->push_back({l.vis, vis_bytes}), ins->push_back({l.color, col_bytes}), ins->push_back({l.alpha, one_bytes});
  }
  ins->push_back({d_bg, col_bytes});
  return SRZ_OK;
}
CompositeArgs composite_args(const srz_frameset *fs, const srz_composite_layer *layers, uint32_t n_layers, uint32_t n_ch, const void *d_bg,
                             uint32_t want_through, void *d_out, uint32_t flags) {
  CompositeArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, layers[0].vis, d_out);
  for (uint32_t k = 0; k < n_layers; ++k) {
    a.lvis[k] = (const float *)layers[k].vis, a.col[k] = (const float *)layers[k].color, a.alpha[k] = (const float *)layers[k].alpha;
    a.opacity[k] = layers[k].opacity;
  }
  a.bg = (const float *)d_bg;
  a.vis_stride = 4ull * plane, a.frame_stride = (uint64_t)(n_ch + want_through) * plane, a.col_stride = (uint64_t)n_ch * plane;
  a.n_layers = n_layers, a.n_ch = n_ch, a.through = want_through;
  a.flags_or = flags;
  return a;
}
} // namespace

int srz_frameset_composite(srz_ctx *ctx, srz_frameset *fs, const srz_composite_layer *layers, uint32_t n_layers, uint32_t n_ch,
                           const void *d_bg, uint32_t want_through, void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_composite");
  std::vector<Range> ins;
  if (int rc = check_composite(ctx, fs, fn, layers, n_layers, n_ch, d_bg, want_through, flags, &ins)) return rc;
  if (!d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null d_out");
  // (n_ch + 1 may be one above SRZ_ATTR_MAX_CH, where srz_frameset_interpolate_bytes answers 0: the bytes by planes of one)
  const size_t need = (size_t)(n_ch + want_through) * srz_frameset_interpolate_bytes(ctx, fs, 1u);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_bg, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_bg, d_out) must be 16-byte aligned");
  if (int rc = check_overlaps_n(ctx, fn + " (d_out against every layer's vis, color, alpha and d_bg)", std::vector<Range>{{d_out, need}}, ins))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_normal_map: caller data only)
  launch_composite(composite_args(fs, layers, n_layers, n_ch, d_bg, want_through, d_out, flags), s);
  return end_pass(ctx);
}

int srz_frameset_composite_grad(srz_ctx *ctx, srz_frameset *fs, const srz_composite_layer *layers, uint32_t n_layers, uint32_t n_ch,
                                const void *d_bg, uint32_t want_through, const void *d_gout, void *const *d_gcolor,
                                void *const *d_galpha, void *d_gbg, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_composite_grad");
  std::vector<Range> ins;
  if (int rc = check_composite(ctx, fs, fn, layers, n_layers, n_ch, d_bg, want_through, flags, &ins)) return rc;
  if (!d_gout) return fail(ctx, SRZ_E_INVALID, fn + ": null d_gout");
  const size_t one_bytes = srz_frameset_interpolate_bytes(ctx, fs, 1u), col_bytes = (size_t)n_ch * one_bytes;
  std::vector<Range> outs;
  const void *any = d_gbg;
  bool misaligned = !aligned<16>({d_bg, d_gout, d_gbg});
  for (uint32_t k = 0; k < n_layers; ++k) {
    void *gc = d_gcolor ? d_gcolor[k] : nullptr, *ga = d_galpha ? d_galpha[k] : nullptr;
    if (gc) any = gc;
    if (ga) any = ga;
    misaligned = misaligned || !aligned<16>({gc, ga});
    outs.push_back({gc, col_bytes}), outs.push_back({ga, one_bytes});
  }
  outs.push_back({d_gbg, col_bytes});
  if (!any) return fail(ctx, SRZ_E_INVALID, fn + ": none of d_gcolor, d_galpha, d_gbg is asked for");
  if (d_gbg && !d_bg) return fail(ctx, SRZ_E_INVALID, fn + ": d_gbg needs d_bg");
  if (misaligned)
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_bg, d_gout, d_gcolor[k], d_galpha[k], d_gbg) must be 16-byte aligned");
  ins.push_back({d_gout, (size_t)(n_ch + want_through) * one_bytes});
  if (int rc = check_overlaps_n(ctx, fn + " (d_gcolor, d_galpha, d_gbg against every layer's vis, color, alpha, d_bg and d_gout)", outs, ins))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc;
  CompositeArgs a = composite_args(fs, layers, n_layers, n_ch, d_bg, want_through, nullptr, flags);
  a.gout = (const float *)d_gout, a.gbg = (float *)d_gbg;
  for (uint32_t k = 0; k < n_layers; ++k) {
    a.gcol[k] = d_gcolor ? (float *)d_gcolor[k] : nullptr, a.galpha[k] = d_galpha ? (float *)d_galpha[k] : nullptr;
    if (a.galpha[k]) a.want_d = 1u;
  }
  launch_composite_grad(a, s);
  return end_pass(ctx);
}

namespace {
// what srz_frameset_texture_set and _texture_set_grad check alike behind their nulls: the counts, then every slot as
// srz_frameset_texture checks its texture (check_texture, not restated).  need_tex: a slot's d_tex may not be null.  *ins gets the
// map's and every texture's range, *tex_bytes every slot's bytes
int check_texset(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, const srz_texset_slot *slots, uint32_t n_slots,
                 const uint8_t *d_batch_slot, uint32_t n_batch_slot, uint32_t n_ch, uint32_t flags, bool need_tex, std::vector<Range> *ins,
                 std::vector<size_t> *tex_bytes) {
  if (n_slots == 0u || n_slots > SRZ_TEXSET_MAX) return fail(ctx, SRZ_E_INVALID, fn + ": n_slots must be 1 .. SRZ_TEXSET_MAX");
  if (n_batch_slot == 0u || n_batch_slot > 65536u) return fail(ctx, SRZ_E_INVALID, fn + ": n_batch_slot must be 1 .. 65536");
  ins->push_back({d_batch_slot, (size_t)n_batch_slot});
  for (uint32_t k = 0; k < n_slots; ++k) {
    const srz_texset_slot &sl = slots[k];
    size_t bytes = 0;
    if (int rc = check_texture(ctx, fs, fn + " (slot " + std::to_string(k) + ")", sl.tex_w, sl.tex_h, n_ch, sl.tex_frames, sl.mode, flags, &bytes))
      return rc;
    if (need_tex && !sl.d_tex) return fail(ctx, SRZ_E_INVALID, fn + ": null d_tex in slot " + std::to_string(k));
    if (!aligned<4>({sl.d_tex, sl.d_gtex}))
      return fail(ctx, SRZ_E_INVALID, fn + ": every slot's texture and its gradient must be 4-byte aligned");
    ins->push_back({sl.d_tex, bytes}), tex_bytes->push_back(bytes);
  }
  return SRZ_OK;
}
TexSetArgs texset_args(const srz_frameset *fs, const void *d_vis, const void *d_uv, const srz_texset_slot *slots, uint32_t n_slots,
                       const uint8_t *d_batch_slot, uint32_t n_batch_slot, uint32_t n_ch, uint32_t out_planes, void *d_out, uint32_t flags) {
  TexSetArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.uv = (const float *)d_uv, a.tri_batch = fs->d_tri_batch, a.batch_slot = d_batch_slot;
  for (uint32_t k = 0; k < n_slots; ++k) {
    const srz_texset_slot &sl = slots[k];
    a.tex[k] = sl.d_tex, a.tex_w[k] = sl.tex_w, a.tex_h[k] = sl.tex_h;
    a.tex_frame_stride[k] = sl.tex_frames == 1u ? 0ull : (uint64_t)sl.tex_h * sl.tex_w * n_ch;
    if (sl.mode == SRZ_TEX_WRAP) a.wrap_mask |= 1u << k;
  }
  a.vis_stride = 4ull * plane, a.frame_stride = out_planes * plane, a.uv_stride = 2ull * plane, a.gout_stride = n_ch * plane;
  a.n_slots = n_slots, a.n_batch_slot = n_batch_slot, a.n_ch = n_ch;
  a.flags_or = flags;
  return a;
}
} // namespace

int srz_frameset_texture_set(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_uv, const srz_texset_slot *slots,
                             uint32_t n_slots, const uint8_t *d_batch_slot, uint32_t n_batch_slot, uint32_t n_ch, void *d_out,
                             size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_texture_set");
  if (!fs || !d_vis || !d_uv || !slots || !d_batch_slot || !d_out)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_uv ? "d_uv" : !slots ? "slots" : !d_batch_slot ? "d_batch_slot" : "d_out"));
  std::vector<Range> ins;
  std::vector<size_t> tex_bytes;
  if (int rc = check_texset(ctx, fs, fn, slots, n_slots, d_batch_slot, n_batch_slot, n_ch, flags, true, &ins, &tex_bytes)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, n_ch), uv_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_vis, d_uv, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_uv, d_out) must be 16-byte aligned");
  ins.push_back({d_vis, srz_frameset_out_bytes(ctx, fs)}), ins.push_back({d_uv, uv_bytes});
  if (int rc = check_overlaps_n(ctx, fn + " (d_out against d_vis, d_uv, the map and every slot's d_tex)", std::vector<Range>{{d_out, need}}, ins))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture)
  launch_tex_set(texset_args(fs, d_vis, d_uv, slots, n_slots, d_batch_slot, n_batch_slot, n_ch, n_ch, d_out, flags), s);
  return end_pass(ctx);
}

int srz_frameset_texture_set_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_uv, const void *d_gout,
                                  const srz_texset_slot *slots, uint32_t n_slots, const uint8_t *d_batch_slot, uint32_t n_batch_slot,
                                  uint32_t n_ch, void *d_guv, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_texture_set_grad");
  if (!fs || !d_vis || !d_uv || !d_gout || !slots || !d_batch_slot)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_uv ? "d_uv" : !d_gout ? "d_gout" : !slots ? "slots" : "d_batch_slot"));
  std::vector<Range> ins;
  std::vector<size_t> tex_bytes;
  if (int rc = check_texset(ctx, fs, fn, slots, n_slots, d_batch_slot, n_batch_slot, n_ch, flags, d_guv != nullptr, &ins, &tex_bytes)) return rc;
  const size_t gout_bytes = srz_frameset_interpolate_bytes(ctx, fs, n_ch), uv_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u);
  std::vector<Range> outs;
  bool any_gtex = false;
  for (uint32_t k = 0; k < n_slots; ++k) any_gtex = any_gtex || slots[k].d_gtex, outs.push_back({slots[k].d_gtex, tex_bytes[k]});
  outs.push_back({d_guv, uv_bytes});
  if (!any_gtex && !d_guv) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_guv nor any slot's d_gtex is asked for");
  if (!aligned<16>({d_vis, d_uv, d_gout, d_guv}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_uv, d_gout, d_guv) must be 16-byte aligned");
  ins.push_back({d_vis, srz_frameset_out_bytes(ctx, fs)}), ins.push_back({d_uv, uv_bytes}), ins.push_back({d_gout, gout_bytes});
  if (int rc = check_overlaps_n(ctx, fn + " (d_guv and every slot's d_gtex against d_vis, d_uv, d_gout, the map and every slot's d_tex)", outs, ins))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture)
  TexSetArgs a = texset_args(fs, d_vis, d_uv, slots, n_slots, d_batch_slot, n_batch_slot, n_ch, 2u, d_guv, flags);
  a.gout = (const float *)d_gout, a.want_tex = any_gtex ? 1u : 0u;
  for (uint32_t k = 0; k < n_slots; ++k) a.gtex[k] = slots[k].d_gtex;
  launch_tex_set_grad(a, s);
  return end_pass(ctx);
}

uint32_t srz_texture_mip_levels(uint32_t tex_w, uint32_t tex_h) {
  if (tex_w == 0u || tex_w > SRZ_TEX_MAX_SIZE || tex_h == 0u || tex_h > SRZ_TEX_MAX_SIZE) return 0u;
  uint32_t n = 1u;
  while ((tex_w > 1u || tex_h > 1u) && (tex_w % 2u == 0u || tex_w == 1u) && (tex_h % 2u == 0u || tex_h == 1u))
    tex_w = std::max(1u, tex_w / 2u), tex_h = std::max(1u, tex_h / 2u), ++n;
  return n;
}

size_t srz_texture_mip_bytes(uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels) {
  const uint32_t most = srz_texture_mip_levels(tex_w, tex_h);
  if (most == 0u || n_levels <= 1u || n_levels > most || n_ch == 0u || n_ch > SRZ_ATTR_MAX_CH || tex_frames == 0u || tex_frames > MIP_MAX_FRAMES)
    return 0;
  return (size_t)mip_texels_before(tex_w, tex_h, n_levels) * tex_frames * n_ch * sizeof(float);
}

int srz_texture_mip_build(srz_ctx *ctx, const float *d_tex, uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames,
                          uint32_t n_levels, float *d_mip, size_t mip_bytes, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_texture_mip_build");
  if (int rc = check_mip(ctx, fn, tex_w, tex_h, n_ch, tex_frames, n_levels, mip_bytes, d_tex, d_mip)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick_stream(ctx, stream);
  const float *src = d_tex;
  float *dst = d_mip;
  for (uint32_t l = 1; l < n_levels; ++l) { // each level from the level above it
    const uint32_t sw = mip_extent(tex_w, l - 1u), sh = mip_extent(tex_h, l - 1u), dw = mip_extent(tex_w, l), dh = mip_extent(tex_h, l);
    launch_mip_build(src, dst, sw, sh, dw, dh, n_ch, tex_frames, s);
    src = dst, dst += (size_t)tex_frames * dh * dw * n_ch;
  }
  return end_pass(ctx);
}

int srz_texture_mip_fold(srz_ctx *ctx, const float *d_gmip, size_t mip_bytes, uint32_t tex_w, uint32_t tex_h, uint32_t n_ch,
                         uint32_t tex_frames, uint32_t n_levels, float *d_gtex, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_texture_mip_fold");
  if (int rc = check_mip(ctx, fn, tex_w, tex_h, n_ch, tex_frames, n_levels, mip_bytes, d_gtex, d_gmip)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick_stream(ctx, stream);
  if (n_levels > 1u) launch_mip_fold(d_gmip, d_gtex, tex_w, tex_h, n_ch, tex_frames, n_levels, s);
  return end_pass(ctx);
}

int srz_frameset_interpolate_deriv(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_attr, uint32_t n_ch,
                                   uint32_t attr_frames, uint32_t attr_tris, void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_interpolate_deriv");
  if (!fs || !d_vis || !d_attr || !d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / attributes / output");
  if (n_ch > SRZ_ATTR_MAX_CH / 2u) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. SRZ_ATTR_MAX_CH / 2");
  size_t attr_bytes = 0;
  if (int rc = check_interp(ctx, fs, fn, n_ch, attr_frames, attr_tris, flags, &attr_bytes)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, 2u * n_ch), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (!aligned<16>({d_vis, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": buffers must be 16-byte aligned");
  if (!aligned<4>({d_attr})) return fail(ctx, SRZ_E_INVALID, fn + ": the attributes must be 4-byte aligned");
  if (ranges_overlap({d_out, need}, {d_vis, vis_bytes}) || ranges_overlap({d_out, need}, {d_attr, attr_bytes}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the output overlaps the visibility buffer or the attributes");
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, PASS_VERTEX, &s)) return rc; // (the set's positions, as srz_frameset_position_grad)
  InterpDerivArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  fill_positions(a, fs);
  a.attr = d_attr;
  a.vis_stride = 4ull * plane, a.frame_stride = 2ull * n_ch * plane;
  a.attr_frame_stride = attr_frames == 1u ? 0ull : (uint64_t)attr_tris * 3u * n_ch;
  a.n_ch = n_ch;
  a.flags_or = flags;
  launch_interp_deriv(a, s);
  return end_pass(ctx);
}

// what srz_frameset_perspective, _perspective_grad and _interpolate_deriv_persp check of q alike; its bytes in *q_bytes
static int check_persp_q(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, uint32_t q_frames, uint32_t q_tris, size_t *q_bytes) {
  if (q_frames != 1u && q_frames != (uint32_t)fs->n_frames) return fail(ctx, SRZ_E_INVALID, fn + ": q_frames must be 1 or the set's frame count");
  if (int rc = check_tri_count(ctx, fs, fn, "q_tris", q_tris)) return rc;
  *q_bytes = (size_t)q_frames * q_tris * 3u * sizeof(float);
  return SRZ_OK;
}
static PerspArgs persp_args(const srz_frameset *fs, const void *d_vis, const float *d_q, uint32_t q_frames, uint32_t q_tris, uint32_t out_planes,
                            void *d_out, uint32_t flags) {
  PerspArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.q = d_q;
  a.vis_stride = 4ull * plane, a.frame_stride = out_planes * plane;
  a.q_frame_stride = q_frames == 1u ? 0ull : (uint64_t)q_tris * 3u;
  a.flags_or = flags;
  return a;
}

int srz_frameset_perspective(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_q, uint32_t q_frames, uint32_t q_tris,
                             void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_perspective");
  if (!fs || !d_vis || !d_q || !d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / q / output");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  size_t q_bytes = 0;
  if (int rc = check_persp_q(ctx, fs, fn, q_frames, q_tris, &q_bytes)) return rc;
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < vis_bytes) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (!aligned<16>({d_vis, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": buffers must be 16-byte aligned");
  if (!aligned<4>({d_q})) return fail(ctx, SRZ_E_INVALID, fn + ": q must be 4-byte aligned");
  if (ranges_overlap({d_out, vis_bytes}, {d_vis, vis_bytes}) || ranges_overlap({d_out, vis_bytes}, {d_q, q_bytes}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the output overlaps the visibility buffer or q");
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (the caller's q, not the set's triangles: no vertex stage)
  launch_persp(persp_args(fs, d_vis, d_q, q_frames, q_tris, 4u, d_out, flags), s);
  return end_pass(ctx);
}

int srz_frameset_perspective_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_q, uint32_t q_frames, uint32_t q_tris,
                                  const void *d_gbary_p, void *d_gbary, float *d_gq, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_perspective_grad");
  if (!fs || !d_vis || !d_q || !d_gbary_p) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / q / gradient planes");
  if (!d_gbary && !d_gq) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gbary nor d_gq is asked for");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  size_t q_bytes = 0;
  if (int rc = check_persp_q(ctx, fs, fn, q_frames, q_tris, &q_bytes)) return rc;
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs), two_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u);
  if (!aligned<16>({d_vis, d_gbary_p, d_gbary})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers must be 16-byte aligned");
  if (!aligned<4>({d_q, d_gq})) return fail(ctx, SRZ_E_INVALID, fn + ": q and its gradient must be 4-byte aligned");
  if (int rc = check_grad_overlap(ctx, fn, {{d_gq, q_bytes}, {d_gbary, two_bytes}}, {{d_vis, vis_bytes}, {d_gbary_p, two_bytes}, {d_q, q_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_perspective)
  PerspArgs a = persp_args(fs, d_vis, d_q, q_frames, q_tris, 2u, d_gbary, flags);
  a.gbary_p = (const float *)d_gbary_p, a.gq = d_gq;
  launch_persp_grad(a, s);
  return end_pass(ctx);
}

int srz_frameset_interpolate_deriv_persp(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const float *d_q, uint32_t q_frames,
                                         uint32_t q_tris, const float *d_attr, uint32_t n_ch, uint32_t attr_frames, uint32_t attr_tris,
                                         void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_interpolate_deriv_persp");
  if (!fs || !d_vis || !d_q || !d_attr || !d_out)
    return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / q / attributes / output");
  if (n_ch > SRZ_ATTR_MAX_CH / 2u) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. SRZ_ATTR_MAX_CH / 2");
  size_t attr_bytes = 0, q_bytes = 0;
  if (int rc = check_interp(ctx, fs, fn, n_ch, attr_frames, attr_tris, flags, &attr_bytes)) return rc;
  if (int rc = check_persp_q(ctx, fs, fn, q_frames, q_tris, &q_bytes)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, 2u * n_ch), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (!aligned<16>({d_vis, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": buffers must be 16-byte aligned");
  if (!aligned<4>({d_attr, d_q})) return fail(ctx, SRZ_E_INVALID, fn + ": the attributes and q must be 4-byte aligned");
  if (ranges_overlap({d_out, need}, {d_vis, vis_bytes}) || ranges_overlap({d_out, need}, {d_attr, attr_bytes}) ||
      ranges_overlap({d_out, need}, {d_q, q_bytes}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the output overlaps the visibility buffer, the attributes or q");
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, PASS_VERTEX, &s)) return rc; // (the set's positions, as srz_frameset_interpolate_deriv)
  PerspDerivArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  fill_positions(a, fs);
  a.attr = d_attr, a.q = d_q;
  a.vis_stride = 4ull * plane, a.frame_stride = 2ull * n_ch * plane;
  a.attr_frame_stride = attr_frames == 1u ? 0ull : (uint64_t)attr_tris * 3u * n_ch;
  a.q_frame_stride = q_frames == 1u ? 0ull : (uint64_t)q_tris * 3u;
  a.n_ch = n_ch;
  a.flags_or = flags;
  launch_interp_deriv_persp(a, s);
  return end_pass(ctx);
}

int srz_frameset_texture_mip(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_uv, const void *d_uvd, const float *d_tex,
                             uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t mode, const float *d_mip,
                             uint32_t n_levels, void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_texture_mip");
  if (!fs || !d_vis || !d_uv || !d_tex || !d_out) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / uv / texture / output");
  size_t tex_bytes = 0, mip_bytes = 0;
  if (int rc = check_texture(ctx, fs, fn, tex_w, tex_h, n_ch, tex_frames, mode, flags, &tex_bytes)) return rc;
  if (int rc = check_tex_mip(ctx, fn, tex_w, tex_h, n_ch, tex_frames, n_levels, d_uvd, &mip_bytes)) return rc;
  if (n_levels > 1u && !d_mip) return fail(ctx, SRZ_E_INVALID, fn + ": n_levels > 1 needs the pyramid");
  if (n_levels == 1u) d_uvd = nullptr, d_mip = nullptr; // (not read: they take no part in the checks either)
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, n_ch), uv_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u);
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs); // (the derivative planes: four per frame, the visibility buffer's size)
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": output buffer too small");
  if (!aligned<16>({d_vis, d_uv, d_uvd, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers must be 16-byte aligned");
  if (!aligned<4>({d_tex, d_mip})) return fail(ctx, SRZ_E_INVALID, fn + ": the texture and the pyramid must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn, {{d_out, need}},
                              {{d_vis, vis_bytes}, {d_uv, uv_bytes}, {d_uvd, vis_bytes}, {d_tex, tex_bytes}, {d_mip, mip_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture)
  launch_tex_mip(texture_mip_args(fs, d_vis, d_uv, d_uvd, d_tex, d_mip, tex_w, tex_h, n_ch, tex_frames, mode, n_levels, n_ch, d_out, flags), s);
  return end_pass(ctx);
}

int srz_frameset_texture_mip_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_uv, const void *d_uvd, const void *d_gout,
                                  const float *d_tex, const float *d_mip, uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames,
                                  uint32_t mode, uint32_t n_levels, float *d_gtex, float *d_gmip, void *d_guv, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_texture_mip_grad");
  if (!fs || !d_vis || !d_uv || !d_gout) return fail(ctx, SRZ_E_INVALID, fn + ": null frameset / visibility buffer / uv / output gradient");
  if (!d_gtex && !d_gmip && !d_guv) return fail(ctx, SRZ_E_INVALID, fn + ": neither the texel gradients nor d_guv is asked for");
  if (d_guv && !d_tex) return fail(ctx, SRZ_E_INVALID, fn + ": d_guv needs the texture");
  size_t tex_bytes = 0, mip_bytes = 0;
  if (int rc = check_texture(ctx, fs, fn, tex_w, tex_h, n_ch, tex_frames, mode, flags, &tex_bytes)) return rc;
  if (int rc = check_tex_mip(ctx, fn, tex_w, tex_h, n_ch, tex_frames, n_levels, d_uvd, &mip_bytes)) return rc;
  if (n_levels > 1u && d_guv && !d_mip) return fail(ctx, SRZ_E_INVALID, fn + ": d_guv needs the pyramid when n_levels > 1");
  if (n_levels > 1u && (d_gtex == nullptr) != (d_gmip == nullptr))
    return fail(ctx, SRZ_E_INVALID, fn + ": d_gtex and d_gmip come together when n_levels > 1");
  if (n_levels == 1u) {
    if (!d_gtex && !d_guv) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gtex nor d_guv is asked for");
    d_uvd = nullptr, d_mip = nullptr, d_gmip = nullptr; // (not read, not written: they take no part in the checks either)
  }
  const size_t gout_bytes = srz_frameset_interpolate_bytes(ctx, fs, n_ch), uv_bytes = srz_frameset_interpolate_bytes(ctx, fs, 2u);
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (!aligned<16>({d_vis, d_uv, d_uvd, d_gout, d_guv})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers must be 16-byte aligned");
  if (!aligned<4>({d_tex, d_mip, d_gtex, d_gmip}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the texture, the pyramid and their gradients must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn, {{d_gtex, tex_bytes}, {d_gmip, mip_bytes}, {d_guv, uv_bytes}},
                              {{d_vis, vis_bytes}, {d_uv, uv_bytes}, {d_uvd, vis_bytes}, {d_gout, gout_bytes}, {d_tex, tex_bytes}, {d_mip, mip_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture)
  TexMipArgs a = texture_mip_args(fs, d_vis, d_uv, d_uvd, d_tex, d_mip, tex_w, tex_h, n_ch, tex_frames, mode, n_levels, 2u, d_guv, flags);
  a.gout = (const float *)d_gout, a.gtex = d_gtex, a.gmip = d_gmip;
  launch_tex_mip_grad(a, s);
  return end_pass(ctx);
}

// ---- the mip pyramid of a cube: the cube viewed as 6 * tex_frames textures of n x n, through the 2D functions above
uint32_t srz_cube_mip_levels(uint32_t n) { return srz_texture_mip_levels(n, n); }

size_t srz_cube_mip_bytes(uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels) {
  if (tex_frames == 0u || tex_frames > MIP_MAX_FRAMES / 6u) return 0; // (6 * tex_frames <= 65536)
  return srz_texture_mip_bytes(n, n, n_ch, 6u * tex_frames, n_levels);
}

int srz_cube_mip_build(srz_ctx *ctx, const float *d_tex, uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels, float *d_mip,
                       size_t mip_bytes, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  if (tex_frames == 0u || tex_frames > MIP_MAX_FRAMES / 6u) return fail(ctx, SRZ_E_INVALID, "srz_cube_mip_build: 6 * tex_frames must be 6 .. 65536");
  return srz_texture_mip_build(ctx, d_tex, n, n, n_ch, 6u * tex_frames, n_levels, d_mip, mip_bytes, stream);
}

int srz_cube_mip_fold(srz_ctx *ctx, const float *d_gmip, size_t mip_bytes, uint32_t n, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels,
                      float *d_gtex, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  if (tex_frames == 0u || tex_frames > MIP_MAX_FRAMES / 6u) return fail(ctx, SRZ_E_INVALID, "srz_cube_mip_fold: 6 * tex_frames must be 6 .. 65536");
  return srz_texture_mip_fold(ctx, d_gmip, mip_bytes, n, n, n_ch, 6u * tex_frames, n_levels, d_gtex, stream);
}

// ---- the prefilter of a cube (no set: tex_frames is any count up to MIP_MAX_FRAMES)
namespace {
bool prefilter_sizes_ok(uint32_t n_src, uint32_t n_dst, uint32_t n_ch, uint32_t tex_frames) {
  return n_src != 0u && n_src <= SRZ_TEX_MAX_SIZE && n_dst != 0u && n_dst <= SRZ_TEX_MAX_SIZE && n_ch != 0u && n_ch <= SRZ_ATTR_MAX_CH &&
         tex_frames != 0u && tex_frames <= MIP_MAX_FRAMES;
}
// what srz_cube_prefilter and _prefilter_grad check alike, the pointers apart
int check_prefilter(srz_ctx *ctx, const std::string &fn, uint32_t n_src, uint32_t n_dst, uint32_t n_ch, uint32_t tex_frames, uint32_t kind,
                    float roughness, float cmin, const void *d_work, size_t work_bytes) {
  if (n_src == 0u || n_src > SRZ_TEX_MAX_SIZE || n_dst == 0u || n_dst > SRZ_TEX_MAX_SIZE)
    return fail(ctx, SRZ_E_INVALID, fn + ": n_src and n_dst must be 1 .. SRZ_TEX_MAX_SIZE");
  if (n_ch == 0u || n_ch > SRZ_ATTR_MAX_CH) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. SRZ_ATTR_MAX_CH");
  if (tex_frames == 0u || tex_frames > MIP_MAX_FRAMES) return fail(ctx, SRZ_E_INVALID, fn + ": tex_frames must be 1 .. 65536");
  if (kind != SRZ_PREFILTER_COSINE && kind != SRZ_PREFILTER_GGX) return fail(ctx, SRZ_E_INVALID, fn + ": kind must be SRZ_PREFILTER_COSINE or SRZ_PREFILTER_GGX");
  if (!std::isfinite(roughness) || roughness < 0.0f || roughness > 1.0f) return fail(ctx, SRZ_E_INVALID, fn + ": roughness must be in [0, 1]");
  if (!std::isfinite(cmin) || cmin < 0.0f || !(cmin < 1.0f)) return fail(ctx, SRZ_E_INVALID, fn + ": cmin must be in [0, 1)");
  if (!d_work) return fail(ctx, SRZ_E_INVALID, fn + ": null d_work");
  if (work_bytes < srz_cube_prefilter_work_bytes(n_src, n_dst, n_ch, tex_frames))
    return fail(ctx, SRZ_E_INVALID, fn + ": work_bytes is below srz_cube_prefilter_work_bytes");
  if (!aligned<16>({d_work})) return fail(ctx, SRZ_E_INVALID, fn + ": d_work must be 16-byte aligned");
  return SRZ_OK;
}
} // namespace

size_t srz_cube_prefilter_work_bytes(uint32_t n_src, uint32_t n_dst, uint32_t n_ch, uint32_t tex_frames) {
  if (!prefilter_sizes_ok(n_src, n_dst, n_ch, tex_frames)) return 0;
  const size_t fwd = prefilter_table_bytes(n_src) + prefilter_part_bytes(n_dst, n_src, n_ch, tex_frames, false);
  const size_t bwd = prefilter_table_bytes(n_dst) + prefilter_q_bytes(n_dst, n_ch, tex_frames) + prefilter_part_bytes(n_src, n_dst, n_ch, tex_frames, true);
  return std::max(fwd, bwd);
}

int srz_cube_prefilter(srz_ctx *ctx, const float *d_src, uint32_t n_src, float *d_dst, uint32_t n_dst, uint32_t n_ch, uint32_t tex_frames,
                       uint32_t kind, float roughness, float cmin, float *d_den, void *d_work, size_t work_bytes, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_cube_prefilter");
  if (!d_src || !d_dst) return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!d_src ? "d_src" : "d_dst"));
  if (int rc = check_prefilter(ctx, fn, n_src, n_dst, n_ch, tex_frames, kind, roughness, cmin, d_work, work_bytes)) return rc;
  if (!aligned<4>({d_src, d_dst, d_den})) return fail(ctx, SRZ_E_INVALID, fn + ": d_src, d_dst and d_den must be 4-byte aligned");
  const size_t need = srz_cube_prefilter_work_bytes(n_src, n_dst, n_ch, tex_frames), den_bytes = (size_t)prefilter_texels(n_dst) * sizeof(float);
  const size_t src_bytes = (size_t)prefilter_texels(n_src) * tex_frames * n_ch * sizeof(float), dst_bytes = den_bytes * tex_frames * n_ch;
  if (int rc = check_overlaps(ctx, fn + " (d_dst, d_den, d_work against d_src)", {{d_dst, dst_bytes}, {d_den, den_bytes}, {d_work, need}},
                              {{d_src, src_bytes}}))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  PrefilterArgs a{};
  a.src = d_src, a.dst = d_dst, a.den_out = d_den, a.work = d_work;
  a.n_src = n_src, a.n_dst = n_dst, a.n_ch = n_ch, a.frames = tex_frames, a.kind = kind, a.roughness = roughness, a.cmin = cmin;
  launch_prefilter(a, pick_stream(ctx, stream));
  return end_pass(ctx);
}

int srz_cube_prefilter_grad(srz_ctx *ctx, const float *d_gdst, const float *d_den, uint32_t n_src, uint32_t n_dst, uint32_t n_ch,
                            uint32_t tex_frames, uint32_t kind, float roughness, float cmin, float *d_gsrc, void *d_work, size_t work_bytes,
                            void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_cube_prefilter_grad");
  if (!d_gdst || !d_den || !d_gsrc) return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!d_gdst ? "d_gdst" : !d_den ? "d_den" : "d_gsrc"));
  if (int rc = check_prefilter(ctx, fn, n_src, n_dst, n_ch, tex_frames, kind, roughness, cmin, d_work, work_bytes)) return rc;
  if (!aligned<4>({d_gdst, d_den, d_gsrc})) return fail(ctx, SRZ_E_INVALID, fn + ": d_gdst, d_den and d_gsrc must be 4-byte aligned");
  const size_t need = srz_cube_prefilter_work_bytes(n_src, n_dst, n_ch, tex_frames), den_bytes = (size_t)prefilter_texels(n_dst) * sizeof(float);
  const size_t gsrc_bytes = (size_t)prefilter_texels(n_src) * tex_frames * n_ch * sizeof(float), gdst_bytes = den_bytes * tex_frames * n_ch;
  if (int rc = check_overlaps(ctx, fn + " (d_gsrc, d_work against d_gdst, d_den)", {{d_gsrc, gsrc_bytes}, {d_work, need}},
                              {{d_gdst, gdst_bytes}, {d_den, den_bytes}}))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  PrefilterArgs a{};
  a.src = d_gdst, a.den = d_den, a.dst = d_gsrc, a.work = d_work;
  a.n_src = n_src, a.n_dst = n_dst, a.n_ch = n_ch, a.frames = tex_frames, a.kind = kind, a.roughness = roughness, a.cmin = cmin;
  launch_prefilter_grad(a, pick_stream(ctx, stream));
  return end_pass(ctx);
}

// ---- SH9 lighting: a cube to its coefficients (no set), and the coefficients at each pixel's normal
namespace {
bool cube_sh_sizes_ok(uint32_t n, uint32_t n_ch, uint32_t tex_frames) {
  return n != 0u && n <= SRZ_TEX_MAX_SIZE && n_ch != 0u && n_ch <= SRZ_SH_MAX_CH && tex_frames != 0u && tex_frames <= MIP_MAX_FRAMES;
}
// what srz_cube_sh and _cube_sh_grad check alike, the pointers apart
int check_cube_sh(srz_ctx *ctx, const std::string &fn, uint32_t n, uint32_t n_ch, uint32_t tex_frames, const void *d_work, size_t work_bytes) {
  if (n == 0u || n > SRZ_TEX_MAX_SIZE) return fail(ctx, SRZ_E_INVALID, fn + ": n must be 1 .. SRZ_TEX_MAX_SIZE");
  if (n_ch == 0u || n_ch > SRZ_SH_MAX_CH) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. SRZ_SH_MAX_CH");
  if (tex_frames == 0u || tex_frames > MIP_MAX_FRAMES) return fail(ctx, SRZ_E_INVALID, fn + ": tex_frames must be 1 .. 65536");
  if (!d_work) return fail(ctx, SRZ_E_INVALID, fn + ": null d_work");
  if (work_bytes < srz_cube_sh_work_bytes(n, n_ch, tex_frames)) return fail(ctx, SRZ_E_INVALID, fn + ": work_bytes is below srz_cube_sh_work_bytes");
  return SRZ_OK;
}
// what srz_frameset_sh and _sh_grad check alike (check_light's shape); the coefficients' bytes in *sh_bytes
int check_sh(srz_ctx *ctx, const srz_frameset *fs, const std::string &fn, uint32_t n_ch, uint32_t sh_frames, uint32_t kind, uint32_t flags,
             size_t *sh_bytes) {
  if (n_ch == 0u || n_ch > SRZ_SH_MAX_CH) return fail(ctx, SRZ_E_INVALID, fn + ": n_ch must be 1 .. SRZ_SH_MAX_CH");
  if (kind != SRZ_SH_IRRADIANCE && kind != SRZ_SH_RADIANCE) return fail(ctx, SRZ_E_INVALID, fn + ": kind must be SRZ_SH_IRRADIANCE or SRZ_SH_RADIANCE");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  if (sh_frames != 1u && sh_frames != (uint32_t)fs->n_frames)
    return fail(ctx, SRZ_E_INVALID, fn + ": sh_frames must be 1 or the set's frame count");
  *sh_bytes = (size_t)sh_frames * 9u * n_ch * sizeof(float);
  return SRZ_OK;
}
ShArgs sh_args(const srz_frameset *fs, const void *d_vis, const void *d_nrm, const float *d_sh, uint32_t n_ch, uint32_t sh_frames, uint32_t kind,
               void *d_out, uint32_t flags) {
  ShArgs a{};
  const uint64_t plane = plane_words(fs);
  fill_walk(a, fs, d_vis, d_out);
  a.nrm = (const float *)d_nrm, a.sh = d_sh;
  a.vis_stride = 4ull * plane, a.frame_stride = n_ch * plane, a.nrm_stride = 3ull * plane;
  a.sh_stride = sh_frames == 1u ? 0ull : 9ull * n_ch;
  a.n_ch = n_ch, a.kind = kind;
  a.flags_or = flags;
  return a;
}
} // namespace

size_t srz_cube_sh_work_bytes(uint32_t n, uint32_t n_ch, uint32_t tex_frames) {
  if (!cube_sh_sizes_ok(n, n_ch, tex_frames)) return 0;
  return cube_sh_work_floats(n, n_ch, tex_frames) * sizeof(float); // (the backward's q fits in front of it)
}

int srz_cube_sh(srz_ctx *ctx, const float *d_src, uint32_t n, uint32_t n_ch, uint32_t tex_frames, float *d_sh, float *d_den, void *d_work,
                size_t work_bytes, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_cube_sh");
  if (!d_src || !d_sh) return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!d_src ? "d_src" : "d_sh"));
  if (int rc = check_cube_sh(ctx, fn, n, n_ch, tex_frames, d_work, work_bytes)) return rc;
  if (!aligned<4>({d_src, d_sh, d_den, d_work})) return fail(ctx, SRZ_E_INVALID, fn + ": d_src, d_sh, d_den and d_work must be 4-byte aligned");
  const size_t need = srz_cube_sh_work_bytes(n, n_ch, tex_frames), sh_bytes = (size_t)tex_frames * 9u * n_ch * sizeof(float);
  const size_t src_bytes = (size_t)prefilter_texels(n) * tex_frames * n_ch * sizeof(float);
  if (int rc = check_overlaps(ctx, fn + " (d_sh, d_den, d_work against d_src)", {{d_sh, sh_bytes}, {d_den, sizeof(float)}, {d_work, need}},
                              {{d_src, src_bytes}}))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  CubeShArgs a{};
  a.src = d_src, a.dst = d_sh, a.den_out = d_den, a.work = (float *)d_work;
  a.n = n, a.n_ch = n_ch, a.frames = tex_frames;
  launch_cube_sh(a, pick_stream(ctx, stream));
  return end_pass(ctx);
}

int srz_cube_sh_grad(srz_ctx *ctx, const float *d_gsh, const float *d_den, uint32_t n, uint32_t n_ch, uint32_t tex_frames, float *d_gsrc,
                     void *d_work, size_t work_bytes, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_cube_sh_grad");
  if (!d_gsh || !d_den || !d_gsrc) return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!d_gsh ? "d_gsh" : !d_den ? "d_den" : "d_gsrc"));
  if (int rc = check_cube_sh(ctx, fn, n, n_ch, tex_frames, d_work, work_bytes)) return rc;
  if (!aligned<4>({d_gsh, d_den, d_gsrc, d_work})) return fail(ctx, SRZ_E_INVALID, fn + ": d_gsh, d_den, d_gsrc and d_work must be 4-byte aligned");
  const size_t need = srz_cube_sh_work_bytes(n, n_ch, tex_frames), sh_bytes = (size_t)tex_frames * 9u * n_ch * sizeof(float);
  const size_t gsrc_bytes = (size_t)prefilter_texels(n) * tex_frames * n_ch * sizeof(float);
  if (int rc = check_overlaps(ctx, fn + " (d_gsrc, d_work against d_gsh, d_den)", {{d_gsrc, gsrc_bytes}, {d_work, need}},
                              {{d_gsh, sh_bytes}, {d_den, sizeof(float)}}))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  CubeShArgs a{};
  a.src = d_gsh, a.den = d_den, a.dst = d_gsrc, a.work = (float *)d_work;
  a.n = n, a.n_ch = n_ch, a.frames = tex_frames;
  launch_cube_sh_grad(a, pick_stream(ctx, stream));
  return end_pass(ctx);
}

int srz_frameset_sh(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const float *d_sh, uint32_t n_ch, uint32_t sh_frames,
                    uint32_t kind, void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_sh");
  if (!fs || !d_vis || !d_nrm || !d_sh || !d_out)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_nrm ? "d_nrm" : !d_sh ? "d_sh" : "d_out"));
  size_t sh_bytes = 0;
  if (int rc = check_sh(ctx, fs, fn, n_ch, sh_frames, kind, flags, &sh_bytes)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, n_ch), nrm_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u);
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_vis, d_nrm, d_out})) return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_nrm, d_out) must be 16-byte aligned");
  if (!aligned<4>({d_sh})) return fail(ctx, SRZ_E_INVALID, fn + ": d_sh must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn + " (d_out against d_vis, d_nrm, d_sh)", {{d_out, need}},
                              {{d_vis, vis_bytes}, {d_nrm, nrm_bytes}, {d_sh, sh_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_light: caller data only)
  launch_sh(sh_args(fs, d_vis, d_nrm, d_sh, n_ch, sh_frames, kind, d_out, flags), s);
  return end_pass(ctx);
}

size_t srz_frameset_sh_work_bytes(srz_ctx *ctx, srz_frameset *fs, uint32_t n_ch) {
  if (!ctx || !fs || n_ch == 0u || n_ch > SRZ_SH_MAX_CH) return 0;
  // [frame][tile][K] partial sums, and [frame][K] rows for the fold of shared coefficients
  return (size_t)fs->n_frames * ((size_t)fs->n_local_bands * fs->tiles_x + 1u) * 9u * n_ch * sizeof(float);
}

int srz_frameset_sh_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_nrm, const float *d_sh, uint32_t n_ch,
                         uint32_t sh_frames, uint32_t kind, const void *d_gout, void *d_gnrm, float *d_gsh, void *d_work, size_t work_bytes,
                         uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_sh_grad");
  if (!fs || !d_vis || !d_nrm || !d_sh || !d_gout)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_nrm ? "d_nrm" : !d_sh ? "d_sh" : "d_gout"));
  if (!d_gnrm && !d_gsh) return fail(ctx, SRZ_E_INVALID, fn + ": neither d_gnrm nor d_gsh is asked for");
  if (d_gsh && !d_work) return fail(ctx, SRZ_E_INVALID, fn + ": d_gsh needs d_work");
  size_t sh_bytes = 0;
  if (int rc = check_sh(ctx, fs, fn, n_ch, sh_frames, kind, flags, &sh_bytes)) return rc;
  const size_t gout_bytes = srz_frameset_interpolate_bytes(ctx, fs, n_ch), nrm_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u);
  const size_t vis_bytes = srz_frameset_out_bytes(ctx, fs);
  const size_t need_work = d_gsh ? srz_frameset_sh_work_bytes(ctx, fs, n_ch) : 0;
  if (work_bytes < need_work) return fail(ctx, SRZ_E_INVALID, fn + ": work_bytes is below srz_frameset_sh_work_bytes");
  if (!aligned<16>({d_vis, d_nrm, d_gout, d_gnrm}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_nrm, d_gout, d_gnrm) must be 16-byte aligned");
  if (!aligned<4>({d_sh, d_gsh, d_gsh ? d_work : nullptr})) return fail(ctx, SRZ_E_INVALID, fn + ": d_sh, d_gsh and d_work must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn + " (d_gnrm, d_gsh, d_work against d_vis, d_nrm, d_sh, d_gout)",
                              {{d_gnrm, nrm_bytes}, {d_gsh, sh_bytes}, {d_gsh ? d_work : nullptr, need_work}},
                              {{d_vis, vis_bytes}, {d_nrm, nrm_bytes}, {d_sh, sh_bytes}, {d_gout, gout_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc;
  ShArgs a = sh_args(fs, d_vis, d_nrm, d_sh, n_ch, sh_frames, kind, nullptr, flags);
  a.gout = (const float *)d_gout, a.gnrm = (float *)d_gnrm;
  a.work = d_gsh ? (float *)d_work : nullptr;
  launch_sh_grad(a, d_gsh, s);
  return end_pass(ctx);
}

int srz_frameset_texture_cube_mip(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_dir, const void *d_lam, const float *d_tex,
                                  uint32_t n, uint32_t n_ch, uint32_t tex_frames, const float *d_mip, uint32_t n_levels, void *d_out,
                                  size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_texture_cube_mip");
  if (!fs || !d_vis || !d_dir || !d_tex || !d_out)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_dir ? "d_dir" : !d_tex ? "d_tex" : "d_out"));
  size_t tex_bytes = 0, mip_bytes = 0;
  if (int rc = check_cube(ctx, fs, fn, n, n_ch, tex_frames, flags, &tex_bytes)) return rc;
  if (int rc = check_cube_mip(ctx, fn, n, n_ch, tex_frames, n_levels, d_lam, &mip_bytes)) return rc;
  if (n_levels > 1u && !d_mip) return fail(ctx, SRZ_E_INVALID, fn + ": n_levels > 1 needs the pyramid");
  if (n_levels == 1u) d_lam = nullptr, d_mip = nullptr; // (not read: they take no part in the checks either)
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, n_ch), dir_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u);
  const size_t lam_bytes = srz_frameset_interpolate_bytes(ctx, fs, 1u), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_vis, d_dir, d_lam, d_out}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_dir, d_lam, d_out) must be 16-byte aligned");
  if (!aligned<4>({d_tex, d_mip})) return fail(ctx, SRZ_E_INVALID, fn + ": d_tex and d_mip must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn, {{d_out, need}},
                              {{d_vis, vis_bytes}, {d_dir, dir_bytes}, {d_lam, lam_bytes}, {d_tex, tex_bytes}, {d_mip, mip_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture_cube)
  launch_cube_mip(cube_mip_args(fs, d_vis, d_dir, d_lam, d_tex, d_mip, n, n_ch, tex_frames, n_levels, n_ch, d_out, flags), s);
  return end_pass(ctx);
}

int srz_frameset_texture_cube_mip_grad(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_dir, const void *d_lam,
                                       const void *d_gout, const float *d_tex, const float *d_mip, uint32_t n, uint32_t n_ch,
                                       uint32_t tex_frames, uint32_t n_levels, float *d_gtex, float *d_gmip, void *d_gdir, void *d_glam,
                                       uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_texture_cube_mip_grad");
  if (!fs || !d_vis || !d_dir || !d_gout)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_dir ? "d_dir" : "d_gout"));
  if (!d_gtex && !d_gmip && !d_gdir && !d_glam) return fail(ctx, SRZ_E_INVALID, fn + ": no output is asked for");
  if ((d_gdir || d_glam) && !d_tex) return fail(ctx, SRZ_E_INVALID, fn + ": d_gdir and d_glam need d_tex");
  size_t tex_bytes = 0, mip_bytes = 0;
  if (int rc = check_cube(ctx, fs, fn, n, n_ch, tex_frames, flags, &tex_bytes)) return rc;
  if (int rc = check_cube_mip(ctx, fn, n, n_ch, tex_frames, n_levels, d_lam, &mip_bytes)) return rc;
  if (n_levels > 1u && (d_gdir || d_glam) && !d_mip) return fail(ctx, SRZ_E_INVALID, fn + ": d_gdir and d_glam need the pyramid when n_levels > 1");
  if (n_levels > 1u && (d_gtex == nullptr) != (d_gmip == nullptr))
    return fail(ctx, SRZ_E_INVALID, fn + ": d_gtex and d_gmip come together when n_levels > 1");
  if (n_levels == 1u) {
    if (!d_gtex && !d_gdir && !d_glam) return fail(ctx, SRZ_E_INVALID, fn + ": no output is asked for");
    d_lam = nullptr, d_mip = nullptr, d_gmip = nullptr; // (not read, not written: they take no part in the checks either)
  }
  const size_t gout_bytes = srz_frameset_interpolate_bytes(ctx, fs, n_ch), dir_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u);
  const size_t lam_bytes = srz_frameset_interpolate_bytes(ctx, fs, 1u), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (!aligned<16>({d_vis, d_dir, d_lam, d_gout, d_gdir, d_glam}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_dir, d_lam, d_gout, d_gdir, d_glam) must be 16-byte aligned");
  if (!aligned<4>({d_tex, d_mip, d_gtex, d_gmip}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the cube, the pyramid and their gradients must be 4-byte aligned");
  if (int rc = check_overlaps(ctx, fn, {{d_gtex, tex_bytes}, {d_gmip, mip_bytes}, {d_gdir, dir_bytes}, {d_glam, lam_bytes}},
                              {{d_vis, vis_bytes}, {d_dir, dir_bytes}, {d_lam, lam_bytes}, {d_gout, gout_bytes}, {d_tex, tex_bytes}, {d_mip, mip_bytes}}))
    return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (as srz_frameset_texture_cube)
  CubeMipArgs a = cube_mip_args(fs, d_vis, d_dir, d_lam, d_tex, d_mip, n, n_ch, tex_frames, n_levels, 3u, d_gdir, flags);
  a.gout = (const float *)d_gout, a.gtex = d_gtex, a.gmip = d_gmip, a.glam = (float *)d_glam;
  launch_cube_mip_grad(a, s);
  return end_pass(ctx);
}

int srz_frameset_cube_level(srz_ctx *ctx, srz_frameset *fs, const void *d_vis, const void *d_dir, const void *d_dird, uint32_t n,
                            uint32_t n_levels, void *d_out, size_t out_bytes, uint32_t flags, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  const std::string fn("srz_frameset_cube_level");
  if (!fs || !d_vis || !d_dir || !d_dird || !d_out)
    return fail(ctx, SRZ_E_INVALID, fn + ": null " + (!fs ? "frameset" : !d_vis ? "d_vis" : !d_dir ? "d_dir" : !d_dird ? "d_dird" : "d_out"));
  if (n == 0u || n > SRZ_TEX_MAX_SIZE) return fail(ctx, SRZ_E_INVALID, fn + ": n must be 1 .. SRZ_TEX_MAX_SIZE");
  if (n_levels == 0u || n_levels > srz_cube_mip_levels(n)) return fail(ctx, SRZ_E_INVALID, fn + ": n_levels must be 1 .. srz_cube_mip_levels(n)");
  if (int rc = check_pass_flags(ctx, fn, flags)) return rc;
  const size_t need = srz_frameset_interpolate_bytes(ctx, fs, 1u), dir_bytes = srz_frameset_interpolate_bytes(ctx, fs, 3u);
  const size_t dird_bytes = srz_frameset_interpolate_bytes(ctx, fs, 6u), vis_bytes = srz_frameset_out_bytes(ctx, fs);
  if (out_bytes < need) return fail(ctx, SRZ_E_INVALID, fn + ": out_bytes is too small for d_out");
  if (!aligned<16>({d_vis, d_dir, d_dird, d_out}))
    return fail(ctx, SRZ_E_INVALID, fn + ": the plane buffers (d_vis, d_dir, d_dird, d_out) must be 16-byte aligned");
  if (int rc = check_overlaps(ctx, fn, {{d_out, need}}, {{d_vis, vis_bytes}, {d_dir, dir_bytes}, {d_dird, dird_bytes}})) return rc;
  hipStream_t s;
  if (int rc = begin_pass(ctx, fs, stream, 0u, &s)) return rc; // (planes only: no vertex stage)
  CubeMipArgs a = cube_mip_args(fs, d_vis, d_dir, nullptr, nullptr, nullptr, n, 1u, 1u, n_levels, 1u, d_out, flags);
  a.dird = (const float *)d_dird;
  launch_cube_level(a, s);
  return end_pass(ctx);
}

int srz_frameset_update_shading(srz_ctx *ctx, srz_frameset *fs, const srz_frame *frames, int n_frames) {
  if (!ctx) return SRZ_E_INVALID;
  if (!fs || !frames) return fail(ctx, SRZ_E_INVALID, "srz_frameset_update_shading: null frameset / frames");
  if (fs->d_draws) return fail(ctx, SRZ_E_INVALID, "srz_frameset_update_shading: a sceneset (its shading changes with srz_sceneset_update)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // (on the context's stream, like srz_sceneset_update: after every render already submitted there, before the next one)
  return refresh_frames(ctx, fs, frames, n_frames, "srz_frameset_update_shading", /*copy_tris=*/false);
}

int srz_frameset_resolve8(srz_ctx *ctx, const srz_frameset *fs, const void *d_planes, void *d_bgr8, size_t bgr8_bytes, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  if (!fs || !d_planes || !d_bgr8) return fail(ctx, SRZ_E_INVALID, "srz_frameset_resolve8: null argument");
  if (bgr8_bytes < (size_t)fs->n_frames * fs->local_rows * (size_t)fs->width * 3) return fail(ctx, SRZ_E_INVALID, "srz_frameset_resolve8: output too small");
  if ((uintptr_t)d_planes & 3u) return fail(ctx, SRZ_E_INVALID, "srz_frameset_resolve8: misaligned planes");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick_stream(ctx, stream);
  launch_resolve8((const float *)d_planes, (uint8_t *)d_bgr8, (uint32_t)fs->n_frames, fs->local_rows, (uint32_t)fs->width,
                  4ull * fs->local_rows * (uint64_t)fs->width, s);
  HIP_TRY(ctx, hipGetLastError());
  return SRZ_OK;
}

int srz_frameset_stats(srz_ctx *ctx, srz_frameset *fs, srz_stats *stats) {
  if (!ctx) return SRZ_E_INVALID;
  if (!fs || !stats) return fail(ctx, SRZ_E_INVALID, "srz_frameset_stats: null argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the counters come from the kernels' own state, and with the fused clear nothing reads the incoming framebuffer: the
  // counting run's pixels go to a scratch buffer of ONE frame that every frame overwrites (16.8 MB instead of 4.3 GB at 256
  // frames of 1024^2)
  float *d_out = nullptr;
  HIP_TRY(ctx, hipMalloc(&d_out, srz_frameset_out_bytes(ctx, fs) / (size_t)std::max(fs->n_frames, 1)));
  int rc = render_impl(ctx, fs, d_out, SRZ_FUSED_CLEAR, ctx->stream, Pass::counting_into_one_frame());
  if (rc == SRZ_OK) rc = read_stats(ctx, ctx->stream, stats);
  (void)hipFree(d_out);
  if (rc == SRZ_OK) fs->stats = *stats, fs->have_stats = true;
  return rc;
}

uint64_t srz_frameset_algorithmic_bytes(const srz_ctx *ctx, const srz_frameset *fs) {
  if (!ctx || !fs) return 0;
  // rows actually owned (not the all-gather padding)
  uint64_t rows = 0;
  for (uint32_t lb = 0; lb < fs->n_local_bands; ++lb) {
    int band = band_of((int)lb, fs->shard_rank, fs->shard_world);
    rows += (uint64_t)std::min(BAND, fs->height - band * BAND);
  }
  uint64_t fb = 16ull * (uint64_t)fs->width * rows * (uint64_t)fs->n_frames;
  uint64_t stream = 96ull * fs->total_tris + 24ull * fs->total_lights;
  uint64_t tex = 0;
  if (fs->have_stats) {
    // B_tex = min(3*texW*texH per frame, 3 bytes per texture-shaded pixel)
    uint64_t cap = 0;
    for (const BatchDesc &b : fs->h_batches)
      if (b.tex_id >= 0 && b.tex_id < MAX_TEX && ctx->h_tex[b.tex_id].bgrx &&
          (b.shader == SRZ_SHADER_TEXTURE || b.shader == SRZ_SHADER_DISPLACEMENT || b.shader == SRZ_SHADER_BUMP))
        cap = std::max<uint64_t>(cap, 3ull * ctx->h_tex[b.tex_id].w * ctx->h_tex[b.tex_id].h);
    tex = std::min<uint64_t>(cap * (uint64_t)fs->n_frames, 3ull * fs->stats.visible_textured);
  }
  return fb + stream + tex;
}

int srz_set_kernel_timing(srz_ctx *ctx, int enabled) {
  if (!ctx) return SRZ_E_INVALID;
  ctx->timing = enabled < 0 ? 0 : (enabled > 2 ? 2 : enabled);
  return SRZ_OK;
}

int srz_kernel_time_ms(srz_ctx *ctx, int reset, double *ms4, int *launches) {
  if (!ctx) return SRZ_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = collect_events(ctx);
  if (rc) return rc;
  for (int i = 0; i < 4; ++i)
    if (ms4) ms4[i] = ctx->acc_launches ? ctx->acc_ms[i] / ctx->acc_launches : 0.0;
  if (launches) *launches = ctx->acc_launches;
  if (reset) {
    ctx->acc_ms[0] = ctx->acc_ms[1] = ctx->acc_ms[2] = ctx->acc_ms[3] = 0.0, ctx->acc_launches = 0, ctx->acc_samples.clear();
    ctx->span_open = false, ctx->span_ms = 0.0;
  }
  return SRZ_OK;
}

/* the whole-launch-set time (ms) of each timed render since the last reset, in submission order, and the span from the
 * first one's start to the latest end (renders submitted to different streams overlap: the span is what they took
 * together).  Call before the resetting srz_kernel_time_ms.  *n = values written (at most cap) */
int srz_kernel_time_samples(srz_ctx *ctx, float *out, int cap, int *n, double *span_ms) {
  if (!ctx || !n || (cap > 0 && !out)) return SRZ_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = collect_events(ctx);
  if (rc) return rc;
  int m = (int)std::min<size_t>(ctx->acc_samples.size(), (size_t)std::max(cap, 0));
  for (int i = 0; i < m; ++i) out[i] = ctx->acc_samples[i];
  *n = m;
  if (span_ms) *span_ms = ctx->span_ms;
  return SRZ_OK;
}

/* self-check: exhaustive (2^32 operands) comparison of the kernels' short exact rcp / sqrt sequences with the IEEE
 * expansions. out4 = {fast-path operands, rcp mismatches, sqrt mismatches, 1/sqrt mismatches} */
int srz_verify_fastmath(srz_ctx *ctx, uint64_t *out4) {
  if (!ctx || !out4) return SRZ_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_stats, 0, 4 * sizeof(unsigned long long), ctx->stream));
  launch_verify_fastmath(ctx->d_stats, ctx->stream);
  unsigned long long h[4];
  HIP_TRY(ctx, hipMemcpyAsync(h, ctx->d_stats, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 4; ++i) out4[i] = h[i];
  return SRZ_OK;
}

int srz_verify_fastdiv(srz_ctx *ctx, uint64_t *out3) {
  if (!ctx || !out3) return SRZ_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_stats, 0, 4 * sizeof(unsigned long long), ctx->stream));
  launch_verify_fastdiv(ctx->d_stats, ctx->stream);
  unsigned long long h[3];
  HIP_TRY(ctx, hipMemcpyAsync(h, ctx->d_stats, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 3; ++i) out3[i] = h[i];
  return SRZ_OK;
}

int srz_verify_fastpow(srz_ctx *ctx, float p, uint64_t *out4) {
  if (!ctx || !out4) return SRZ_E_INVALID;
  if (!(p > 0.0f && p <= 4096.0f) || p == std::trunc(p)) return fail(ctx, SRZ_E_INVALID, "srz_verify_fastpow: p must be a non-integer in (0, 4096]");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_stats, 0, 4 * sizeof(unsigned long long), ctx->stream));
  launch_verify_fastpow(ctx->d_stats, p, ctx->stream);
  unsigned long long h[4];
  HIP_TRY(ctx, hipMemcpyAsync(h, ctx->d_stats, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 4; ++i) out4[i] = h[i];
  return SRZ_OK;
}

/* diagnostic (tests): what the LAST render of the set left in its counters — out4 = { tiles the ordered rasteriser (k_raster_slow)
 * took, tiles the FAST shading builds handed to the generic one, the tile-list pool's capacity per sub-pool, the largest demand a
 * sub-pool has reported }.  Waits for the device. */
int srz_frameset_debug_counters(srz_ctx *ctx, srz_frameset *fs, uint32_t *out6) {
  if (!ctx || !fs || !out6) return ctx ? fail(ctx, SRZ_E_INVALID, "srz_frameset_debug_counters: null argument") : SRZ_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  uint32_t h[2] = {0, 0};
  HIP_TRY(ctx, hipMemcpy(h, fs->d_slow_count, sizeof h, hipMemcpyDeviceToHost));
  out6[0] = h[0], out6[1] = h[1], out6[2] = fs->pool_sub_cap, out6[3] = max_pool_demand(fs, 0, srz_frameset::DEMAND_PARTS);
  const uint32_t decided = fs->clear_tune.h_wgs ? *static_cast<volatile uint32_t *>(fs->clear_tune.h_wgs) : 0u;
  out6[4] = ctx->env_clear_wgs ? ctx->env_clear_wgs : (decided ? decided : fs->clear_tune.wgs), out6[5] = (fs->clear_tune.done || decided) ? 1u : 0u;
  return SRZ_OK;
}

/* diagnostic (tests): which shading builds the set's next colour render or shade launches — out2 = { fast_kinds (bit k: some frame
 * is shaded by the FAST build of kind k, frame_kind), 1 if some frame takes the generic build }.  Host state only: launches nothing. */
int srz_frameset_shade_kinds(srz_ctx *ctx, srz_frameset *fs, uint32_t *out2) {
  if (!ctx || !fs || !out2) return ctx ? fail(ctx, SRZ_E_INVALID, "srz_frameset_shade_kinds: null argument") : SRZ_E_INVALID;
  out2[0] = fs->fast_kinds, out2[1] = fs->any_generic ? 1u : 0u;
  return SRZ_OK;
}

int srz_verify_fastlen(srz_ctx *ctx, uint64_t *out5) {
  if (!ctx || !out5) return SRZ_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_stats, 0, 5 * sizeof(unsigned long long), ctx->stream));
  launch_verify_fastlen(ctx->d_stats, ctx->stream);
  unsigned long long h[5];
  HIP_TRY(ctx, hipMemcpyAsync(h, ctx->d_stats, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 5; ++i) out5[i] = h[i];
  return SRZ_OK;
}

/* diagnostic: raw counters of the last STATS run (incl. per-phase cycle sums); not part of the stable ABI */
int srz_debug_counters(srz_ctx *ctx, uint64_t *out, int n) {
  if (!ctx || !out) return SRZ_E_INVALID;
#ifdef SRZ_PHASE_PROBE /* dev build: the device counters as they are now (k_shade's phase clocks), then zeroed */
  (void)hipDeviceSynchronize();
  (void)hipMemcpy(ctx->dbg, ctx->d_stats, sizeof ctx->dbg, hipMemcpyDeviceToHost);
  (void)hipMemset(ctx->d_stats, 0, sizeof ctx->dbg);
#endif
  for (int i = 0; i < n && i < ST_COUNT; ++i) out[i] = ctx->dbg[i];
  return ST_COUNT;
}

/* ---- multi-GPU: the band exchange on RCCL ---------------------------------------------------------------------------
 * librccl is loaded on first use (a single-GPU program never needs it); if the process already holds a copy (PyTorch
 * ships its own), that one is used. */
} // extern "C"
namespace {
struct RcclApi {
  void *handle = nullptr;
  struct UniqueId { char internal[128]; };
  int (*GetUniqueId)(UniqueId *) = nullptr;
  int (*CommInitRank)(void **, int, UniqueId, int) = nullptr;
  int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  std::string error;
};
RcclApi &rccl() {
  static RcclApi api;
  static bool tried = false;
  if (tried) return api;
  tried = true;
  const char *names[] = {"librccl.so", "librccl.so.1"};
  for (const char *n : names)
    if (!api.handle) api.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL); // a copy the process already loaded
  for (const char *n : names)
    if (!api.handle) api.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
  if (!api.handle) api.handle = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!api.handle) {
    api.error = std::string("cannot load librccl: ") + (dlerror() ? dlerror() : "?");
    return api;
  }
  api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(api.handle, "ncclGetUniqueId"));
  api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(api.handle, "ncclCommInitRank"));
  api.AllGather = reinterpret_cast<decltype(api.AllGather)>(dlsym(api.handle, "ncclAllGather"));
  api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.handle, "ncclCommDestroy"));
  api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.handle, "ncclGetErrorString"));
  if (!api.GetUniqueId || !api.CommInitRank || !api.AllGather || !api.CommDestroy) api.error = "librccl lacks the nccl* entry points";
  return api;
}
std::string rccl_err(int rc) {
  RcclApi &r = rccl();
  return r.GetErrorString ? r.GetErrorString(rc) : ("rccl error " + std::to_string(rc));
}
} // namespace
extern "C" {

struct srz_comm {
  void *comm = nullptr;
  int rank = 0, world = 1;
  // srz_frameset_allgather_sparse: every rank's {message header, recv_bytes} (SPARSE_SLOT bytes each), on the device and in
  // pinned host memory
  static constexpr size_t SPARSE_SLOT = 32;
  uint8_t *d_sizes = nullptr, *h_sizes = nullptr;
};

int srz_comm_unique_id(uint8_t *out128) {
  if (!out128) return fail(nullptr, SRZ_E_INVALID, "srz_comm_unique_id: out is NULL");
  RcclApi &r = rccl();
  if (!r.error.empty()) return fail(nullptr, SRZ_E_NODEVICE, "srz_comm_unique_id: " + r.error);
  RcclApi::UniqueId id;
  const int rc = r.GetUniqueId(&id);
  if (rc != 0) return fail(nullptr, SRZ_E_NODEVICE, "ncclGetUniqueId: " + rccl_err(rc));
  std::memcpy(out128, id.internal, 128);
  return SRZ_OK;
}

int srz_comm_create(srz_ctx *ctx, const uint8_t *id128, int rank, int world, srz_comm **out) {
  if (!ctx) return SRZ_E_INVALID;
  if (!out || !id128 || world < 1 || rank < 0 || rank >= world) return fail(ctx, SRZ_E_INVALID, "srz_comm_create: bad arguments");
  *out = nullptr;
  RcclApi &r = rccl();
  if (!r.error.empty()) return fail(ctx, SRZ_E_NODEVICE, "srz_comm_create: " + r.error);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  srz_comm *c = new (std::nothrow) srz_comm();
  if (!c) return fail(ctx, SRZ_E_NOMEM, "srz_comm_create: out of host memory");
  RcclApi::UniqueId id;
  std::memcpy(id.internal, id128, 128);
  const int rc = r.CommInitRank(&c->comm, world, id, rank);
  if (rc != 0) {
    delete c;
    return fail(ctx, SRZ_E_NODEVICE, "ncclCommInitRank: " + rccl_err(rc));
  }
  c->rank = rank, c->world = world;
  ctx->shard_rank = rank, ctx->shard_world = world; // = srz_set_shard: framesets created from now on are this rank's bands
  *out = c;
  return SRZ_OK;
}

void srz_comm_destroy(srz_ctx *ctx, srz_comm *c) {
  if (!c) return;
  if (ctx) (void)hipSetDevice(ctx->device), (void)hipDeviceSynchronize();
  if (c->comm) (void)rccl().CommDestroy(c->comm);
  (void)hipFree(c->d_sizes);
  if (c->h_sizes) (void)hipHostFree(c->h_sizes);
  delete c;
}

size_t srz_frameset_exchange_bytes(const srz_ctx *ctx, const srz_frameset *fs, int what) {
  if (!fs) return 0;
  const size_t row = what == SRZ_EXCHANGE_BGR8 ? (size_t)fs->width * 3u : (size_t)fs->width * sizeof(float);
  const size_t planes = what == SRZ_EXCHANGE_BGR8 ? 1u : 4u;
  return (size_t)fs->n_frames * planes * fs->local_rows * row;
}

int srz_frameset_deinterleave(srz_ctx *ctx, const srz_frameset *fs, const void *d_gathered, void *d_full, int what, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  if (!fs || !d_gathered || !d_full || (what != SRZ_EXCHANGE_PLANES && what != SRZ_EXCHANGE_BGR8))
    return fail(ctx, SRZ_E_INVALID, "srz_frameset_deinterleave: bad arguments");
  if (fs->shard_world == 1) return fail(ctx, SRZ_E_INVALID, "srz_frameset_deinterleave: the frameset is not sharded");
  const uint32_t row_bytes = what == SRZ_EXCHANGE_BGR8 ? (uint32_t)fs->width * 3u : (uint32_t)fs->width * 4u;
  if (what == SRZ_EXCHANGE_PLANES && (((uintptr_t)d_gathered | (uintptr_t)d_full) & 3u))
    return fail(ctx, SRZ_E_INVALID, "srz_frameset_deinterleave: misaligned buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick_stream(ctx, stream);
  launch_deinterleave(d_gathered, d_full, (uint32_t)fs->shard_world, (uint32_t)fs->n_frames * (what == SRZ_EXCHANGE_BGR8 ? 1u : 4u),
                      fs->bands_per_rank, row_bytes, s);
  HIP_TRY(ctx, hipGetLastError());
  return SRZ_OK;
}

int srz_frameset_allgather(srz_ctx *ctx, srz_comm *c, const srz_frameset *fs, const void *d_shard, void *d_gathered, void *d_full,
                           int what, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  if (!c || !fs || !d_shard || !d_gathered || !d_full) return fail(ctx, SRZ_E_INVALID, "srz_frameset_allgather: null argument");
  if (fs->shard_world != c->world || fs->shard_rank != c->rank)
    return fail(ctx, SRZ_E_INVALID, "srz_frameset_allgather: the frameset was not created under this communicator's shard");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick_stream(ctx, stream);
  const size_t bytes = srz_frameset_exchange_bytes(ctx, fs, what);
  if (bytes == 0) return fail(ctx, SRZ_E_INVALID, "srz_frameset_allgather: bad exchange kind");
  if (c->world == 1) { // one rank: the shard is the frame
    HIP_TRY(ctx, hipMemcpyAsync(d_full, d_shard, bytes, hipMemcpyDeviceToDevice, s));
    return SRZ_OK;
  }
  const int rc = rccl().AllGather(d_shard, d_gathered, bytes, /* ncclUint8 */ 1, c->comm, s);
  if (rc != 0) return fail(ctx, SRZ_E_NODEVICE, "ncclAllGather: " + rccl_err(rc));
  return srz_frameset_deinterleave(ctx, fs, d_gathered, d_full, what, stream);
}

int srz_frameset_allgather_inplace(srz_ctx *ctx, srz_comm *c, const srz_frameset *fs, void *d_gathered, int what, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  if (!c || !fs || !d_gathered) return fail(ctx, SRZ_E_INVALID, "srz_frameset_allgather_inplace: null argument");
  if (fs->shard_world != c->world || fs->shard_rank != c->rank)
    return fail(ctx, SRZ_E_INVALID, "srz_frameset_allgather_inplace: the frameset was not created under this communicator's shard");
  const size_t bytes = srz_frameset_exchange_bytes(ctx, fs, what);
  if (bytes == 0 || (what != SRZ_EXCHANGE_PLANES && what != SRZ_EXCHANGE_BGR8)) return fail(ctx, SRZ_E_INVALID, "srz_frameset_allgather_inplace: bad exchange kind");
  if (c->world == 1) return SRZ_OK; // one rank: its shard is the whole buffer
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick_stream(ctx, stream);
  // in place: sendbuff == recvbuff + rank * count (the form NCCL / RCCL document for an all-gather without a copy of the own part)
  const int rc = rccl().AllGather(static_cast<const uint8_t *>(d_gathered) + (size_t)c->rank * bytes, d_gathered, bytes, /* ncclUint8 */ 1, c->comm, s);
  if (rc != 0) return fail(ctx, SRZ_E_NODEVICE, "ncclAllGather (in place): " + rccl_err(rc));
  return SRZ_OK;
}

size_t srz_frameset_gathered_row_offset(const srz_ctx *ctx, const srz_frameset *fs, int what, int frame, int plane, int row) {
  if (!fs || frame < 0 || frame >= fs->n_frames || row < 0 || row >= fs->height) return (size_t)-1;
  if (what != SRZ_EXCHANGE_PLANES && what != SRZ_EXCHANGE_BGR8) return (size_t)-1;
  const size_t planes = what == SRZ_EXCHANGE_BGR8 ? 1u : 4u;
  if (plane < 0 || (size_t)plane >= planes) return (size_t)-1;
  const size_t row_bytes = what == SRZ_EXCHANGE_BGR8 ? (size_t)fs->width * 3u : (size_t)fs->width * sizeof(float);
  const size_t band = (size_t)row / BAND, world = (size_t)fs->shard_world;
  const size_t rank = (size_t)rank_of_band((int)band, (int)world), local_row = (band / world) * BAND + (size_t)row % BAND;
  const size_t shard_rows = fs->shard_world == 1 ? (size_t)fs->height : (size_t)fs->bands_per_rank * BAND;
  return (((rank * (size_t)fs->n_frames + (size_t)frame) * planes + (size_t)plane) * shard_rows + local_row) * row_bytes;
}

int srz_frameset_read_gathered_frame(srz_ctx *ctx, const srz_frameset *fs, const void *d_gathered, int what, int frame, void *host_out,
                                     void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  if (!fs || !d_gathered || !host_out || frame < 0 || frame >= fs->n_frames || (what != SRZ_EXCHANGE_PLANES && what != SRZ_EXCHANGE_BGR8))
    return fail(ctx, SRZ_E_INVALID, "srz_frameset_read_gathered_frame: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick_stream(ctx, stream);
  const size_t planes = what == SRZ_EXCHANGE_BGR8 ? 1u : 4u;
  const size_t row_bytes = what == SRZ_EXCHANGE_BGR8 ? (size_t)fs->width * 3u : (size_t)fs->width * sizeof(float);
  const size_t band_bytes = row_bytes * BAND, world = (size_t)fs->shard_world;
  const size_t n_bands = ((size_t)fs->height + BAND - 1) / BAND;
  // band by band (a rank's bands are consecutive in its shard but, with the rotated band → rank map, not equidistant in the image)
  (void)band_bytes, (void)world;
  for (size_t p = 0; p < planes; ++p)
    for (size_t b = 0; b < n_bands; ++b) {
      const size_t rows = std::min<size_t>(BAND, (size_t)fs->height - b * BAND);
      const uint8_t *src = static_cast<const uint8_t *>(d_gathered) + srz_frameset_gathered_row_offset(ctx, fs, what, frame, (int)p, (int)(b * BAND));
      uint8_t *dst = static_cast<uint8_t *>(host_out) + (p * (size_t)fs->height + b * BAND) * row_bytes;
      HIP_TRY(ctx, hipMemcpyAsync(dst, src, rows * row_bytes, hipMemcpyDeviceToHost, s));
    }
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return SRZ_OK;
}

/* ---- the tile-sparse exchange (message format: include/srz.h) ------------------------------------------------------------------ */
} // extern "C"
namespace {
bool sparse_kind(int what) { return what == SRZ_EXCHANGE_PLANES || what == SRZ_EXCHANGE_BGR8; }
SparseArgs sparse_args(const srz_frameset *fs, int what) {
  SparseArgs a{};
  a.tile_info = fs->d_tile_info, a.frames = fs->d_frames, a.row_cnt = fs->d_sparse_rows, a.flags_or = fs->last_flags;
  a.n_frames = (uint32_t)fs->n_frames, a.n_local_bands = fs->n_local_bands, a.bands_per_rank = fs->bands_per_rank, a.tiles_x = fs->tiles_x;
  a.width = (uint32_t)fs->width, a.height = (uint32_t)fs->height, a.local_rows = fs->local_rows;
  a.rank = (uint32_t)fs->shard_rank, a.world = (uint32_t)fs->shard_world;
  a.planes = what == SRZ_EXCHANGE_BGR8 ? 1u : 4u, a.px_bytes = what == SRZ_EXCHANGE_BGR8 ? 3u : 4u, a.row_bytes = a.width * a.px_bytes;
  const uint64_t n_tab = (uint64_t)a.n_frames * a.bands_per_rank * a.tiles_x;
  a.payload_off = (SPARSE_HEADER + 4u * n_tab + 15u) & ~(uint64_t)15u;
  return a;
}
uint64_t sparse_tile_bytes(const SparseArgs &a) { return (uint64_t)a.planes * BAND * TILE * a.px_bytes; }
} // namespace
extern "C" {

size_t srz_frameset_sparse_capacity(const srz_ctx *ctx, const srz_frameset *fs, int what) {
  if (!fs || !sparse_kind(what)) return 0;
  const SparseArgs a = sparse_args(fs, what);
  return (size_t)(a.payload_off + (uint64_t)a.n_frames * a.bands_per_rank * a.tiles_x * sparse_tile_bytes(a));
}

int srz_frameset_sparse_pack(srz_ctx *ctx, srz_frameset *fs, const void *d_shard, void *d_msg, size_t msg_bytes, int what, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  if (!fs || !d_shard || !d_msg || !sparse_kind(what)) return fail(ctx, SRZ_E_INVALID, "srz_frameset_sparse_pack: bad arguments");
  if (fs->shard_rank != ctx->shard_rank || fs->shard_world != ctx->shard_world)
    return fail(ctx, SRZ_E_INVALID, "srz_frameset_sparse_pack: the frameset was created under a different shard");
  const size_t cap = srz_frameset_sparse_capacity(ctx, fs, what);
  if (msg_bytes < cap)
    return fail(ctx, SRZ_E_INVALID, "srz_frameset_sparse_pack: message buffer of " + std::to_string(msg_bytes) + " bytes, " +
                                        std::to_string(cap) + " needed (srz_frameset_sparse_capacity)");
  if ((uintptr_t)d_msg & 15u) return fail(ctx, SRZ_E_INVALID, "srz_frameset_sparse_pack: the message must be 16-byte aligned");
  if (!fs->rendered) return fail(ctx, SRZ_E_INVALID, "srz_frameset_sparse_pack: the frameset has not been rendered");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick_stream(ctx, stream);
  if (!fs->d_sparse_rows) HIP_TRY(ctx, hipMalloc(&fs->d_sparse_rows, sizeof(uint32_t) * std::max<size_t>((size_t)fs->n_frames * fs->bands_per_rank, 1)));
  SparseArgs a = sparse_args(fs, what);
  a.shard = d_shard, a.msg = static_cast<uint8_t *>(d_msg);
  launch_sparse_pack(a, s);
  HIP_TRY(ctx, hipGetLastError());
  return SRZ_OK;
}

int srz_frameset_sparse_unpack(srz_ctx *ctx, const srz_frameset *fs, const void *d_recv, size_t msg_stride, void *d_gathered, int what,
                               void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  if (!fs || !d_recv || !d_gathered || !sparse_kind(what)) return fail(ctx, SRZ_E_INVALID, "srz_frameset_sparse_unpack: bad arguments");
  if (fs->shard_rank != ctx->shard_rank || fs->shard_world != ctx->shard_world)
    return fail(ctx, SRZ_E_INVALID, "srz_frameset_sparse_unpack: the frameset was created under a different shard");
  const SparseArgs a = sparse_args(fs, what);
  if (msg_stride < a.payload_off || (msg_stride & 15u) || ((uintptr_t)d_recv & 15u))
    return fail(ctx, SRZ_E_INVALID, "srz_frameset_sparse_unpack: the stride must be a multiple of 16 bytes of at least a message's header and "
                                    "table (" + std::to_string(a.payload_off) + " bytes), the messages 16-byte aligned");
  if (what == SRZ_EXCHANGE_PLANES && ((uintptr_t)d_gathered & 3u)) return fail(ctx, SRZ_E_INVALID, "srz_frameset_sparse_unpack: misaligned buffer");
  if (fs->shard_world == 1) return SRZ_OK; // (no peers)
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  launch_sparse_unpack(a, d_recv, msg_stride, d_gathered, pick_stream(ctx, stream));
  HIP_TRY(ctx, hipGetLastError());
  return SRZ_OK;
}

int srz_frameset_allgather_sparse(srz_ctx *ctx, srz_comm *c, const srz_frameset *fs, const void *d_msg, void *d_recv, size_t recv_bytes,
                                  void *d_gathered, int what, void *stream) {
  if (!ctx) return SRZ_E_INVALID;
  if (!c || !fs || !d_msg || !d_recv || !d_gathered) return fail(ctx, SRZ_E_INVALID, "srz_frameset_allgather_sparse: null argument");
  if (fs->shard_world != c->world || fs->shard_rank != c->rank)
    return fail(ctx, SRZ_E_INVALID, "srz_frameset_allgather_sparse: the frameset was not created under this communicator's shard");
  if (!sparse_kind(what)) return fail(ctx, SRZ_E_INVALID, "srz_frameset_allgather_sparse: bad exchange kind");
  if (((uintptr_t)d_msg | (uintptr_t)d_recv) & 15u) return fail(ctx, SRZ_E_INVALID, "srz_frameset_allgather_sparse: messages must be 16-byte aligned");
  if (what == SRZ_EXCHANGE_PLANES && ((uintptr_t)d_gathered & 3u)) return fail(ctx, SRZ_E_INVALID, "srz_frameset_allgather_sparse: misaligned buffer");
  if (c->world == 1) return SRZ_OK; // one rank: its shard is the whole buffer
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick_stream(ctx, stream);
  const size_t slot = srz_comm::SPARSE_SLOT, W = (size_t)c->world;
  if (!c->d_sizes) {
    HIP_TRY(ctx, hipMalloc(&c->d_sizes, slot * W));
    HIP_TRY(ctx, hipHostMalloc(&c->h_sizes, slot * W, hipHostMallocDefault));
  }
  // 1. every rank's header and recv_bytes.  (h_sizes is free: the previous call synchronised the stream after its last use)
  uint8_t *mine = c->d_sizes + slot * (size_t)c->rank;
  std::memcpy(c->h_sizes + slot * (size_t)c->rank + SPARSE_HEADER, &recv_bytes, sizeof recv_bytes);
  HIP_TRY(ctx, hipMemcpyAsync(mine, d_msg, SPARSE_HEADER, hipMemcpyDeviceToDevice, s));
  HIP_TRY(ctx, hipMemcpyAsync(mine + SPARSE_HEADER, c->h_sizes + slot * (size_t)c->rank + SPARSE_HEADER, sizeof recv_bytes, hipMemcpyHostToDevice, s));
  int rc = rccl().AllGather(mine, c->d_sizes, slot, /* ncclUint8 */ 1, c->comm, s);
  if (rc != 0) return fail(ctx, SRZ_E_NODEVICE, "ncclAllGather (message sizes): " + rccl_err(rc));
  // 2. the call's one blocking point: the host needs M, the largest message, to size the padded all-gather
  HIP_TRY(ctx, hipMemcpyAsync(c->h_sizes, c->d_sizes, slot * W, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  uint64_t m = 0, min_recv = ~0ull;
  int short_rank = -1;
  for (size_t r = 0; r < W; ++r) {
    uint64_t b = 0, rb = 0;
    std::memcpy(&b, c->h_sizes + slot * r + 8, sizeof b);
    std::memcpy(&rb, c->h_sizes + slot * r + SPARSE_HEADER, sizeof rb);
    m = std::max(m, b);
    if (rb < min_recv) min_recv = rb, short_rank = (int)r;
  }
  m = (m + 15u) & ~(uint64_t)15u;
  const size_t cap = srz_frameset_sparse_capacity(ctx, fs, what);
  // every rank sees the same numbers and takes the same branch: no rank fails alone between the two collectives
  if (m > cap || m < sparse_args(fs, what).payload_off)
    return fail(ctx, SRZ_E_INVALID, "srz_frameset_allgather_sparse: a message header announces " + std::to_string(m) +
                                        " bytes (capacity " + std::to_string(cap) + "): not a message of this frameset");
  if (min_recv < W * m)
    return fail(ctx, SRZ_E_NOMEM, "srz_frameset_allgather_sparse: rank " + std::to_string(short_rank) + " has a receive buffer of " +
                                      std::to_string(min_recv) + " bytes, " + std::to_string(W * m) + " needed (world x the largest message, " +
                                      std::to_string(m) + " bytes)");
  // 3. M bytes of every rank's message (d_msg holds the capacity, which is >= M), then the peers' tiles into d_gathered
  rc = rccl().AllGather(d_msg, d_recv, (size_t)m, /* ncclUint8 */ 1, c->comm, s);
  if (rc != 0) return fail(ctx, SRZ_E_NODEVICE, "ncclAllGather (messages): " + rccl_err(rc));
  return srz_frameset_sparse_unpack(ctx, fs, d_recv, (size_t)m, d_gathered, what, stream);
}

/* Page-locks `bytes` of the caller's memory at `ptr` (hipHostRegister): planes inside a registered range move between host and
 * device by DMA at the link's rate in srz_draw / srz_draw_scene / srz_draw_batch instead of through the runtime's staging copies. */
int srz_host_register(srz_ctx *ctx, void *ptr, size_t bytes) {
  if (!ctx || !ptr || !bytes) return ctx ? fail(ctx, SRZ_E_INVALID, "srz_host_register: null argument") : SRZ_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipHostRegister(ptr, bytes, hipHostRegisterDefault));
  return SRZ_OK;
}
int srz_host_unregister(srz_ctx *ctx, void *ptr) {
  if (!ctx || !ptr) return ctx ? fail(ctx, SRZ_E_INVALID, "srz_host_unregister: null argument") : SRZ_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (nothing of ours may still be copying from / to the range)
  HIP_TRY(ctx, hipHostUnregister(ptr));
  return SRZ_OK;
}

int srz_sync(srz_ctx *ctx) {
  if (!ctx) return SRZ_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return SRZ_OK;
}

// Re-upload the shading data of a set: each frame's eye, ka, ks, p, kh, kn, lights and flags, each batch's shader and texture (a sceneset's
// draws too: srz_sceneset_update writes them first; srz_draw's one-frame set its triangles, copy_tris).  The structure must be the set's
// (frame count, size, light and batch counts, triangles per batch): else SRZ_E_INVALID and the set is unchanged.  Asynchronous on the
// context's stream.
static int refresh_frames(srz_ctx *ctx, srz_frameset *fs, const srz_frame *frames, int n_frames, const char *who, bool copy_tris) {
  auto bad = [&](int code, const char *what) { return fail(ctx, code, std::string(who) + ": " + what); };
  if (n_frames != fs->n_frames) return bad(SRZ_E_INVALID, "frame count changed");
  for (int f = 0; f < n_frames; ++f) { // (everything is checked before anything changes)
    const srz_frame &fr = frames[f];
    const FrameDesc &d = fs->h_frames[f];
    if (fr.width != fs->width || fr.height != fs->height) return bad(SRZ_E_INVALID, "frame size changed");
    if (fr.n_lights != d.n_lights || (fr.n_lights && !fr.lights)) return bad(SRZ_E_INVALID, "light count changed");
    if (fr.n_batches != d.n_batches || (fr.n_batches && !fr.batches)) return bad(SRZ_E_INVALID, "batch count changed");
    for (uint32_t b = 0; b < fr.n_batches; ++b) {
      const srz_batch &sb = fr.batches[b];
      if (sb.n_tris != fs->h_batches[d.batch_off + b].count) return bad(SRZ_E_INVALID, "triangle count of a batch changed");
      if (sb.shader < SRZ_SHADER_NORMAL || sb.shader > SRZ_SHADER_BUMP) return bad(SRZ_E_INVALID, "unknown shader type");
      if (copy_tris && sb.n_tris && !sb.tris) return bad(SRZ_E_INVALID, "batch with null triangle pointer");
    }
  }
  if (int rc = ensure_stage_ring(ctx, fs, who)) return rc;
  bool batches_changed = false;
  for (int f = 0; f < n_frames; ++f) {
    const srz_frame &fr = frames[f];
    FrameDesc &d = fs->h_frames[f];
    set_shading(d, fr);
    if (fr.n_lights) std::memcpy(&fs->h_lights[d.light_off], fr.lights, sizeof(srz_light) * fr.n_lights);
    for (uint32_t b = 0; b < fr.n_batches; ++b) {
      BatchDesc &bd = fs->h_batches[d.batch_off + b];
      if (bd.shader != fr.batches[b].shader || bd.tex_id != fr.batches[b].tex_id)
        bd.shader = fr.batches[b].shader, bd.tex_id = fr.batches[b].tex_id, batches_changed = true;
    }
  }
  classify_frames(fs);
  // (the host copies of the descriptors are re-classified by now: if the lists for a new build kind cannot be had, the set stays
  // refused by render_impl until an update succeeds — its old lists are intact, but its frames no longer match them)
  fs->update_failed = ensure_worklists(fs) != hipSuccess;
  if (fs->update_failed) return bad(SRZ_E_NOMEM, "hipMalloc of the work lists failed");
  if (int rc = upload_dyn(ctx, fs)) return rc;
  if (batches_changed) fs->sdesc_version = 0; // re-resolve batch → shader / texture at the next render or shade
  if (copy_tris) {
    for (int f = 0; f < n_frames; ++f) {
      size_t o = fs->h_frames[f].tri_off;
      for (uint32_t b = 0; b < frames[f].n_batches; ++b) {
        const srz_batch &sb = frames[f].batches[b];
        if (sb.n_tris) HIP_TRY(ctx, hipMemcpyAsync(fs->d_tris + o, sb.tris, sizeof(srz_tri) * sb.n_tris, hipMemcpyHostToDevice, ctx->stream));
        o += sb.n_tris;
      }
    }
  }
  fs->have_stats = false;
  return SRZ_OK;
}

static int draw_impl(srz_ctx *ctx, int primitive, const srz_frame *frame, const srz_scene_frame *scene, float *z, float *c0,
                     float *c1, float *c2, srz_stats *stats) {
  if (!ctx) return SRZ_E_INVALID;
  if (primitive != SRZ_PRIMITIVE_LINES && primitive != SRZ_PRIMITIVE_TRIANGLES)
    return fail(ctx, SRZ_E_PRIMITIVE, "Primitive Type is not supported!");
  if ((!frame && !scene) || !z || !c0 || !c1 || !c2) return fail(ctx, SRZ_E_INVALID, "srz_draw: null argument");
  if (ctx->shard_world != 1) return fail(ctx, SRZ_E_INVALID, "srz_draw: whole-frame draw needs an unsharded ctx (srz_set_shard(ctx,0,1))");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int W = frame ? frame->width : scene->width, H = frame ? frame->height : scene->height;
  // ---- the structure of this call; equal to the previous call's → its frameset and framebuffer are reused ----------------
  std::vector<uint64_t> sig;
  if (frame) {
    if ((frame->n_lights && !frame->lights) || (frame->n_batches && !frame->batches)) return fail(ctx, SRZ_E_INVALID, "srz_draw: null lights/batches");
    sig = {1u, (uint64_t)(uint32_t)W << 32 | (uint32_t)H, frame->n_lights, frame->n_batches};
    for (uint32_t b = 0; b < frame->n_batches; ++b)
      sig.push_back((uint64_t)frame->batches[b].n_tris << 32 | (uint64_t)(uint8_t)frame->batches[b].shader << 16 | (uint16_t)frame->batches[b].tex_id);
  } else {
    sig = {2u, (uint64_t)(uint32_t)W << 32 | (uint32_t)H, scene->n_lights, scene->n_draws};
  }
  int rc = SRZ_OK;
  bool reuse = ctx->draw_fs && sig == ctx->draw_sig;
  if (reuse) {
    ctx->draw_fs->approx_shade = ctx->opt_approx_shade; // (the ctx's own one-frame set follows the option call by call)
    rc = frame ? refresh_frames(ctx, ctx->draw_fs, frame, 1, "srz_draw", /*copy_tris=*/true) : srz_sceneset_update(ctx, ctx->draw_fs, scene, 1);
    if (rc != SRZ_OK && !frame) reuse = false, rc = SRZ_OK; // (a scene whose mesh bindings changed: rebuild)
    if (rc != SRZ_OK) return rc;
  }
  if (!reuse) {
    if (ctx->draw_fs) srz_frameset_destroy(ctx, ctx->draw_fs);
    (void)hipFree(ctx->draw_out);
    ctx->draw_fs = nullptr, ctx->draw_out = nullptr, ctx->draw_sig.clear();
    rc = frame ? build_frameset(ctx, frame, 1, &ctx->draw_fs, true, /*tris_aos=*/true) : sceneset_create_impl(ctx, scene, 1, &ctx->draw_fs, false);
    if (rc) return rc;
    if (hipMalloc(&ctx->draw_out, 4 * (size_t)W * H * sizeof(float)) != hipSuccess) {
      srz_frameset_destroy(ctx, ctx->draw_fs);
      ctx->draw_fs = nullptr;
      return fail(ctx, SRZ_E_NOMEM, "srz_draw: hipMalloc failed");
    }
    ctx->draw_sig = sig;
  }
  srz_frameset *fs = ctx->draw_fs;
  float *d_out = ctx->draw_out;
  const uint32_t fflags = frame ? frame->flags : scene->flags;
  const size_t plane = (size_t)W * H, pb = plane * sizeof(float);
  hipError_t e = hipSuccess;
  const bool fused = (fflags & SRZ_FUSED_CLEAR) != 0;
  float *host[4] = {z, c0, c1, c2};
  if (!fused)
    for (int p = 0; p < 4 && e == hipSuccess; ++p) e = hipMemcpyAsync(d_out + p * plane, host[p], pb, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    if (stats) rc = stats_pass(ctx, fs, fused ? nullptr : d_out, 0, s, stats);
    if (rc == SRZ_OK) rc = render_impl(ctx, fs, d_out, 0, s, Pass::colour());
  }
  // (planes the caller page-locked with srz_host_register move by DMA straight from / to his memory; pageable ones through the
  // runtime's staging buffers.  SRZ_NO_Z_READBACK: the depth plane stays on the device)
  for (int p = (fflags & SRZ_NO_Z_READBACK) ? 1 : 0; p < 4 && e == hipSuccess && rc == SRZ_OK; ++p)
    e = hipMemcpyAsync(host[p], d_out + p * plane, pb, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(ctx, SRZ_E_NODEVICE, std::string("srz_draw: ") + hipGetErrorString(e));
  return rc;
}

int srz_draw(srz_ctx *ctx, int primitive, const srz_frame *frame, float *z, float *c0, float *c1, float *c2,
             srz_stats *stats) {
  if (ctx && !frame) return fail(ctx, SRZ_E_INVALID, "srz_draw: null argument");
  return draw_impl(ctx, primitive, frame, nullptr, z, c0, c1, c2, stats);
}

int srz_draw_scene(srz_ctx *ctx, int primitive, const srz_scene_frame *frame, float *z, float *c0, float *c1, float *c2,
                   srz_stats *stats) {
  if (ctx && !frame) return fail(ctx, SRZ_E_INVALID, "srz_draw_scene: null argument");
  return draw_impl(ctx, primitive, nullptr, frame, z, c0, c1, c2, stats);
}

int srz_draw_batch(srz_ctx *ctx, int primitive, const srz_frame *frames, int n_frames, float *const *planes, srz_stats *stats) {
  if (!ctx) return SRZ_E_INVALID;
  if (primitive != SRZ_PRIMITIVE_LINES && primitive != SRZ_PRIMITIVE_TRIANGLES)
    return fail(ctx, SRZ_E_PRIMITIVE, "Primitive Type is not supported!");
  if (!frames || n_frames <= 0 || !planes) return fail(ctx, SRZ_E_INVALID, "srz_draw_batch: null argument");
  for (int f = 0; f < n_frames; ++f)
    if (!planes[f]) return fail(ctx, SRZ_E_INVALID, "srz_draw_batch: null plane pointer");
  if (ctx->shard_world != 1) return fail(ctx, SRZ_E_INVALID, "srz_draw_batch: whole-frame draw needs an unsharded ctx");
  HIP_TRY(ctx, hipSetDevice(ctx->device)); // (the read-back stream first: a set is never left behind by its failure)
  if (!ctx->stream3)
    if (int rc = create_side(ctx, "srz_draw_batch", &ctx->stream3, false, ctx->ev_piece)) return rc;
  srz_frameset *fs = nullptr;
  int rc = srz_frameset_create(ctx, frames, n_frames, &fs);
  if (rc) return rc;
  const size_t fb = 4ull * (size_t)fs->width * (size_t)fs->height * sizeof(float); // one frame: z,c0,c1,c2 planes
  // (the device planes are kept between calls: allocating and freeing half a gigabyte costs as much as moving it)
  hipError_t e = hipSuccess;
  if (ctx->batch_out_bytes < fb * (size_t)n_frames) {
    (void)hipFree(ctx->batch_out);
    ctx->batch_out = nullptr, ctx->batch_out_bytes = 0;
    e = hipMalloc(&ctx->batch_out, fb * (size_t)n_frames);
    if (e != hipSuccess) {
      srz_frameset_destroy(ctx, fs);
      return fail(ctx, SRZ_E_NOMEM, "srz_draw_batch: hipMalloc failed");
    }
    ctx->batch_out_bytes = fb * (size_t)n_frames;
  }
  float *d_out = ctx->batch_out;
  hipStream_t s = ctx->stream;
  // The set is rendered in pieces of whole frames (~128 MB of planes each), all enqueued at once; a second stream brings piece k
  // back to the caller's planes while piece k + 1 renders (and, for accumulate-mode frames, while its planes go up) — with planes
  // the caller page-locked (srz_host_register) both directions are DMA at the link's rate, pageable ones go through the runtime's
  // staging copies.  A counting run (stats) renders in one piece first.
  const int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_frames, ((size_t)128 << 20) / fb));
  const int n_pieces = (n_frames + per - 1) / per;
  const size_t plane_b = fb / 4;
  if (stats) { // (frames with SRZ_FUSED_CLEAR ignore what the scratch copy holds)
    for (int f = 0; f < n_frames && e == hipSuccess; ++f)
      if (!(frames[f].flags & SRZ_FUSED_CLEAR))
        e = hipMemcpyAsync(reinterpret_cast<uint8_t *>(d_out) + fb * f, planes[f], fb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) rc = stats_pass(ctx, fs, d_out, 0, s, stats);
  }
  // (piece k's read-back is issued AFTER piece k + 1's render has been enqueued: a copy to pageable memory holds the calling thread
  // until it is done, and the device must have its next piece by then)
  auto read_back = [&](int k) {
    const int f0 = k * per, n = std::min(per, n_frames - f0);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream3, ctx->ev_piece[k % srz_ctx::EV_RING], 0); // "piece k has been rendered"
    for (int f = f0; f < f0 + n && e == hipSuccess; ++f) {
      const size_t skip = (frames[f].flags & SRZ_NO_Z_READBACK) ? plane_b : 0; // (the depth plane is the first of a frame's four)
      e = hipMemcpyAsync(reinterpret_cast<uint8_t *>(planes[f]) + skip, reinterpret_cast<uint8_t *>(d_out) + fb * f + skip, fb - skip,
                         hipMemcpyDeviceToHost, ctx->stream3);
    }
  };
  for (int k = 0; k < n_pieces && e == hipSuccess && rc == SRZ_OK; ++k) {
    const int f0 = k * per, n = std::min(per, n_frames - f0);
    if (!stats) // accumulate-mode frames start from the caller's planes (a counting run has uploaded them already)
      for (int f = f0; f < f0 + n && e == hipSuccess; ++f)
        if (!(frames[f].flags & SRZ_FUSED_CLEAR))
          e = hipMemcpyAsync(reinterpret_cast<uint8_t *>(d_out) + fb * f, planes[f], fb, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) break;
    rc = render_impl(ctx, fs, d_out, 0, s, Pass::colour_frames(f0, n));
    if (rc != SRZ_OK) break;
    e = hipEventRecord(ctx->ev_piece[k % srz_ctx::EV_RING], s); // (slot k % 8 was last waited for by piece k - 8's read-back, issued long ago)
    if (k > 0) read_back(k - 1);
  }
  if (e == hipSuccess && rc == SRZ_OK) read_back(n_pieces - 1);
  { // both streams drain before the buffers go, whatever happened above
    const hipError_t e1 = hipStreamSynchronize(s), e2 = hipStreamSynchronize(ctx->stream3);
    if (e == hipSuccess) e = e1 != hipSuccess ? e1 : e2;
  }
  srz_frameset_destroy(ctx, fs);
  if (e != hipSuccess) return fail(ctx, SRZ_E_NODEVICE, std::string("srz_draw_batch: ") + hipGetErrorString(e));
  return rc;
}

} // extern "C"
