/* CPU-only: the oracle (oracle/srz_oracle.c) under AddressSanitizer + UBSan on seeded adversarial frames — odd sizes, every
 * shader type incl. BUMP / DISPLACEMENT on a 3 x 5 texture, 0..5 lights, triangles that are degenerate, far off screen, huge,
 * non-finite, exactly on pixel centres.  Built by `make -C oracle asan`, run by tests/test_host_fuzz.py.  The oracle is test
 * infrastructure; this only checks that the checker itself reads and writes inside its buffers.
 *   oracle_asan <frames> <seed>     prints "frames=<n> visible=<sum>" and exits 0
 *   oracle_asan --file <path>       the same for frames a test wrote (tests/support.py dump_frames: the hostile shading inputs of
 *                                   tests/test_oracle_shading_edges.py), little-endian: "SRZF", u32 textures, per texture i32 slot, w, h,
 *                                   row_stride + row_stride * h bytes; u32 frames, per frame i32 w, h, f32 eye[3] ka[3] ks[3] p kh kn,
 *                                   u32 lights, batches, flags, the lights (6 f32 each), per batch i32 shader, tex_id, u32 n + n srz_tri */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/srz.h"

int orc_draw(int primitive, const srz_frame *fr, float *z, float *c0, float *c1, float *c2, srz_stats *st);
int orc_draw_omp(const srz_frame *fr, float *z, float *c0, float *c1, float *c2, int band, int *threads_used, int num_threads);
int orc_draw_rows(const srz_frame *fr, float *z, float *c0, float *c1, float *c2, int row0, int row1);
int orc_texture_set(int tex_id, const uint8_t *bgr, int w, int h, int row_stride);
void orc_resolve8(int W, int H, const float *c0, const float *c1, const float *c2, uint8_t *bgr8);

static uint64_t st;
static uint64_t rnd(void) {
  st ^= st << 13, st ^= st >> 7, st ^= st << 17;
  return st;
}
static float unit(void) { return (float)(rnd() >> 40) / 16777216.0f; }
static float coord(int size) {
  switch (rnd() % 12) {
  case 0: return -1e6f * unit();
  case 1: return 1e6f * unit();
  case 2: return (float)(rnd() % (uint64_t)(size + 1));        /* exactly on a pixel corner / centre */
  case 3: return NAN;
  case 4: return (rnd() & 1) ? INFINITY : -INFINITY;
  case 5: return -0.0f;
  default: return unit() * (float)size * 1.2f - 0.1f * (float)size;
  }
}

static void need(FILE *in, void *dst, size_t n) {
  if (n && fread(dst, 1, n, in) != n) {
    fprintf(stderr, "oracle_asan: short file\n");
    exit(2);
  }
}

static void bad_file(const char *what) {
  fprintf(stderr, "oracle_asan: bad file (%s)\n", what);
  exit(2);
}
static void *must(void *p) {
  if (!p) bad_file("out of memory");
  return p;
}

static int run_file(const char *path) {
  FILE *in = fopen(path, "rb");
  if (!in) return 2;
  char magic[4];
  uint32_t n_tex, n_frames;
  need(in, magic, 4), need(in, &n_tex, 4);
  if (memcmp(magic, "SRZF", 4) != 0 || n_tex > 64) bad_file("header");
  for (uint32_t i = 0; i < n_tex; ++i) {
    int32_t q[4];
    need(in, q, sizeof q);
    if (q[1] < 1 || q[1] > 4096 || q[2] < 1 || q[2] > 4096 || q[3] < 3 * q[1] || q[3] > 3 * 4096 + 4096) bad_file("texture size");
    uint8_t *px = (uint8_t *)must(malloc((size_t)q[3] * q[2])); /* exactly row_stride * h bytes */
    need(in, px, (size_t)q[3] * q[2]);
    int rc = orc_texture_set(q[0], px, q[1], q[2], q[3]);
    free(px);
    if (rc != SRZ_OK) bad_file("texture refused");
  }
  need(in, &n_frames, 4);
  unsigned long long visible = 0;
  for (uint32_t f = 0; f < n_frames; ++f) {
    srz_frame fr;
    memset(&fr, 0, sizeof fr);
    int32_t wh[2];
    float k[12];
    uint32_t u[3];
    need(in, wh, sizeof wh), need(in, k, sizeof k), need(in, u, sizeof u);
    if (wh[0] < 1 || wh[0] > 4096 || wh[1] < 1 || wh[1] > 4096 || u[0] > 64 || u[1] > 64) bad_file("frame size or counts");
    fr.width = wh[0], fr.height = wh[1];
    memcpy(fr.eye, k, 12), memcpy(fr.ka, k + 3, 12), memcpy(fr.ks, k + 6, 12);
    fr.p = k[9], fr.kh = k[10], fr.kn = k[11];
    fr.n_lights = u[0], fr.n_batches = u[1], fr.flags = u[2];
    srz_light *lights = (srz_light *)must(malloc(sizeof(srz_light) * (u[0] ? u[0] : 1)));
    need(in, lights, sizeof(srz_light) * u[0]);
    srz_batch *batches = (srz_batch *)must(calloc(u[1] ? u[1] : 1, sizeof(srz_batch)));
    for (uint32_t b = 0; b < u[1]; ++b) {
      int32_t st2[2];
      uint32_t n;
      need(in, st2, sizeof st2), need(in, &n, 4);
      if (n > (1u << 20)) bad_file("triangle count");
      srz_tri *t = (srz_tri *)must(malloc(sizeof(srz_tri) * (n ? n : 1)));
      need(in, t, sizeof(srz_tri) * n);
      batches[b].shader = st2[0], batches[b].tex_id = st2[1], batches[b].n_tris = n, batches[b].tris = t;
    }
    fr.lights = lights, fr.batches = batches;
    const size_t px = (size_t)fr.width * fr.height;
    float *pl = (float *)must(malloc(sizeof(float) * 4 * px));
    srz_stats s;
    int used = 0;
    int rc = orc_draw(SRZ_PRIMITIVE_TRIANGLES, &fr, pl, pl + px, pl + 2 * px, pl + 3 * px, &s);
    if (rc == SRZ_OK) visible += s.visible;
    rc |= orc_draw_omp(&fr, pl, pl + px, pl + 2 * px, pl + 3 * px, 8, &used, 2) < 0;
    free(pl), free(lights);
    for (uint32_t b = 0; b < u[1]; ++b) free((void *)batches[b].tris);
    free(batches);
    if (rc != SRZ_OK) {
      fprintf(stderr, "oracle_asan: frame %u returned %d\n", f, rc);
      fclose(in);
      return 1;
    }
  }
  fclose(in);
  printf("frames=%u visible=%llu\n", n_frames, visible);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 2 && strcmp(argv[1], "--file") == 0) return run_file(argv[2]);
  const int n_frames = argc > 1 ? atoi(argv[1]) : 40;
  st = 0x2545f4914f6cdd1dull ^ (uint64_t)(argc > 2 ? atoll(argv[2]) : 1);
  uint8_t tex[3 * 5 * 3];
  for (size_t i = 0; i < sizeof tex; ++i) tex[i] = (uint8_t)rnd();
  if (orc_texture_set(0, tex, 3, 5, 9) != SRZ_OK) return 1;
  unsigned long long visible = 0;
  for (int f = 0; f < n_frames; ++f) {
    const int W = 1 + (int)(rnd() % 97), H = 1 + (int)(rnd() % 71);
    const uint32_t n_batches = 1 + (uint32_t)(rnd() % 4), n_lights = (uint32_t)(rnd() % 6);
    srz_light lights[6];
    for (uint32_t l = 0; l < n_lights; ++l)
      for (int k = 0; k < 3; ++k) lights[l].pos[k] = coord(W), lights[l].intensity[k] = 500.0f * unit();
    srz_batch batches[4];
    srz_tri *tris[4];
    for (uint32_t b = 0; b < n_batches; ++b) {
      const uint32_t n = (uint32_t)(rnd() % 40);
      tris[b] = (srz_tri *)malloc(sizeof(srz_tri) * (n ? n : 1));
      for (uint32_t t = 0; t < n; ++t) {
        srz_tri *q = &tris[b][t];
        const int wild = (int)(rnd() % 4) == 0;
        const float cx = unit() * (float)W, cy = unit() * (float)H, r = 1.0f + unit() * 30.0f;
        for (int v = 0; v < 3; ++v) {
          q->pos[v][0] = wild ? coord(W) : cx + (unit() - 0.5f) * r, q->pos[v][1] = wild ? coord(H) : cy + (unit() - 0.5f) * r;
          q->pos[v][2] = wild ? coord(50) : 0.1f + unit() * 49.0f;
          for (int k = 0; k < 3; ++k) q->nrm[v][k] = (rnd() % 16 == 0) ? 0.0f : unit() * 2.0f - 1.0f;
          q->uv[v][0] = (rnd() % 8 == 0) ? coord(2) : unit(), q->uv[v][1] = (rnd() % 8 == 0) ? 1.0f : unit();
        }
        if (rnd() % 10 == 0) memcpy(q->pos[1], q->pos[0], sizeof q->pos[0]); /* degenerate */
      }
      batches[b].shader = (int32_t)(rnd() % 5), batches[b].tex_id = 0, batches[b].n_tris = n, batches[b]._pad = 0, batches[b].tris = tris[b];
    }
    srz_frame fr;
    memset(&fr, 0, sizeof fr);
    fr.width = W, fr.height = H;
    for (int k = 0; k < 3; ++k) fr.eye[k] = coord(W), fr.ka[k] = 0.005f, fr.ks[k] = 0.7937f;
    static const float ps[] = {150.0f, 0.0f, 1.0f, 7.5f, 3000.0f};
    fr.p = ps[rnd() % 5], fr.kh = 0.2f, fr.kn = 0.1f;
    fr.n_lights = n_lights, fr.n_batches = n_batches, fr.lights = lights, fr.batches = batches;
    fr.flags = (rnd() & 1) ? SRZ_FUSED_CLEAR : 0u;
    if (rnd() % 8 == 0) fr.flags |= SRZ_UNIFIED;
    const size_t px = (size_t)W * H;
    float *pl = (float *)malloc(sizeof(float) * 4 * px); /* exactly W*H per plane: ASan sees any stray access */
    float *z = pl, *c0 = pl + px, *c1 = pl + 2 * px, *c2 = pl + 3 * px;
    for (size_t i = 0; i < px; ++i) z[i] = (rnd() % 50 == 0) ? NAN : INFINITY, c0[i] = c1[i] = c2[i] = 0.0f;
    srz_stats s;
    int used = 0;
    int rc = orc_draw(SRZ_PRIMITIVE_TRIANGLES, &fr, z, c0, c1, c2, &s);
    if (rc == SRZ_OK) visible += s.visible;
    rc |= orc_draw_omp(&fr, z, c0, c1, c2, 8, &used, 2) < 0;
    rc |= orc_draw_rows(&fr, z, c0, c1, c2, H / 3, H);
    uint8_t *img = (uint8_t *)malloc(3 * px);
    orc_resolve8(W, H, c0, c1, c2, img);
    free(img), free(pl);
    for (uint32_t b = 0; b < n_batches; ++b) free(tris[b]);
    if (rc != SRZ_OK) {
      fprintf(stderr, "oracle_asan: frame %d returned %d\n", f, rc);
      return 1;
    }
  }
  printf("frames=%d visible=%llu\n", n_frames, visible);
  return 0;
}
