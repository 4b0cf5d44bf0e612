/* The G-buffer's test reference (tests/gbufref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math).  Written from the
 * reference's source and the oracle's text, it includes nothing of the library: per pixel of a visibility buffer (owner id word,
 * alpha, beta) the attributes the reference's two fragment paths hand to their shaders,
 *   V (processFragByAVX2, src/Rasterizer.cpp:380-389): gamma = 1 - (alpha + beta); normal and uv by fmaf chains; NormalSIMD::normalized
 *     (src/Tools.cpp:13-24: a length that is not > 0 gives the zero vector); kd of the TEXTURE shader = getTextureColor<__m256>
 *     (include/loader/TextureLoader.hpp:51-101) behind the prologue of src/Shader.cpp:134-140: cvtps_epi32 of the scaled coordinate
 *     clamped to [0, size - 1], the texel times rcp(255) — correctly rounded here, as the oracle has it;
 *   S (processFragByScalar, src/Rasterizer.cpp:470-492): gamma = 1 - alpha - beta; products and sums; glm::normalize = v * (1 / sqrt(dot));
 *     kd of TEXTURE / BUMP / DISPLACEMENT = getTextureColor(vec2) (src/TextureLoader.cpp:14-31): clamp to [0, 1], scale, truncate,
 *     black outside, texel / 255.
 * fmaf where the reference fuses and nothing else fused. */
#include <math.h>
#include <stdint.h>
#include <stddef.h>

#define SH_NORMAL 0
#define SH_TEXTURE 1
#define SH_PHONG 2
#define SH_DISPLACEMENT 3
#define SH_BUMP 4

typedef struct {
  int32_t shader, tw, th, _pad;
  const uint8_t *bgr; /* th rows of tw BGR texels, tightly packed; NULL: no texture (the batch's albedo is then left at (1, 1, 1):
                       * a caller without the texture compares the other groups only) */
} gr_batch;

static float sse_max(float a, float b) { return a > b ? a : b; }
static float sse_min(float a, float b) { return a < b ? a : b; }
static float std_clamp(float v, float lo, float hi) { return (v < lo) ? lo : (hi < v) ? hi : v; }
static int32_t cvtps_epi32(float f) { /* round to nearest even; out of range -> 0x80000000 */
  if (!(f >= -2147483648.0f && f < 2147483648.0f)) return INT32_MIN;
  return (int32_t)lrintf(f);
}
static int32_t cvttss_si32(float f) { /* truncation; NaN and everything outside int32 -> 0x80000000 */
  if (!(f >= -2147483648.0f && f < 2147483648.0f)) return INT32_MIN;
  return (int32_t)f;
}
static uint32_t bits(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }

/* out: 9 planes of n_px words — nx ny nz | u v | batch + 1 | kd0 kd1 kd2.  A pixel nobody owns (id 0, or an index outside the n_tris
 * triangles): zeros when fused, else its words stay.  tris: n_tris records of 24 floats (pos 9, nrm 9, uv 6); tri_batch: each
 * triangle's batch. */
void gr_gbuffer(const float *tris, uint32_t n_tris, const int32_t *tri_batch, const gr_batch *batches, size_t n_px, const uint32_t *id,
                const float *al, const float *be, int fused, uint32_t *out) {
  for (size_t p = 0; p < n_px; ++p) {
    const uint32_t w = id[p], idx = (w & 0x7fffffffu) - 1u;
    if (idx >= n_tris) {
      if (fused)
        for (int k = 0; k < 9; ++k) out[k * n_px + p] = 0u;
      continue;
    }
    const int isS = (w >> 31) != 0;
    const float *t = tris + 24 * (size_t)idx, *nr = t + 9, *uv = t + 18;
    const float alpha = al[p], beta = be[p];
    const gr_batch *b = batches + tri_batch[idx];
    float n[3], u, v, kd[3] = {1.0f, 1.0f, 1.0f};
    if (!isS) {
      const float gamma = 1.0f - (alpha + beta);
      for (int c = 0; c < 3; ++c) n[c] = fmaf(alpha, nr[c], fmaf(beta, nr[3 + c], gamma * nr[6 + c]));
      const float len = sqrtf(fmaf(n[0], n[0], fmaf(n[1], n[1], n[2] * n[2])));
      if (len > 0.0f) {
        const float inv = 1.0f / len;
        n[0] = n[0] * inv, n[1] = n[1] * inv, n[2] = n[2] * inv;
      } else {
        n[0] = n[1] = n[2] = 0.0f;
      }
      u = fmaf(alpha, uv[0], fmaf(beta, uv[2], gamma * uv[4]));
      v = fmaf(alpha, uv[1], fmaf(beta, uv[3], gamma * uv[5]));
      if (b->shader == SH_TEXTURE && b->bgr) {
        const float tw = (float)b->tw, th = (float)b->th;
        float su = u * tw, sv = v * th;
        su = sse_max(0.0f, sse_min(su, tw - 1.0f));
        sv = sse_max(0.0f, sse_min(sv, th - 1.0f));
        const int32_t xi = cvtps_epi32(su), yi = cvtps_epi32(sv);
        const uint8_t *px = b->bgr + ((size_t)yi * b->tw + xi) * 3;
        const float inv255 = 1.0f / 255.0f;
        kd[0] = (float)px[0] * inv255, kd[1] = (float)px[1] * inv255, kd[2] = (float)px[2] * inv255;
      }
    } else {
      const float gamma = 1.0f - alpha - beta;
      for (int c = 0; c < 3; ++c) n[c] = alpha * nr[c] + beta * nr[3 + c] + gamma * nr[6 + c];
      const float is = 1.0f / sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      n[0] = n[0] * is, n[1] = n[1] * is, n[2] = n[2] * is;
      u = alpha * uv[0] + beta * uv[2] + gamma * uv[4];
      v = alpha * uv[1] + beta * uv[3] + gamma * uv[5];
      if ((b->shader == SH_TEXTURE || b->shader == SH_BUMP || b->shader == SH_DISPLACEMENT) && b->bgr) {
        const float cu = std_clamp(u, 0.0f, 1.0f), cv = std_clamp(v, 0.0f, 1.0f);
        const float fx = cu * (float)b->tw, fy = cv * (float)b->th;
        const int x = cvttss_si32(fx), y = cvttss_si32(fy);
        if (x < 0 || x >= b->tw || y < 0 || y >= b->th) {
          kd[0] = kd[1] = kd[2] = 0.0f;
        } else {
          const uint8_t *px = b->bgr + ((size_t)y * b->tw + x) * 3;
          kd[0] = px[0] / 255.0f, kd[1] = px[1] / 255.0f, kd[2] = px[2] / 255.0f;
        }
      }
    }
    out[0 * n_px + p] = bits(n[0]), out[1 * n_px + p] = bits(n[1]), out[2 * n_px + p] = bits(n[2]);
    out[3 * n_px + p] = bits(u), out[4 * n_px + p] = bits(v);
    out[5 * n_px + p] = (uint32_t)tri_batch[idx] + 1u;
    out[6 * n_px + p] = bits(kd[0]), out[7 * n_px + p] = bits(kd[1]), out[8 * n_px + p] = bits(kd[2]);
  }
}
