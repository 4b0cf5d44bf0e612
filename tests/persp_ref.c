/* The perspective-correct barycentrics' test reference (tests/perspref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math).
 * It includes nothing of the library and is the executable statement of the rule include/srz.h gives for
 * srz_frameset_perspective, _perspective_grad and _interpolate_deriv_persp.  Per owned pixel of a visibility buffer (owner id word,
 * alpha, beta; gamma = 1 - (alpha + beta) for V, 1 - alpha - beta for S) with q0, q1, q2 the owner's reciprocal clip w:
 *   n0 = alpha * q0;  n1 = beta * q1;  n2 = gamma * q2;  s = (n0 + n1) + n2
 *   valid = q0, q1, q2 and s are positive normal floats (x >= 2^-126 && x < INFINITY)
 *   forward   valid: alpha' = n0 / s, beta' = n1 / s; else the words of alpha, beta; z, id and nobody's four words copied
 *   backward  t = fmaf(ga, alpha', gb * beta'); r = 1.0f / s; g0 = (ga - t) * r; g1 = (gb - t) * r; g2 = (-t) * r
 *             galpha = fmaf(g0, q0, -(g2 * q2)); gbeta = fmaf(g1, q1, -(g2 * q2)); gq += g0 * alpha, g1 * beta, g2 * gamma
 *             not valid: galpha = ga, gbeta = gb, no add
 *   deriv     e_k = (corner_k - u) * q_k with u interpolated under alpha', beta', gamma' as the owner's class interpolates;
 *             d/dx = fmaf(e0 - e2, gax, (e1 - e2) * gbx) / s, d/dy with gay, gby; not valid: the screen-linear constants
 * float32 throughout, fmaf where written and nothing else fused; the gradient with respect to q in DOUBLE (the sum of the float32
 * terms, added exactly enough to stand for the exact sum), with the count of contributing pixels per triangle and the sum of |term|
 * per element, from which the tests derive their bound. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

static float as_f(uint32_t w) {
  float f;
  memcpy(&f, &w, 4);
  return f;
}
static uint32_t as_u(float f) {
  uint32_t w;
  memcpy(&w, &f, 4);
  return w;
}
static int ok(float x) { return x >= 0x1p-126f && x < INFINITY; }

typedef struct {
  float ap, bp, s, gamma;
  int valid;
} px_t;

static px_t pixel(uint32_t w, float alpha, float beta, const float *q) {
  px_t r;
  r.gamma = (w >> 31) ? 1.0f - alpha - beta : 1.0f - (alpha + beta);
  const float n0 = alpha * q[0], n1 = beta * q[1], n2 = r.gamma * q[2];
  r.s = (n0 + n1) + n2;
  r.valid = ok(q[0]) && ok(q[1]) && ok(q[2]) && ok(r.s);
  r.ap = r.valid ? n0 / r.s : alpha, r.bp = r.valid ? n1 / r.s : beta;
  return r;
}

/* q: [n_tris][3]; z, id, al, be: the four planes of one frame's visibility buffer as words, n_px each; out: four planes of n_px
 * words, every one written. */
void pr_forward(const float *q, uint32_t n_tris, size_t n_px, const uint32_t *z, const uint32_t *id, const uint32_t *al, const uint32_t *be,
                uint32_t *out) {
  for (size_t p = 0; p < n_px; ++p) {
    const uint32_t w = id[p], idx = (w & 0x7fffffffu) - 1u;
    out[p] = z[p], out[n_px + p] = w, out[2 * n_px + p] = al[p], out[3 * n_px + p] = be[p];
    if (idx >= n_tris) continue;
    const px_t r = pixel(w, as_f(al[p]), as_f(be[p]), q + (size_t)idx * 3u);
    if (r.valid) out[2 * n_px + p] = as_u(r.ap), out[3 * n_px + p] = as_u(r.bp);
  }
}

/* gbp: the two planes of the gradient with respect to alpha', beta' (words at nobody's pixels are never read).  gq, gabs:
 * [n_tris][3] doubles, added into; count: [n_tris] valid pixels, added into (any of the three may be null).  gbary: 2 planes of
 * n_px (null: not wanted); a nobody pixel: 0 when fused, else its words stay. */
void pr_grad(const float *q, uint32_t n_tris, size_t n_px, const uint32_t *id, const uint32_t *al, const uint32_t *be, const float *gbp,
             int fused, double *gq, double *gabs, uint32_t *count, float *gbary) {
  for (size_t p = 0; p < n_px; ++p) {
    const uint32_t w = id[p], idx = (w & 0x7fffffffu) - 1u;
    if (idx >= n_tris) {
      if (fused && gbary) gbary[p] = 0.0f, gbary[n_px + p] = 0.0f;
      continue;
    }
    const float *qt = q + (size_t)idx * 3u;
    const float alpha = as_f(al[p]), beta = as_f(be[p]);
    const px_t r = pixel(w, alpha, beta, qt);
    const float ga = gbp[p], gb = gbp[n_px + p];
    if (!r.valid) {
      if (gbary) gbary[p] = ga, gbary[n_px + p] = gb;
      continue;
    }
    const float t = fmaf(ga, r.ap, gb * r.bp), rs = 1.0f / r.s;
    const float g0 = (ga - t) * rs, g1 = (gb - t) * rs, g2 = (-t) * rs;
    const float m = g2 * qt[2];
    if (gbary) gbary[p] = fmaf(g0, qt[0], -m), gbary[n_px + p] = fmaf(g1, qt[1], -m);
    const float term[3] = {g0 * alpha, g1 * beta, g2 * r.gamma}; /* the float32 products the pass adds */
    if (count) count[idx] += 1u;
    for (int k = 0; k < 3; ++k) {
      if (gq) gq[(size_t)idx * 3u + k] += (double)term[k];
      if (gabs) gabs[(size_t)idx * 3u + k] += fabs((double)term[k]);
    }
  }
}

/* pos: [n_tris][9] ax ay z0 bx by z1 cx cy z2; attr: [n_tris][3][n_ch]; out: 2 * n_ch planes of n_px. */
void pr_deriv(const float *q, const float *pos, const float *attr, uint32_t n_ch, uint32_t n_tris, size_t n_px, const uint32_t *id,
              const uint32_t *al, const uint32_t *be, int fused, float *out) {
  for (size_t p = 0; p < n_px; ++p) {
    const uint32_t w = id[p], idx = (w & 0x7fffffffu) - 1u;
    if (idx >= n_tris) {
      if (fused)
        for (uint32_t ch = 0; ch < 2u * n_ch; ++ch) out[ch * n_px + p] = 0.0f;
      continue;
    }
    const float *P = pos + (size_t)idx * 9u, *qt = q + (size_t)idx * 3u, *t = attr + (size_t)idx * 3u * n_ch;
    const float area = (P[3] - P[0]) * (P[7] - P[1]) - (P[4] - P[1]) * (P[6] - P[0]);
    const float rr = 1.0f / area;
    const float gax = (P[4] - P[7]) * rr, gay = (P[6] - P[3]) * rr, gbx = (P[7] - P[1]) * rr, gby = (P[0] - P[6]) * rr;
    const px_t r = pixel(w, as_f(al[p]), as_f(be[p]), qt);
    const float gp = (w >> 31) ? 1.0f - r.ap - r.bp : 1.0f - (r.ap + r.bp);
    for (uint32_t ch = 0; ch < n_ch; ++ch) {
      const float a = t[ch], b = t[n_ch + ch], c = t[2u * n_ch + ch];
      float dx, dy;
      if (r.valid) {
        const float u = (w >> 31) ? r.ap * a + r.bp * b + gp * c : fmaf(r.ap, a, fmaf(r.bp, b, gp * c));
        const float e0 = (a - u) * qt[0], e1 = (b - u) * qt[1], e2 = (c - u) * qt[2];
        dx = fmaf(e0 - e2, gax, (e1 - e2) * gbx) / r.s, dy = fmaf(e0 - e2, gay, (e1 - e2) * gby) / r.s;
      } else {
        const float da = a - c, db = b - c;
        dx = fmaf(da, gax, db * gbx), dy = fmaf(da, gay, db * gby);
      }
      out[(2u * ch) * n_px + p] = dx, out[(2u * ch + 1u) * n_px + p] = dy;
    }
  }
}
