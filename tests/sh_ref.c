/* The SH9 passes' test reference (tests/shref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math; no flush to zero).  It
 * includes nothing of the library.  The rules include/srz.h states for srz_cube_sh, srz_cube_sh_grad, srz_frameset_sh and the order
 * of operations it fixes for srz_frameset_sh_grad are written down ONCE, below, in terms of a type `real`; this file includes itself
 * twice, so that the one text exists as binary32 (sr32_*: the rule itself, what the GPU is held to bit for bit) and as binary64
 * (sr64_*: the same operations carried out in double, what the binary32 build's error is measured against).  The constants are the
 * header's binary32 values in both builds: they are the rule's data, not its arithmetic.
 *   cube_sh:      a cube -> nine coefficients per channel and the normaliser, in the header's FIXED TREE restated literally: 64 lane
 *                 sums per face row, the butterfly as a loop over all 64 lanes, rows then faces by plain adds;
 *   cube_sh_grad: the gather per source texel;
 *   forward:      the coefficients at each pixel's normal;
 *   grad:         the normal's gradient planes, and per coefficient the pixel's term g_c * e_k ACCUMULATED IN DOUBLE with the sum of
 *                 |term| and the count of contributing pixels, from which the tests derive their bound. */
#ifndef SR_BODY
#include <math.h>
#include <stddef.h>
#include <stdint.h>

static int owned(uint32_t id, uint32_t n_tris) { return ((id & 0x7fffffffu) - 1u) < n_tris; }
static const float YC[5] = {0x1.20dd76p-2f, 0x1.f45438p-2f, 0x1.17b142p+0f, 0x1.42f602p-2f, 0x1.17b142p-1f};
static const float HC[5] = {0x1.20dd76p-2f, 0x1.4d8d7ap-2f, 0x1.17b142p-2f, 0x1.42f602p-4f, 0x1.17b142p-3f};
static const int CIDX[9] = {0, 1, 1, 1, 2, 2, 3, 2, 4};
static const float FOURPI = 12.566371f;

#define SR_BODY
#define real float
#define SR(name) sr32_##name
#define SQRT sqrtf
#define FMA fmaf
#include "sh_ref.c"
#undef real
#undef SR
#undef SQRT
#undef FMA
#define real double
#define SR(name) sr64_##name
#define SQRT sqrt
#define FMA fma
#include "sh_ref.c"

#else /* ---------------------------------------------------------------------------------------- the rules, once, in `real` */

static real SR(dot)(const real *a, const real *b) { return FMA(a[0], b[0], FMA(a[1], b[1], a[2] * b[2])); }
static int SR(pos)(real x) { return x > 0 && x < (real)INFINITY; }
static void SR(poly)(real x, real y, real z, real *p) {
  p[0] = 1, p[1] = y, p[2] = z, p[3] = x, p[4] = x * y, p[5] = y * z;
  p[6] = FMA((real)3 * z, z, (real)-1), p[7] = x * z, p[8] = FMA(x, x, -(y * y));
}
/* srz_cube_prefilter's texel geometry of texel (f, y, x) at N, then w_k = jac * (Yc[k] * p_k(d)); -> jac */
static real SR(texel)(uint32_t N, uint32_t f, uint32_t y, uint32_t x, real *w) {
  const real s = (real)(2u * x + 1u) / (real)N - (real)1, t = (real)(2u * y + 1u) / (real)N - (real)1;
  const real r2 = FMA(s, s, FMA(t, t, (real)1)), inv = (real)1 / SQRT(r2);
  real px, py, pz;
  switch (f) {
  case 0: px = 1, py = -t, pz = -s; break;
  case 1: px = -1, py = -t, pz = s; break;
  case 2: px = s, py = 1, pz = t; break;
  case 3: px = s, py = -1, pz = -t; break;
  case 4: px = s, py = -t, pz = 1; break;
  default: px = -s, py = -t, pz = -1; break;
  }
  const real jac = (inv * inv) * inv;
  real p[9];
  SR(poly)(px * inv, py * inv, pz * inv, p);
  for (int k = 0; k < 9; ++k) w[k] = jac * ((real)YC[CIDX[k]] * p[k]);
  return jac;
}
/* the 64 lane sums of one slot through the butterfly -> what every lane ends with (lane 0's word) */
static real SR(butterfly)(real *lane) {
  for (int o = 32; o > 0; o >>= 1) {
    real nv[64];
    for (int l = 0; l < 64; ++l) nv[l] = lane[l] + lane[l ^ o];
    for (int l = 0; l < 64; ++l) lane[l] = nv[l];
  }
  return lane[0];
}
/* src: [frames][6][n][n][C]; sh: [frames][9][C]; den: one real or null */
void SR(cube_sh)(uint32_t n, uint32_t C, uint32_t frames, const real *src, real *sh, real *den_out) {
  const uint32_t K = 9u * C + 1u;
  for (uint32_t fr = 0; fr < frames; ++fr) {
    real cube[64];
    for (uint32_t e = 0; e < K; ++e) cube[e] = 0;
    for (uint32_t f = 0; f < 6u; ++f) {
      real face[64];
      for (uint32_t e = 0; e < K; ++e) face[e] = 0;
      for (uint32_t y = 0; y < n; ++y) {
        const real *row = src + (((size_t)fr * 6u + f) * n + y) * (size_t)n * C;
        static real lane[64][64]; /* [slot][lane] */
        for (uint32_t e = 0; e < K; ++e)
          for (int j = 0; j < 64; ++j) lane[e][j] = 0;
        for (uint32_t j = 0; j < 64u; ++j)
          for (uint32_t x = j; x < n; x += 64u) {
            real w[9];
            const real jac = SR(texel)(n, f, y, x, w);
            for (uint32_t k = 0; k < 9u; ++k)
              for (uint32_t c = 0; c < C; ++c) lane[k * C + c][j] = FMA(w[k], row[(size_t)x * C + c], lane[k * C + c][j]);
            lane[9u * C][j] = lane[9u * C][j] + jac;
          }
        for (uint32_t e = 0; e < K; ++e) face[e] = face[e] + SR(butterfly)(lane[e]);
      }
      for (uint32_t e = 0; e < K; ++e) cube[e] = cube[e] + face[e];
    }
    for (uint32_t e = 0; e < 9u * C; ++e) sh[(size_t)fr * 9u * C + e] = ((real)FOURPI * cube[e]) / cube[9u * C];
    if (den_out && fr == 0u) den_out[0] = cube[9u * C];
  }
}
/* gsh: [frames][9][C]; den: one real; gsrc: [frames][6][n][n][C], written */
void SR(cube_sh_grad)(uint32_t n, uint32_t C, uint32_t frames, const real *gsh, const real *den, real *gsrc) {
  for (uint32_t fr = 0; fr < frames; ++fr) {
    real q[63];
    for (uint32_t e = 0; e < 9u * C; ++e) q[e] = ((real)FOURPI * gsh[(size_t)fr * 9u * C + e]) / den[0];
    for (uint32_t f = 0; f < 6u; ++f)
      for (uint32_t y = 0; y < n; ++y)
        for (uint32_t x = 0; x < n; ++x) {
          real w[9];
          SR(texel)(n, f, y, x, w);
          real *g = gsrc + ((((size_t)fr * 6u + f) * n + y) * (size_t)n + x) * C;
          for (uint32_t c = 0; c < C; ++c) {
            real v = w[0] * q[c];
            for (uint32_t k = 1; k < 9u; ++k) v = FMA(w[k], q[k * C + c], v);
            g[c] = v;
          }
        }
  }
}

typedef struct {
  real N[3], inl, e[9];
} SR(Px);
static int SR(px)(const real *n, int kind, SR(Px) *px) {
  const real nn = SR(dot)(n, n);
  if (!SR(pos)(nn)) return 0;
  px->inl = (real)1 / SQRT(nn);
  for (int i = 0; i < 3; ++i) px->N[i] = n[i] * px->inl;
  real p[9];
  SR(poly)(px->N[0], px->N[1], px->N[2], p);
  const float *Kc = kind ? YC : HC;
  px->e[0] = (real)Kc[0];
  for (int k = 1; k < 9; ++k) px->e[k] = (real)Kc[CIDX[k]] * p[k];
  return 1;
}
/* nrm: [3][n]; sh: [9][C]; out: [C][n], written at owned pixels, and at nobody's (zeros) when fused */
void SR(forward)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *sh, uint32_t C, int kind, int fused, real *out) {
  for (size_t i = 0; i < n; ++i) {
    if (!owned(ids[i], n_tris)) {
      if (fused)
        for (uint32_t c = 0; c < C; ++c) out[c * n + i] = 0;
      continue;
    }
    const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]};
    SR(Px) px;
    const int lit = SR(px)(nk, kind, &px);
    for (uint32_t c = 0; c < C; ++c) {
      real v = 0;
      if (lit) {
        v = sh[c] * px.e[0];
        for (uint32_t k = 1; k < 9u; ++k) v = FMA(sh[k * C + c], px.e[k], v);
      }
      out[c * n + i] = v;
    }
  }
}
/* gout: [C][n]; gnrm: [3][n] or null; gsum, gabs: [9 C] doubles added into, count: [9 C] uint32 added into (all three or none);
 * terms: [9 C][n] of real or null — the pixel's own terms */
void SR(grad)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *sh, uint32_t C, int kind, const real *gout, int fused,
              real *gnrm, double *gsum, double *gabs, uint32_t *count, real *terms) {
  const float *Kc = kind ? YC : HC;
  for (size_t i = 0; i < n; ++i) {
    if (!owned(ids[i], n_tris)) {
      if (fused && gnrm) gnrm[i] = gnrm[n + i] = gnrm[2 * n + i] = 0;
      continue;
    }
    const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]};
    real gn[3] = {0, 0, 0};
    SR(Px) px;
    const int lit = SR(px)(nk, kind, &px);
    if (lit) {
      real gp[9];
      for (uint32_t k = 1; k < 9u; ++k) {
        real ge = gout[i] * sh[k * C];
        for (uint32_t c = 1; c < C; ++c) ge = FMA(gout[c * n + i], sh[k * C + c], ge);
        gp[k] = ge * (real)Kc[CIDX[k]];
      }
      const real x = px.N[0], y = px.N[1], z = px.N[2];
      const real gN[3] = {FMA((real)2 * x, gp[8], FMA(gp[7], z, FMA(gp[4], y, gp[3]))),
                          FMA((real)-2 * y, gp[8], FMA(gp[5], z, FMA(gp[4], x, gp[1]))),
                          FMA((real)6 * z, gp[6], FMA(gp[7], x, FMA(gp[5], y, gp[2])))};
      const real d = SR(dot)(gN, px.N);
      for (int c = 0; c < 3; ++c) gn[c] = (gN[c] - px.N[c] * d) * px.inl;
    }
    if (gnrm)
      for (int c = 0; c < 3; ++c) gnrm[c * n + i] = gn[c];
    for (uint32_t k = 0; k < 9u; ++k)
      for (uint32_t c = 0; c < C; ++c) {
        const real term = lit ? gout[c * n + i] * px.e[k] : 0;
        if (terms) terms[(size_t)(k * C + c) * n + i] = term;
        if (gsum && lit) gsum[k * C + c] += (double)term, gabs[k * C + c] += fabs((double)term), count[k * C + c] += 1u;
      }
  }
}
/* [n] bits: OWNED 1 | LIT 2, by this build's rule */
void SR(classify)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, uint8_t *cls) {
  for (size_t i = 0; i < n; ++i) {
    cls[i] = 0;
    if (!owned(ids[i], n_tris)) continue;
    const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]};
    SR(Px) px;
    cls[i] = 1 | (SR(px)(nk, 0, &px) ? 2 : 0);
  }
}
#endif
