/* The cube prefilter's test reference (tests/prefilterref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math, once as
 * binary32 — `real` is float: the arithmetic the library is held to, bit for bit — and once with -DPFR_DOUBLE — `real` is double: the
 * same text as a binary64 function, for adjointness, the closed forms and the measured binary32 error).  It includes
 * tests/cube_ref.c unchanged for the faces' axes, and nothing of the library.  A cube [frames][6][n_src][n_src][n_ch] convolved into
 * a cube [frames][6][n_dst][n_dst][n_ch] by the rule include/srz.h states for srz_cube_prefilter, restated here:
 *   texel (f, y, x) of an N x N face:  s = (real)(2 x + 1) / (real)N - 1;  t likewise from y;  p = n_f + s su_f + t sv_f (the
 *     component along the normal is +-1, the one su names is s, negated where su is negative, the one sv names likewise t);
 *     r2 = fma(s, s, fma(t, t, 1));  inv = 1 / sqrt(r2);  d = p * inv;  jac = (inv * inv) * inv
 *   pair (o, i):  c = fma(do.x, di.x, fma(do.y, di.y, do.z * di.z));  c = c > 1 ? 1 : c;  skipped iff !(c > cmin)
 *   COSINE: w = c * jac_i.   GGX: r = roughness < 0.0625 ? 0.0625 : roughness;  a = r * r;  a2 = a * a;  nh2 = fma(0.5, c, 0.5);
 *     t = fma(nh2, a2 - 1, 1);  w = (c * jac_i) / (t * t)
 *   sums: a source row, columns ascending, num = fma(w, src, num), den = den + w from +0; a face's rows ascending by plain adds from
 *     +0; the six faces likewise;  dst = den > 0 ? num / den : 0
 *   backward: q = den_o > 0 ? gdst / den_o : 0;  gsrc[i] = the same three-level sum over the OUTPUT texels of fma(w(o, i), q, acc) */
#include "cube_ref.c"
#include <stdlib.h>

#ifdef PFR_DOUBLE
typedef double real;
#define R_FMA fma
#define R_SQRT sqrt
#else
typedef float real;
#define R_FMA fmaf
#define R_SQRT sqrtf
#endif
#define R(x) ((real)(x))

int pfr_real_bytes(void) { return (int)sizeof(real); }

typedef struct {
  real d[3], jac;
} PfTexel;

static void pf_texel(int N, int f, int y, int x, PfTexel *g) {
  const real s = (real)(2 * x + 1) / (real)N - R(1), t = (real)(2 * y + 1) / (real)N - R(1);
  real p[3];
  p[f / 2] = f % 2 ? R(-1) : R(1);
  p[SU_AXIS[f]] = SU_SIGN[f] < 0 ? -s : s;
  p[SV_AXIS[f]] = SV_SIGN[f] < 0 ? -t : t;
  const real r2 = R_FMA(s, s, R_FMA(t, t, R(1)));
  const real inv = R(1) / R_SQRT(r2);
  for (int k = 0; k < 3; ++k) g->d[k] = p[k] * inv;
  g->jac = (inv * inv) * inv;
}

/* the geometry of every texel of an N x N cube, [6 N N] */
void pfr_geometry(int N, real *d3, real *jac) {
  for (int f = 0; f < 6; ++f)
    for (int y = 0; y < N; ++y)
      for (int x = 0; x < N; ++x) {
        PfTexel g;
        pf_texel(N, f, y, x, &g);
        const size_t at = ((size_t)f * N + y) * N + x;
        d3[3 * at] = g.d[0], d3[3 * at + 1] = g.d[1], d3[3 * at + 2] = g.d[2], jac[at] = g.jac;
      }
}

/* 0: the pair is skipped */
static int pf_weight(const real dout[3], const real din[3], real jac_in, int kind, real a2m1, real cmin, real *w) {
  real c = R_FMA(dout[0], din[0], R_FMA(dout[1], din[1], dout[2] * din[2]));
  c = c > R(1) ? R(1) : c;
  if (!(c > cmin)) return 0;
  if (kind == 0) {
    *w = c * jac_in;
  } else {
    const real nh2 = R_FMA(R(0.5), c, R(0.5));
    const real t = R_FMA(nh2, a2m1, R(1));
    *w = (c * jac_in) / (t * t);
  }
  return 1;
}

static real pf_a2m1(float roughness) {
  const real r = (real)roughness < R(0.0625) ? R(0.0625) : (real)roughness;
  const real a = r * r;
  return a * a - R(1);
}

static PfTexel *pf_table(int N) {
  PfTexel *g = (PfTexel *)malloc((size_t)6 * N * N * sizeof(PfTexel));
  for (int f = 0; f < 6; ++f)
    for (int y = 0; y < N; ++y)
      for (int x = 0; x < N; ++x) pf_texel(N, f, y, x, &g[((size_t)f * N + y) * N + x]);
  return g;
}

/* src [frames][6][n_src][n_src][n_ch] -> dst [frames][6][n_dst][n_dst][n_ch], den [6][n_dst][n_dst], count [6][n_dst][n_dst]: the
 * pairs of an output texel that were not skipped (den and count may be null) */
void pfr_forward(const real *src, int n_src, int n_dst, uint32_t n_ch, uint32_t frames, int kind, float roughness, float cmin_, real *dst,
                 real *den_out, uint32_t *count) {
  PfTexel *gi = pf_table(n_src), *go = pf_table(n_dst);
  const real a2m1 = pf_a2m1(roughness), cmin = (real)cmin_;
  const size_t n_in = (size_t)6 * n_src * n_src, n_out = (size_t)6 * n_dst * n_dst;
  real *row = (real *)malloc(3 * (size_t)n_ch * sizeof(real)), *face = row + n_ch, *cube = face + n_ch;
  for (uint32_t fr = 0; fr < frames; ++fr)
    for (size_t o = 0; o < n_out; ++o) {
      real den_c = R(0);
      uint32_t cnt = 0;
      for (uint32_t ch = 0; ch < n_ch; ++ch) cube[ch] = R(0);
      for (int f = 0; f < 6; ++f) {
        real den_f = R(0);
        for (uint32_t ch = 0; ch < n_ch; ++ch) face[ch] = R(0);
        for (int y = 0; y < n_src; ++y) {
          real den_r = R(0);
          for (uint32_t ch = 0; ch < n_ch; ++ch) row[ch] = R(0);
          for (int x = 0; x < n_src; ++x) {
            const size_t i = ((size_t)f * n_src + y) * n_src + x;
            real w;
            if (!pf_weight(go[o].d, gi[i].d, gi[i].jac, kind, a2m1, cmin, &w)) continue;
            ++cnt;
            den_r = den_r + w;
            for (uint32_t ch = 0; ch < n_ch; ++ch) row[ch] = R_FMA(w, src[((size_t)fr * n_in + i) * n_ch + ch], row[ch]);
          }
          den_f = den_f + den_r;
          for (uint32_t ch = 0; ch < n_ch; ++ch) face[ch] = face[ch] + row[ch];
        }
        den_c = den_c + den_f;
        for (uint32_t ch = 0; ch < n_ch; ++ch) cube[ch] = cube[ch] + face[ch];
      }
      for (uint32_t ch = 0; ch < n_ch; ++ch) dst[((size_t)fr * n_out + o) * n_ch + ch] = den_c > R(0) ? cube[ch] / den_c : R(0);
      if (den_out && fr == 0) den_out[o] = den_c;
      if (count && fr == 0) count[o] = cnt;
    }
  free(row), free(gi), free(go);
}

/* gdst [frames][6][n_dst][n_dst][n_ch], den [6][n_dst][n_dst] as pfr_forward wrote it -> gsrc [frames][6][n_src][n_src][n_ch] */
void pfr_grad(const real *gdst, const real *den, int n_src, int n_dst, uint32_t n_ch, uint32_t frames, int kind, float roughness, float cmin_,
              real *gsrc) {
  PfTexel *gi = pf_table(n_src), *go = pf_table(n_dst);
  const real a2m1 = pf_a2m1(roughness), cmin = (real)cmin_;
  const size_t n_in = (size_t)6 * n_src * n_src, n_out = (size_t)6 * n_dst * n_dst;
  real *q = (real *)malloc((n_out + 3) * (size_t)n_ch * sizeof(real)), *row = q + n_out * n_ch, *face = row + n_ch, *cube = face + n_ch;
  for (uint32_t fr = 0; fr < frames; ++fr) {
    for (size_t o = 0; o < n_out; ++o)
      for (uint32_t ch = 0; ch < n_ch; ++ch) q[o * n_ch + ch] = den[o] > R(0) ? gdst[((size_t)fr * n_out + o) * n_ch + ch] / den[o] : R(0);
    for (size_t i = 0; i < n_in; ++i) {
      for (uint32_t ch = 0; ch < n_ch; ++ch) cube[ch] = R(0);
      for (int f = 0; f < 6; ++f) {
        for (uint32_t ch = 0; ch < n_ch; ++ch) face[ch] = R(0);
        for (int y = 0; y < n_dst; ++y) {
          for (uint32_t ch = 0; ch < n_ch; ++ch) row[ch] = R(0);
          for (int x = 0; x < n_dst; ++x) {
            const size_t o = ((size_t)f * n_dst + y) * n_dst + x;
            real w;
            if (!pf_weight(go[o].d, gi[i].d, gi[i].jac, kind, a2m1, cmin, &w)) continue;
            for (uint32_t ch = 0; ch < n_ch; ++ch) row[ch] = R_FMA(w, q[o * n_ch + ch], row[ch]);
          }
          for (uint32_t ch = 0; ch < n_ch; ++ch) face[ch] = face[ch] + row[ch];
        }
        for (uint32_t ch = 0; ch < n_ch; ++ch) cube[ch] = cube[ch] + face[ch];
      }
      for (uint32_t ch = 0; ch < n_ch; ++ch) gsrc[((size_t)fr * n_in + i) * n_ch + ch] = cube[ch];
    }
  }
  free(q), free(gi), free(go);
}
