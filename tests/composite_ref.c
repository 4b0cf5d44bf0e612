/* The depth-layer composite's test reference (tests/compositeref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math, once as
 * binary32 — `real` is float: the arithmetic the library is held to, bit for bit — and once with -DCMR_DOUBLE — `real` is double: the
 * same text as a binary64 function, for central differences, torch's float64 autograd and the measured binary32 error).  Nothing of
 * the library is involved.  The rule include/srz.h states for srz_frameset_composite / _composite_grad, restated here for ONE frame
 * of P pixels, every buffer planar [plane][P]:
 *   layer k covers pixel p iff (id & 0x7fffffff) - 1 < n_tris in uint32 arithmetic (0 and the bare class bit wrap: nobody)
 *   forward: T = 1, acc_c = +0; for the covering layers in order: w = a * T; acc_c = acc_c + col_c * w; T = T * (1 - a);
 *     with bg: acc_c = acc_c + bg_c * T
 *   backward: T_k, w_k recomputed; gbg_c = g_c * T_n; S = gT, with bg S = fma(g_c, bg_c, S) in channel order; for the covering
 *     layers from last to first: d = fma(g_c, col_c, d) from +0 in channel order; gcol_c = g_c * w_k; galpha = T_k * (d - S);
 *     S = fma(a, d, (1 - a) * S); +0 in gcol and galpha where the layer does not cover the pixel
 * A layer's alpha is its plane's word, or, with a null plane, the scalar opacity. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef CMR_DOUBLE
typedef double real;
#define R_FMA fma
#else
typedef float real;
#define R_FMA fmaf
#endif
#define R(x) ((real)(x))
#define CMR_MAX 8

int cmr_real_bytes(void) { return (int)sizeof(real); }

/* cov[p] = 1 where the id word names an owner among n_tris triangles */
void cmr_cover(const uint32_t *ids, size_t P, uint32_t n_tris, uint8_t *cov) {
  for (size_t p = 0; p < P; ++p) cov[p] = (uint32_t)((ids[p] & 0x7fffffffu) - 1u) < n_tris;
}

/* cov[k]: P bytes; col[k]: [C][P]; alpha[k]: [P] or NULL (opacity[k]); bg: [C][P] or NULL; out: [C][P]; through: [P] or NULL */
void cmr_forward(int L, int C, size_t P, const uint8_t *const *cov, const real *const *col, const real *const *alpha, const real *opacity,
                 const real *bg, real *out, real *through) {
  for (size_t p = 0; p < P; ++p) {
    real T = R(1), w[CMR_MAX];
    for (int k = 0; k < L; ++k) {
      if (!cov[k][p]) continue;
      const real a = alpha[k] ? alpha[k][p] : opacity[k];
      w[k] = a * T;
      T = T * (R(1) - a);
    }
    for (int c = 0; c < C; ++c) {
      real acc = R(0);
      for (int k = 0; k < L; ++k)
        if (cov[k][p]) acc = acc + col[k][(size_t)c * P + p] * w[k];
      if (bg) acc = acc + bg[(size_t)c * P + p] * T;
      out[(size_t)c * P + p] = acc;
    }
    if (through) through[p] = T;
  }
}

/* g: [C][P]; gT: [P] or NULL (0); gcol[k]: [C][P] or NULL; galpha[k]: [P] or NULL; gbg: [C][P] or NULL — every asked-for word written */
void cmr_grad(int L, int C, size_t P, const uint8_t *const *cov, const real *const *col, const real *const *alpha, const real *opacity,
              const real *bg, const real *g, const real *gT, real *const *gcol, real *const *galpha, real *gbg) {
  for (size_t p = 0; p < P; ++p) {
    real T = R(1), a[CMR_MAX], Tk[CMR_MAX];
    for (int k = 0; k < L; ++k) {
      if (!cov[k][p]) continue;
      a[k] = alpha[k] ? alpha[k][p] : opacity[k];
      Tk[k] = T;
      T = T * (R(1) - a[k]);
    }
    real S = gT ? gT[p] : R(0);
    for (int c = 0; c < C; ++c) {
      const real gc = g[(size_t)c * P + p];
      if (bg) S = R_FMA(gc, bg[(size_t)c * P + p], S);
      if (gbg) gbg[(size_t)c * P + p] = gc * T;
    }
    for (int k = L - 1; k >= 0; --k) {
      if (!cov[k][p]) {
        if (galpha[k]) galpha[k][p] = R(0);
        if (gcol[k])
          for (int c = 0; c < C; ++c) gcol[k][(size_t)c * P + p] = R(0);
        continue;
      }
      const real w = a[k] * Tk[k];
      real d = R(0);
      for (int c = 0; c < C; ++c) {
        const real gc = g[(size_t)c * P + p];
        d = R_FMA(gc, col[k][(size_t)c * P + p], d);
        if (gcol[k]) gcol[k][(size_t)c * P + p] = gc * w;
      }
      if (galpha[k]) galpha[k][p] = Tk[k] * (d - S);
      S = R_FMA(a[k], d, (R(1) - a[k]) * S);
    }
  }
}
