/* The lighting pass's test reference (tests/lightref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math; no flush to zero).
 * It includes nothing of the library.  The rule include/srz.h states for srz_frameset_light and the order of operations it fixes for
 * srz_frameset_light_grad are written down ONCE, below, in terms of a type `real`; this file includes itself twice, so that the one
 * text exists as binary32 (lr32_*: the rule itself, what the GPU is held to bit for bit) and as binary64 (lr64_*: the same
 * operations carried out in double, what the binary32 build's error is measured against).  Per pixel of a visibility buffer (owner id
 * word) with its normal, position and albedo:
 *   forward: the colour planes;
 *   grad:    the gradient planes of the normal, the position and the albedo, and per entry of the parameter frame the pixel's term
 *            (eye, ka, ks: summed over the lights in light order first; a light's pos and intensity: its own) ACCUMULATED IN DOUBLE,
 *            with the sum of |term| and the count of contributing pixels, from which the tests derive their bound;
 *   classify: per pixel owned / lit / view, per light and pixel skipped / diffuse on / specular enabled / specular on. */
#ifndef LR_BODY
#include <math.h>
#include <stddef.h>
#include <stdint.h>

static int owned(uint32_t id, uint32_t n_tris) { return ((id & 0x7fffffffu) - 1u) < n_tris; }

#define LR_BODY
#define real float
#define LR(name) lr32_##name
#define SQRT sqrtf
#define FMA fmaf
#include "light_ref.c"
#undef real
#undef LR
#undef SQRT
#undef FMA
#define real double
#define LR(name) lr64_##name
#define SQRT sqrt
#define FMA fma
#include "light_ref.c"

#else /* ---------------------------------------------------------------------------------------- the rule, once, in `real` */

static real LR(dot)(const real *a, const real *b) { return FMA(a[0], b[0], FMA(a[1], b[1], a[2] * b[2])); }
static int LR(pos)(real x) { return x > 0 && x < (real)INFINITY; }
/* square-and-multiply in binary64, rounded once to `real` */
static real LR(powi)(real x, unsigned n) {
  double b = (double)x, r = 1.0;
  while (n) {
    if (n & 1u) r = r * b;
    b = b * b;
    n >>= 1;
  }
  return (real)r;
}
typedef struct {
  real N[3], P[3], Vd[3], inl, iv;
  int view;
} LR(Px);
typedef struct {
  real Lv[3], Ld[3], H[3], E[3], ir, att, ih, cdr, cd, csr, cs, sp;
  int spec;
} LR(Term);
static int LR(px)(const real *n, const real *P, const real *par, LR(Px) *px) {
  const real nn = LR(dot)(n, n);
  if (!LR(pos)(nn)) return 0;
  px->inl = 1 / SQRT(nn);
  real V[3];
  for (int i = 0; i < 3; ++i) px->N[i] = n[i] * px->inl, px->P[i] = P[i], V[i] = par[i] - P[i];
  const real vv = LR(dot)(V, V);
  px->view = LR(pos)(vv);
  px->iv = px->view ? 1 / SQRT(vv) : 0;
  for (int i = 0; i < 3; ++i) px->Vd[i] = px->view ? V[i] * px->iv : 0;
  return 1;
}
static int LR(term)(const LR(Px) *px, const real *lp, unsigned p, LR(Term) *t) {
  for (int i = 0; i < 3; ++i) t->Lv[i] = lp[i] - px->P[i];
  const real r2 = LR(dot)(t->Lv, t->Lv);
  if (!LR(pos)(r2)) return 0;
  t->ir = 1 / SQRT(r2), t->att = 1 / r2;
  real Hs[3];
  for (int i = 0; i < 3; ++i) t->Ld[i] = t->Lv[i] * t->ir, Hs[i] = t->Ld[i] + px->Vd[i], t->H[i] = 0, t->E[i] = lp[3 + i] * t->att;
  t->cdr = LR(dot)(px->N, t->Ld), t->cd = t->cdr > 0 ? t->cdr : 0;
  const real h2 = LR(dot)(Hs, Hs);
  t->spec = px->view && h2 > 0;
  t->ih = t->csr = t->cs = t->sp = 0;
  if (t->spec) {
    t->ih = 1 / SQRT(h2);
    for (int i = 0; i < 3; ++i) t->H[i] = Hs[i] * t->ih;
    t->csr = LR(dot)(px->N, t->H), t->cs = t->csr > 0 ? t->csr : 0;
    t->sp = LR(powi)(t->cs, p);
  }
  return 1;
}

/* planes: [3][n] of real; kd may be null (ones); par: 9 + 6 n_lights reals; out: [3][n], written at owned pixels, and at nobody's
 * (zeros) when fused */
void LR(forward)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *pos, const real *kd, const real *par,
                 int n_lights, unsigned p, int fused, real *out) {
  for (size_t i = 0; i < n; ++i) {
    if (!owned(ids[i], n_tris)) {
      if (fused) out[i] = out[n + i] = out[2 * n + i] = 0;
      continue;
    }
    const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]}, Pk[3] = {pos[i], pos[n + i], pos[2 * n + i]};
    const real kk[3] = {kd ? kd[i] : 1, kd ? kd[n + i] : 1, kd ? kd[2 * n + i] : 1};
    real acc[3] = {0, 0, 0};
    LR(Px) px;
    if (LR(px)(nk, Pk, par, &px))
      for (int l = 0; l < n_lights; ++l) {
        const real *lp = par + 9 + 6 * l;
        LR(Term) t;
        if (!LR(term)(&px, lp, p, &t)) continue;
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + (kk[c] * FMA(t.E[c], t.cd, par[3 + c] * lp[3 + c]) + (par[6 + c] * t.E[c]) * t.sp);
      }
    for (int c = 0; c < 3; ++c) out[c * n + i] = acc[c];
  }
}

/* gnrm, gpos, gkd: [3][n] or null; gsum, gabs: [K] doubles added into, count: [K] uint32 added into (all three or none); terms: [K][n]
 * of real or null — the pixel's own terms, for the tests that need one pixel's */
void LR(grad)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *pos, const real *kd, const real *par, int n_lights,
              unsigned p, const real *gout, int fused, real *gnrm, real *gpos, real *gkd, double *gsum, double *gabs, uint32_t *count,
              real *terms) {
  const int K = 9 + 6 * n_lights;
  real *outs[3] = {gnrm, gpos, gkd};
  for (size_t i = 0; i < n; ++i) {
    if (!owned(ids[i], n_tris)) {
      if (fused)
        for (int o = 0; o < 3; ++o)
          if (outs[o]) outs[o][i] = outs[o][n + i] = outs[o][2 * n + i] = 0;
      continue;
    }
    const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]}, Pk[3] = {pos[i], pos[n + i], pos[2 * n + i]};
    const real kk[3] = {kd ? kd[i] : 1, kd ? kd[n + i] : 1, kd ? kd[2 * n + i] : 1};
    const real g[3] = {gout[i], gout[n + i], gout[2 * n + i]};
    const real *ka = par + 3, *ks = par + 6;
    real gN[3] = {0, 0, 0}, gVd[3] = {0, 0, 0}, gP[3] = {0, 0, 0}, gk_d[3] = {0, 0, 0}, tka[3] = {0, 0, 0}, tks[3] = {0, 0, 0}, gn[3] = {0, 0, 0};
    real term[9 + 6 * 8];
    uint8_t has[9 + 6 * 8];
    for (int k = 0; k < K; ++k) term[k] = 0, has[k] = 0;
    LR(Px) px;
    if (LR(px)(nk, Pk, par, &px)) {
      for (int k = 0; k < 9; ++k) has[k] = 1;
      for (int l = 0; l < n_lights; ++l) {
        const real *lp = par + 9 + 6 * l, *I = lp + 3;
        LR(Term) t;
        if (!LR(term)(&px, lp, p, &t)) continue;
        real gk[3], gs[3], ge[3], gLd[3], *tl = term + 9 + 6 * l;
        for (int c = 0; c < 3; ++c) {
          gk[c] = g[c] * kk[c], gs[c] = g[c] * ks[c];
          gk_d[c] = gk_d[c] + g[c] * FMA(t.E[c], t.cd, ka[c] * I[c]);
          tka[c] = tka[c] + gk[c] * I[c];
          tks[c] = tks[c] + (g[c] * t.E[c]) * t.sp;
          tl[3 + c] = g[c] * (kk[c] * FMA(t.att, t.cd, ka[c]) + (ks[c] * t.att) * t.sp);
          ge[c] = g[c] * FMA(kk[c], t.cd, ks[c] * t.sp);
        }
        const real g_cd = t.cdr > 0 ? LR(dot)(gk, t.E) : 0, g_sp = LR(dot)(gs, t.E), g_att = LR(dot)(ge, I);
        for (int c = 0; c < 3; ++c) gLd[c] = g_cd * px.N[c], gN[c] = gN[c] + g_cd * t.Ld[c];
        if (t.spec && t.csr > 0) {
          const real g_cs = g_sp * ((real)p * LR(powi)(t.cs, p - 1u));
          real gH[3];
          for (int c = 0; c < 3; ++c) gH[c] = g_cs * px.N[c], gN[c] = gN[c] + g_cs * t.H[c];
          const real d = LR(dot)(gH, t.H);
          for (int c = 0; c < 3; ++c) {
            const real gHs = (gH[c] - t.H[c] * d) * t.ih;
            gLd[c] = gLd[c] + gHs, gVd[c] = gVd[c] + gHs;
          }
        }
        const real d = LR(dot)(gLd, t.Ld), w = 2 * (-((g_att * t.att) * t.att));
        for (int c = 0; c < 3; ++c) {
          tl[c] = FMA(t.Lv[c], w, (gLd[c] - t.Ld[c] * d) * t.ir);
          gP[c] = gP[c] - tl[c];
        }
        for (int k = 0; k < 6; ++k) has[9 + 6 * l + k] = 1;
      }
      if (px.view) {
        const real d = LR(dot)(gVd, px.Vd);
        for (int c = 0; c < 3; ++c) {
          term[c] = (gVd[c] - px.Vd[c] * d) * px.iv;
          gP[c] = gP[c] - term[c];
        }
      }
      const real d = LR(dot)(gN, px.N);
      for (int c = 0; c < 3; ++c) gn[c] = (gN[c] - px.N[c] * d) * px.inl, term[3 + c] = tka[c], term[6 + c] = tks[c];
    }
    for (int c = 0; c < 3; ++c) {
      if (gnrm) gnrm[c * n + i] = gn[c];
      if (gpos) gpos[c * n + i] = gP[c];
      if (gkd) gkd[c * n + i] = gk_d[c];
    }
    for (int k = 0; k < K; ++k) {
      if (terms) terms[(size_t)k * n + i] = term[k];
      if (gsum && has[k]) gsum[k] += (double)term[k], gabs[k] += fabs((double)term[k]), count[k] += 1u;
    }
  }
}

/* cls: [n] OWNED 1 | LIT 2 | VIEW 4;  lcls: [n_lights][n] SKIPPED 1 | DIFFUSE ON 2 (cdr > 0) | SPECULAR ENABLED 4 (view && h2 > 0) |
 * SPECULAR ON 8 (enabled and csr > 0) | REACHED 16 (the pixel is lit: the light was looked at) */
void LR(classify)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *pos, const real *par, int n_lights, unsigned p,
                  uint8_t *cls, uint8_t *lcls) {
  for (size_t i = 0; i < n; ++i) {
    cls[i] = 0;
    for (int l = 0; l < n_lights; ++l) lcls[(size_t)l * n + i] = 0;
    if (!owned(ids[i], n_tris)) continue;
    cls[i] = 1;
    const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]}, Pk[3] = {pos[i], pos[n + i], pos[2 * n + i]};
    LR(Px) px;
    if (!LR(px)(nk, Pk, par, &px)) continue;
    cls[i] |= 2 | (px.view ? 4 : 0);
    for (int l = 0; l < n_lights; ++l) {
      LR(Term) t;
      uint8_t *o = lcls + (size_t)l * n + i;
      if (!LR(term)(&px, par + 9 + 6 * l, p, &t)) *o = 16 | 1;
      else *o = 16 | (t.cdr > 0 ? 2 : 0) | (t.spec ? 4 : 0) | (t.spec && t.csr > 0 ? 8 : 0);
    }
  }
}
#endif
