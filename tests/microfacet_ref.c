/* The Cook-Torrance pass's test reference (tests/microfacetref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math; no flush to
 * zero).  It includes nothing of the library.  The rule include/srz.h states for srz_frameset_microfacet and the order of operations
 * it fixes for srz_frameset_microfacet_grad are written down ONCE, below, in terms of a type `real`; this file includes itself twice,
 * so that the one text exists as binary32 (mr32_*: the rule itself, what the GPU is held to bit for bit) and as binary64 (mr64_*: the
 * same operations carried out in double, what the binary32 build's error is measured against).  Per pixel of a visibility buffer
 * (owner id word) with its normal, position, base colour and material (roughness, metallic):
 *   forward: the colour planes;
 *   grad:    the gradient planes of the normal, the position, the base colour and the material, and per entry of the parameter frame
 *            the pixel's term (eye, amb: the pixel's own; a light's pos and intensity: its own) ACCUMULATED IN DOUBLE, with the sum
 *            of |term| and the count of contributing pixels, from which the tests derive their bound;
 *   classify: per pixel owned / lit / view / the clamps' branches / nv > 0, per light and pixel skipped / facing / specular / the
 *            inner clamps of nh and vh. */
#ifndef MR_BODY
#include <math.h>
#include <stddef.h>
#include <stdint.h>

static int owned(uint32_t id, uint32_t n_tris) { return ((id & 0x7fffffffu) - 1u) < n_tris; }

#define MR_BODY
#define real float
#define MR(name) mr32_##name
#define SQRT sqrtf
#define FMA fmaf
#include "microfacet_ref.c"
#undef real
#undef MR
#undef SQRT
#undef FMA
#define real double
#define MR(name) mr64_##name
#define SQRT sqrt
#define FMA fma
#include "microfacet_ref.c"

#else /* ---------------------------------------------------------------------------------------- the rule, once, in `real` */

#define INV_PI ((real)0x1.45f306p-2f)
#define RMIN ((real)0.0625f)

static real MR(dot)(const real *a, const real *b) { return FMA(a[0], b[0], FMA(a[1], b[1], a[2] * b[2])); }
static int MR(pos)(real x) { return x > 0 && x < (real)INFINITY; }
typedef struct {
  real N[3], P[3], Vd[3], inl, iv;
  int view;
  real base[3], r, m, rc, mc, al, a2, k, omk, om, F0[3], cdif[3], nv;
  int r_in, m_in;
} MR(Px);
typedef struct {
  real Lv[3], Ld[3], H[3], E[3], F[3], f[3], ir, att, ih, nl, nhr, nh, vhr, vh, t, tt, D, gl, gv, Vs, DV, x, x2, x4, x5;
  int spec;
} MR(Term);
static int MR(px)(const real *n, const real *P, const real *base, const real *mat, const real *par, MR(Px) *px) {
  const real nn = MR(dot)(n, n);
  if (!MR(pos)(nn)) return 0;
  px->inl = 1 / SQRT(nn);
  real V[3];
  for (int i = 0; i < 3; ++i) px->N[i] = n[i] * px->inl, px->P[i] = P[i], V[i] = par[i] - P[i];
  const real vv = MR(dot)(V, V);
  px->view = MR(pos)(vv);
  px->iv = px->view ? 1 / SQRT(vv) : 0;
  for (int i = 0; i < 3; ++i) px->Vd[i] = px->view ? V[i] * px->iv : 0;
  const real r = mat[0], m = mat[1];
  px->r = r, px->m = m;
  px->rc = r > RMIN ? (r < 1 ? r : 1) : RMIN, px->r_in = r > RMIN && r < 1;
  px->mc = m > 0 ? (m < 1 ? m : 1) : 0, px->m_in = m > 0 && m < 1;
  px->al = px->rc * px->rc, px->a2 = px->al * px->al, px->k = (real)0.5f * px->al, px->omk = 1 - px->k, px->om = 1 - px->mc;
  for (int c = 0; c < 3; ++c) {
    px->base[c] = base[c];
    px->F0[c] = FMA(px->mc, base[c] - (real)0.04f, (real)0.04f);
    px->cdif[c] = base[c] * px->om;
  }
  px->nv = px->view ? MR(dot)(px->N, px->Vd) : 0;
  return 1;
}
/* lp: the light's {pos[3], intensity[3]}.  0: the light adds nothing at this pixel (skipped, or nl not above 0: *skipped tells) */
static int MR(term)(const MR(Px) *px, const real *lp, MR(Term) *t, int *skipped) {
  for (int i = 0; i < 3; ++i) t->Lv[i] = lp[i] - px->P[i];
  const real r2 = MR(dot)(t->Lv, t->Lv);
  *skipped = !MR(pos)(r2);
  if (*skipped) return 0;
  t->ir = 1 / SQRT(r2), t->att = 1 / r2;
  real Hs[3];
  for (int i = 0; i < 3; ++i) t->Ld[i] = t->Lv[i] * t->ir, Hs[i] = t->Ld[i] + px->Vd[i], t->E[i] = lp[3 + i] * t->att;
  t->nl = MR(dot)(px->N, t->Ld);
  if (!(t->nl > 0)) return 0;
  const real h2 = MR(dot)(Hs, Hs);
  t->spec = px->view && h2 > 0 && px->nv > 0;
  if (t->spec) {
    t->ih = 1 / SQRT(h2);
    for (int i = 0; i < 3; ++i) t->H[i] = Hs[i] * t->ih;
    t->nhr = MR(dot)(px->N, t->H), t->nh = t->nhr > 0 ? (t->nhr < 1 ? t->nhr : 1) : 0;
    t->vhr = MR(dot)(px->Vd, t->H), t->vh = t->vhr > 0 ? (t->vhr < 1 ? t->vhr : 1) : 0;
    t->t = FMA(t->nh * t->nh, px->a2 - 1, 1), t->tt = t->t * t->t, t->D = (px->a2 * INV_PI) / t->tt;
    t->gl = FMA(t->nl, px->omk, px->k), t->gv = FMA(px->nv, px->omk, px->k), t->Vs = (real)0.25f / (t->gl * t->gv);
    t->DV = t->D * t->Vs;
    t->x = 1 - t->vh, t->x2 = t->x * t->x, t->x4 = t->x2 * t->x2, t->x5 = t->x4 * t->x;
    for (int c = 0; c < 3; ++c) {
      t->F[c] = FMA(1 - px->F0[c], t->x5, px->F0[c]);
      t->f[c] = FMA(px->cdif[c] * INV_PI, 1 - t->F[c], t->F[c] * t->DV);
    }
  } else
    for (int c = 0; c < 3; ++c) t->f[c] = px->cdif[c] * INV_PI;
  return 1;
}

/* planes: [3][n] of real, mat [2][n]; base may be null (ones); par: 6 + 6 n_lights reals; out: [3][n], written at owned pixels, and
 * at nobody's (zeros) when fused */
void MR(forward)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *pos, const real *base, const real *mat,
                 const real *par, int n_lights, int fused, real *out) {
  for (size_t i = 0; i < n; ++i) {
    if (!owned(ids[i], n_tris)) {
      if (fused) out[i] = out[n + i] = out[2 * n + i] = 0;
      continue;
    }
    const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]}, Pk[3] = {pos[i], pos[n + i], pos[2 * n + i]};
    const real bk[3] = {base ? base[i] : 1, base ? base[n + i] : 1, base ? base[2 * n + i] : 1}, mk[2] = {mat[i], mat[n + i]};
    real o[3] = {0, 0, 0};
    MR(Px) px;
    if (MR(px)(nk, Pk, bk, mk, par, &px)) {
      real acc[3] = {0, 0, 0};
      for (int l = 0; l < n_lights; ++l) {
        MR(Term) t;
        int skipped;
        if (!MR(term)(&px, par + 6 + 6 * l, &t, &skipped)) continue;
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + (t.f[c] * t.E[c]) * t.nl;
      }
      for (int c = 0; c < 3; ++c) o[c] = FMA(par[3 + c], bk[c], acc[c]);
    }
    for (int c = 0; c < 3; ++c) out[c * n + i] = o[c];
  }
}

/* gnrm, gpos, gbase: [3][n] or null, gmat: [2][n] or null; gsum, gabs: [K] doubles added into, count: [K] uint32 added into (all
 * three or none); terms: [K][n] of real or null — the pixel's own terms, for the tests that need one pixel's */
void MR(grad)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *pos, const real *base, const real *mat,
              const real *par, int n_lights, const real *gout, int fused, real *gnrm, real *gpos, real *gbase, real *gmat, double *gsum,
              double *gabs, uint32_t *count, real *terms) {
  const int K = 6 + 6 * n_lights;
  real *outs[3] = {gnrm, gpos, gbase};
  for (size_t i = 0; i < n; ++i) {
    if (!owned(ids[i], n_tris)) {
      if (fused) {
        for (int o = 0; o < 3; ++o)
          if (outs[o]) outs[o][i] = outs[o][n + i] = outs[o][2 * n + i] = 0;
        if (gmat) gmat[i] = gmat[n + i] = 0;
      }
      continue;
    }
    const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]}, Pk[3] = {pos[i], pos[n + i], pos[2 * n + i]};
    const real bk[3] = {base ? base[i] : 1, base ? base[n + i] : 1, base ? base[2 * n + i] : 1}, mk[2] = {mat[i], mat[n + i]};
    const real g[3] = {gout[i], gout[n + i], gout[2 * n + i]};
    const real *amb = par + 3;
    real gN[3] = {0, 0, 0}, gVd[3] = {0, 0, 0}, gP[3] = {0, 0, 0}, gb[3] = {0, 0, 0}, gn[3] = {0, 0, 0}, gm[2] = {0, 0};
    real g_a2 = 0, g_k = 0, g_nv = 0, g_om = 0, g_mc = 0;
    real term[6 + 6 * 8];
    uint8_t has[6 + 6 * 8];
    for (int k = 0; k < K; ++k) term[k] = 0, has[k] = 0;
    MR(Px) px;
    if (MR(px)(nk, Pk, bk, mk, par, &px)) {
      for (int k = 0; k < 6; ++k) has[k] = 1;
      for (int c = 0; c < 3; ++c) gb[c] = g[c] * amb[c], term[3 + c] = g[c] * bk[c];
      for (int l = 0; l < n_lights; ++l) {
        const real *lp = par + 6 + 6 * l, *I = lp + 3;
        MR(Term) t;
        int skipped;
        if (!MR(term)(&px, lp, &t, &skipped)) continue;
        real gf[3], ge[3], q[3], gcd[3], gLd[3], *tl = term + 6 + 6 * l;
        for (int c = 0; c < 3; ++c) {
          const real gq = g[c] * t.nl;
          gf[c] = gq * t.E[c], ge[c] = gq * t.f[c], q[c] = t.f[c] * t.E[c];
          tl[3 + c] = ge[c] * t.att;
        }
        real g_nl = MR(dot)(g, q);
        const real g_att = MR(dot)(ge, I);
        for (int c = 0; c < 3; ++c) gLd[c] = 0;
        if (t.spec) {
          real gF[3], gF0[3], omF0[3], bm[3];
          for (int c = 0; c < 3; ++c) {
            gcd[c] = (gf[c] * (1 - t.F[c])) * INV_PI;
            gF[c] = gf[c] * (t.DV - px.cdif[c] * INV_PI);
            gF0[c] = gF[c] * (1 - t.x5);
            omF0[c] = 1 - px.F0[c], bm[c] = px.base[c] - (real)0.04f;
            gb[c] = gb[c] + gF0[c] * px.mc;
          }
          g_mc = g_mc + MR(dot)(gF0, bm);
          const real gDV = MR(dot)(gf, t.F), gD = gDV * t.Vs, gVs = gDV * t.D;
          const real gx = MR(dot)(gF, omF0) * ((real)5.0f * t.x4);
          const real g_vhr = t.vhr > 0 && t.vhr < 1 ? -gx : 0;
          const real gw = -(gVs * t.Vs), ggl = gw / t.gl, ggv = gw / t.gv;
          g_nl = FMA(ggl, px.omk, g_nl);
          g_nv = FMA(ggv, px.omk, g_nv);
          g_k = g_k + FMA(ggl, 1 - t.nl, ggv * (1 - px.nv));
          const real g_t = -(((real)2.0f * (gD * t.D)) / t.t);
          g_a2 = g_a2 + FMA(g_t, t.nh * t.nh, gD * (INV_PI / t.tt));
          const real g_nhr = t.nhr > 0 && t.nhr < 1 ? g_t * (((real)2.0f * t.nh) * (px.a2 - 1)) : 0;
          real gH[3];
          for (int c = 0; c < 3; ++c) {
            gH[c] = FMA(g_nhr, px.N[c], g_vhr * px.Vd[c]);
            gN[c] = gN[c] + g_nhr * t.H[c];
            gVd[c] = gVd[c] + g_vhr * t.H[c];
          }
          const real d = MR(dot)(gH, t.H);
          for (int c = 0; c < 3; ++c) {
            const real gHs = (gH[c] - t.H[c] * d) * t.ih;
            gLd[c] = gHs, gVd[c] = gVd[c] + gHs;
          }
        } else
          for (int c = 0; c < 3; ++c) gcd[c] = gf[c] * INV_PI;
        g_om = g_om + MR(dot)(gcd, px.base);
        for (int c = 0; c < 3; ++c) {
          gb[c] = gb[c] + gcd[c] * px.om;
          gLd[c] = FMA(g_nl, px.N[c], gLd[c]);
          gN[c] = gN[c] + g_nl * t.Ld[c];
        }
        const real d = MR(dot)(gLd, t.Ld), w = 2 * (-((g_att * t.att) * t.att));
        for (int c = 0; c < 3; ++c) {
          tl[c] = FMA(t.Lv[c], w, (gLd[c] - t.Ld[c] * d) * t.ir);
          gP[c] = gP[c] - tl[c];
        }
        for (int k = 0; k < 6; ++k) has[6 + 6 * l + k] = 1;
      }
      if (px.view) {
        for (int c = 0; c < 3; ++c) gN[c] = FMA(g_nv, px.Vd[c], gN[c]), gVd[c] = FMA(g_nv, px.N[c], gVd[c]);
        const real d = MR(dot)(gVd, px.Vd);
        for (int c = 0; c < 3; ++c) {
          term[c] = (gVd[c] - px.Vd[c] * d) * px.iv;
          gP[c] = gP[c] - term[c];
        }
      }
      const real d = MR(dot)(gN, px.N);
      for (int c = 0; c < 3; ++c) gn[c] = (gN[c] - px.N[c] * d) * px.inl;
      const real g_al = FMA(g_a2, (real)2.0f * px.al, (real)0.5f * g_k);
      gm[0] = px.r_in ? g_al * ((real)2.0f * px.rc) : 0;
      gm[1] = px.m_in ? g_mc - g_om : 0;
    }
    for (int c = 0; c < 3; ++c) {
      if (gnrm) gnrm[c * n + i] = gn[c];
      if (gpos) gpos[c * n + i] = gP[c];
      if (gbase) gbase[c * n + i] = gb[c];
    }
    if (gmat) gmat[i] = gm[0], gmat[n + i] = gm[1];
    for (int k = 0; k < K; ++k) {
      if (terms) terms[(size_t)k * n + i] = term[k];
      if (gsum && has[k]) gsum[k] += (double)term[k], gabs[k] += fabs((double)term[k]), count[k] += 1u;
    }
  }
}

/* cls: [n] OWNED 1 | LIT 2 | VIEW 4 | NV_POS 8 (nv > 0);  mcls: [n] of the lit pixels R_LOW 1 (r <= RMIN, or a NaN) | R_HIGH 2 (r >= 1) |
 * M_LOW 4 (m <= 0, or a NaN) | M_HIGH 8 (m >= 1) | R_NAN 16 | M_NAN 32;  lcls: [n_lights][n] SKIPPED 1 | FACING 2 (nl > 0) | SPEC 4 |
 * NH_IN 8 (0 < nhr < 1) | VH_IN 16 (0 < vhr < 1) | REACHED 32 (the pixel is lit: the light was looked at) */
void MR(classify)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *pos, const real *mat, const real *par,
                  int n_lights, uint8_t *cls, uint8_t *mcls, uint8_t *lcls) {
  for (size_t i = 0; i < n; ++i) {
    cls[i] = mcls[i] = 0;
    for (int l = 0; l < n_lights; ++l) lcls[(size_t)l * n + i] = 0;
    if (!owned(ids[i], n_tris)) continue;
    cls[i] = 1;
    const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]}, Pk[3] = {pos[i], pos[n + i], pos[2 * n + i]};
    const real bk[3] = {1, 1, 1}, mk[2] = {mat[i], mat[n + i]};
    MR(Px) px;
    if (!MR(px)(nk, Pk, bk, mk, par, &px)) continue;
    cls[i] |= 2 | (px.view ? 4 : 0) | (px.nv > 0 ? 8 : 0);
    mcls[i] = (!(px.r > RMIN) ? 1 : 0) | (px.r >= 1 ? 2 : 0) | (!(px.m > 0) ? 4 : 0) | (px.m >= 1 ? 8 : 0) | (px.r != px.r ? 16 : 0) |
              (px.m != px.m ? 32 : 0);
    for (int l = 0; l < n_lights; ++l) {
      MR(Term) t;
      int skipped;
      uint8_t *o = lcls + (size_t)l * n + i;
      if (!MR(term)(&px, par + 6 + 6 * l, &t, &skipped)) *o = 32 | (skipped ? 1 : 0);
      else
        *o = 32 | 2 | (t.spec ? 4 : 0) | (t.spec && t.nhr > 0 && t.nhr < 1 ? 8 : 0) | (t.spec && t.vhr > 0 && t.vhr < 1 ? 16 : 0);
    }
  }
}
#undef INV_PI
#undef RMIN
#endif
