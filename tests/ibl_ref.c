/* The image-based-lighting passes' test reference (tests/iblref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math; no flush to
 * zero).  It includes nothing of the library.  The rules include/srz.h states for srz_frameset_reflect / _reflect_grad,
 * srz_brdf_table and srz_frameset_ibl / _ibl_grad are written down ONCE, below, in terms of a type `real`; this file includes itself
 * twice, so that the one text exists as binary32 (ib32_*: the rules themselves, what the GPU is held to bit for bit) and as binary64
 * (ib64_*: the same operations carried out in double, what the binary32 build's error is measured against).
 *   reflect / reflect_grad: per pixel of a visibility buffer (owner id word) with its normal and position, and the eye;
 *   table:                  the split-sum table [n][n][2] from n and m alone;
 *   ibl / ibl_grad:         per pixel with base colour, material, nv, irradiance and specular planes and the table; the table's
 *                           gradient ACCUMULATED IN DOUBLE with the sum of |term| and the count of contributing pixels per word, from
 *                           which the tests derive their bound;
 *   classify:               the branch every pixel took. */
#ifndef IB_BODY
#include <math.h>
#include <stddef.h>
#include <stdint.h>

static int owned(uint32_t id, uint32_t n_tris) { return ((id & 0x7fffffffu) - 1u) < n_tris; }

#define IB_BODY
#define real float
#define IB(name) ib32_##name
#define SQRT sqrtf
#define FMA fmaf
#define FLOOR floorf
#include "ibl_ref.c"
#undef real
#undef IB
#undef SQRT
#undef FMA
#undef FLOOR
#define real double
#define IB(name) ib64_##name
#define SQRT sqrt
#define FMA fma
#define FLOOR floor
#include "ibl_ref.c"

#else /* ---------------------------------------------------------------------------------------- the rules, once, in `real` */

#define INV_PI ((real)0x1.45f306p-2f)
#define RMIN ((real)0.0625f)
#define RSPAN ((real)0.9375f)

static real IB(dot)(const real *a, const real *b) { return FMA(a[0], b[0], FMA(a[1], b[1], a[2] * b[2])); }
static int IB(pos)(real x) { return x > 0 && x < (real)INFINITY; }

/* ------------------------------------------------------------------------------------------------------------ reflect */
typedef struct {
  real N[3], Vd[3], inl, iv, nv, t2;
} IB(Rf);
/* 0: not lit, or no view: four zeros, no gradient */
static int IB(rf)(const real *n, const real *P, const real *eye, IB(Rf) *r) {
  const real nn = IB(dot)(n, n);
  if (!IB(pos)(nn)) return 0;
  r->inl = 1 / SQRT(nn);
  real V[3];
  for (int i = 0; i < 3; ++i) r->N[i] = n[i] * r->inl, V[i] = eye[i] - P[i];
  const real vv = IB(dot)(V, V);
  if (!IB(pos)(vv)) return 0;
  r->iv = 1 / SQRT(vv);
  for (int i = 0; i < 3; ++i) r->Vd[i] = V[i] * r->iv;
  r->nv = IB(dot)(r->N, r->Vd), r->t2 = 2 * r->nv;
  return 1;
}
/* nrm, pos: [3][n]; eye: 3 reals; out: [4][n], written at owned pixels, and at nobody's (zeros) when fused */
void IB(reflect)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *pos, const real *eye, int fused, real *out) {
  for (size_t i = 0; i < n; ++i) {
    if (!owned(ids[i], n_tris)) {
      if (fused) out[i] = out[n + i] = out[2 * n + i] = out[3 * n + i] = 0;
      continue;
    }
    const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]}, Pk[3] = {pos[i], pos[n + i], pos[2 * n + i]};
    real o[4] = {0, 0, 0, 0};
    IB(Rf) r;
    if (IB(rf)(nk, Pk, eye, &r)) {
      for (int c = 0; c < 3; ++c) o[c] = FMA(r.t2, r.N[c], -r.Vd[c]);
      o[3] = r.nv;
    }
    for (int c = 0; c < 4; ++c) out[c * n + i] = o[c];
  }
}
/* gout: [4][n]; gnrm, gpos: [3][n] or null */
void IB(reflect_grad)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *pos, const real *eye, const real *gout,
                      int fused, real *gnrm, real *gpos) {
  for (size_t i = 0; i < n; ++i) {
    if (!owned(ids[i], n_tris)) {
      if (fused) {
        if (gnrm) gnrm[i] = gnrm[n + i] = gnrm[2 * n + i] = 0;
        if (gpos) gpos[i] = gpos[n + i] = gpos[2 * n + i] = 0;
      }
      continue;
    }
    const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]}, Pk[3] = {pos[i], pos[n + i], pos[2 * n + i]};
    const real gR[3] = {gout[i], gout[n + i], gout[2 * n + i]};
    real gn[3] = {0, 0, 0}, gP[3] = {0, 0, 0};
    IB(Rf) r;
    if (IB(rf)(nk, Pk, eye, &r)) {
      const real g_nv = FMA((real)2.0f, IB(dot)(gR, r.N), gout[3 * n + i]);
      real gN[3], gVd[3];
      for (int c = 0; c < 3; ++c) gN[c] = FMA(g_nv, r.Vd[c], gR[c] * r.t2), gVd[c] = FMA(g_nv, r.N[c], -gR[c]);
      const real dv = IB(dot)(gVd, r.Vd), dn = IB(dot)(gN, r.N);
      for (int c = 0; c < 3; ++c) {
        gP[c] = -((gVd[c] - r.Vd[c] * dv) * r.iv);
        gn[c] = (gN[c] - r.N[c] * dn) * r.inl;
      }
    }
    for (int c = 0; c < 3; ++c) {
      if (gnrm) gnrm[c * n + i] = gn[c];
      if (gpos) gpos[c * n + i] = gP[c];
    }
  }
}
/* cls: [n] OWNED 1 | LIT 2 | VIEW 4 | NV_POS 8 (nv > 0) */
void IB(reflect_classify)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *pos, const real *eye, uint8_t *cls) {
  for (size_t i = 0; i < n; ++i) {
    cls[i] = 0;
    if (!owned(ids[i], n_tris)) continue;
    cls[i] = 1;
    const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]}, Pk[3] = {pos[i], pos[n + i], pos[2 * n + i]};
    if (!IB(pos)(IB(dot)(nk, nk))) continue;
    cls[i] |= 2;
    IB(Rf) r;
    if (IB(rf)(nk, Pk, eye, &r)) cls[i] |= 4 | (r.nv > 0 ? 8 : 0);
  }
}

/* ------------------------------------------------------------------------------------------------------------ the table */
/* one entry: row i (nv), column j (roughness) of an n x n table with m rings of 2 m samples; hx_sum (may be null): the A sums of the
 * two signs of hx apart, [2] */
static void IB(entry)(int n, int m, int i, int j, real *A, real *B, real *hx_sum) {
  const real nv = (real)i / (real)(n - 1), rc = FMA(RSPAN, (real)j / (real)(n - 1), RMIN);
  const real al = rc * rc, a2 = al * al, k = (real)0.5f * al, omk = 1 - k;
  const real vx = SQRT(FMA(-nv, nv, 1)), gv = FMA(nv, omk, k), fm = (real)m;
  real sa = 0, sb = 0, sg[2] = {0, 0};
  for (int a = 0; a < m; ++a) {
    const real u = ((real)a + (real)0.5f) / fm, q = 1 - u, xi = FMA(-q, q, 1), wr = ((real)2.0f * q) / fm;
    const real s = (a2 * xi) / FMA(-xi, 1 - a2, 1), r = SQRT(s), hz = SQRT(1 - s);
    real ra = 0, rb = 0, rs[2] = {0, 0};
    for (int b = 0; b < m; ++b) {
      const real t = ((real)b + (real)0.5f) / fm, tt = t * t, den = 1 + tt, c = (1 - tt) / den, wa = ((real)2.0f / den) / fm;
      for (int sgn = 0; sgn < 2; ++sgn) {
        const real hx = sgn ? -(r * c) : r * c;
        const real vh = FMA(vx, hx, nv * hz), nl = FMA((real)2.0f * vh, hz, -nv);
        const int take = vh > 0 && nl > 0;
        const real gl = FMA(nl, omk, k), f = (nl * vh) / (hz * (gl * gv));
        const real x = 1 - (vh < 1 ? vh : 1), x2 = x * x, x4 = x2 * x2, x5 = x4 * x;
        const real ta = take ? (f * (1 - x5)) * wa : 0, tb = take ? (f * x5) * wa : 0;
        ra = ra + ta, rb = rb + tb, rs[sgn] = rs[sgn] + ta;
      }
    }
    sa = FMA(ra, wr, sa), sb = FMA(rb, wr, sb);
    sg[0] = FMA(rs[0], wr, sg[0]), sg[1] = FMA(rs[1], wr, sg[1]);
  }
  *A = sa * INV_PI, *B = sb * INV_PI;
  if (hx_sum) hx_sum[0] = sg[0] * INV_PI, hx_sum[1] = sg[1] * INV_PI;
}
/* tab: [n][n][2]; hx_sum: [n][n][2] or null */
void IB(table)(int n, int m, real *tab, real *hx_sum) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      IB(entry)(n, m, i, j, tab + 2 * (i * n + j), tab + 2 * (i * n + j) + 1, hx_sum ? hx_sum + 2 * (i * n + j) : NULL);
}

/* ------------------------------------------------------------------------------------------------------------ ibl */
typedef struct {
  real base[3], F0[3], cdif[3], irr[3], spec[3], sc[3];
  real rc, mc, om, nvc, tx, ty, A, B, dAx, dBx, dAy, dBy, sx, sy;
  int r_in, m_in, nv_in, x0, y0;
} IB(Px);
static void IB(px)(const real *base, real r, real m, real nv, const real *irr, const real *spec, const real *tab, int n, IB(Px) *p) {
  p->rc = r > RMIN ? (r < 1 ? r : 1) : RMIN, p->r_in = r > RMIN && r < 1;
  p->mc = m > 0 ? (m < 1 ? m : 1) : 0, p->m_in = m > 0 && m < 1;
  p->nvc = nv > 0 ? (nv < 1 ? nv : 1) : 0, p->nv_in = nv > 0 && nv < 1;
  p->sx = (real)(n - 1), p->sy = (real)(n - 1) / RSPAN;
  const real x = p->nvc * p->sx, y = (p->rc - RMIN) * p->sy;
  const int fx = (int)FLOOR(x), fy = (int)FLOOR(y);
  p->x0 = fx < n - 2 ? fx : n - 2, p->y0 = fy < n - 2 ? fy : n - 2;
  p->tx = x - (real)p->x0, p->ty = y - (real)p->y0;
  const real *t00 = tab + 2 * (p->x0 * n + p->y0), *t01 = t00 + 2, *t10 = t00 + 2 * n, *t11 = t10 + 2;
  real v[2], dx[2], dy[2];
  for (int e = 0; e < 2; ++e) {
    const real d0 = t01[e] - t00[e], d1 = t11[e] - t10[e];
    const real top = FMA(p->ty, d0, t00[e]), bot = FMA(p->ty, d1, t10[e]);
    dx[e] = bot - top, v[e] = FMA(p->tx, dx[e], top), dy[e] = FMA(p->tx, d1 - d0, d0);
  }
  p->A = v[0], p->B = v[1], p->dAx = dx[0], p->dBx = dx[1], p->dAy = dy[0], p->dBy = dy[1];
  p->om = 1 - p->mc;
  for (int c = 0; c < 3; ++c) {
    p->base[c] = base[c], p->irr[c] = irr[c], p->spec[c] = spec[c];
    p->F0[c] = FMA(p->mc, base[c] - (real)0.04f, (real)0.04f);
    p->cdif[c] = base[c] * p->om;
    p->sc[c] = FMA(p->F0[c], p->A, p->B);
  }
}
#define IB_LOAD                                                                                                                     \
  const real bk[3] = {base ? base[i] : 1, base ? base[n + i] : 1, base ? base[2 * n + i] : 1};                                      \
  const real ik[3] = {irr[i], irr[n + i], irr[2 * n + i]}, sk[3] = {spec[i], spec[n + i], spec[2 * n + i]};                         \
  IB(Px) p;                                                                                                                         \
  IB(px)(bk, mat[i], mat[n + i], nv[i], ik, sk, tab, tn, &p)
/* base [3][n] or null (ones), mat [2][n], nv [n], irr, spec [3][n], tab [tn][tn][2]; out [3][n] */
void IB(ibl)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *base, const real *mat, const real *nv, const real *irr,
             const real *spec, const real *tab, int tn, int fused, real *out) {
  for (size_t i = 0; i < n; ++i) {
    if (!owned(ids[i], n_tris)) {
      if (fused) out[i] = out[n + i] = out[2 * n + i] = 0;
      continue;
    }
    IB_LOAD;
    for (int c = 0; c < 3; ++c) out[c * n + i] = FMA(p.cdif[c], p.irr[c], p.spec[c] * p.sc[c]);
  }
}
/* gout [3][n]; gbase, girr, gspec [3][n], gmat [2][n], gnv [n]: each or null; gsum, gabs: [tn][tn][2] doubles added into, count: the
 * same shape uint32 added into (all three or none); terms: [8][n] of real or null — the pixel's own four A terms, then its four B
 * terms, in the order (x0, y0), (x0, y0 + 1), (x0 + 1, y0), (x0 + 1, y0 + 1); cell: [2][n] int32 or null — x0, y0 */
void IB(ibl_grad)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *base, const real *mat, const real *nv, const real *irr,
                  const real *spec, const real *tab, int tn, const real *gout, int fused, real *gbase, real *gmat, real *gnv, real *girr,
                  real *gspec, double *gsum, double *gabs, uint32_t *count, real *terms, int32_t *cell) {
  real *three[3] = {gbase, girr, gspec};
  for (size_t i = 0; i < n; ++i) {
    if (!owned(ids[i], n_tris)) {
      if (fused) {
        for (int o = 0; o < 3; ++o)
          if (three[o]) three[o][i] = three[o][n + i] = three[o][2 * n + i] = 0;
        if (gmat) gmat[i] = gmat[n + i] = 0;
        if (gnv) gnv[i] = 0;
      }
      continue;
    }
    IB_LOAD;
    const real g[3] = {gout[i], gout[n + i], gout[2 * n + i]};
    real gcd[3], gs[3], gF0[3], bm[3], gb[3], gi[3], gsp[3];
    for (int c = 0; c < 3; ++c) {
      gcd[c] = g[c] * p.irr[c], gi[c] = g[c] * p.cdif[c];
      gs[c] = g[c] * p.spec[c], gsp[c] = g[c] * p.sc[c];
      gF0[c] = gs[c] * p.A, bm[c] = p.base[c] - (real)0.04f;
      gb[c] = FMA(gF0[c], p.mc, gcd[c] * p.om);
    }
    const real gA = IB(dot)(gs, p.F0), gB = IB(dot)(g, p.spec);
    const real g_mc = IB(dot)(gF0, bm), g_om = IB(dot)(gcd, p.base);
    const real g_x = FMA(gA, p.dAx, gB * p.dBx), g_y = FMA(gA, p.dAy, gB * p.dBy);
    const real gm0 = p.r_in ? g_y * p.sy : 0, gm1 = p.m_in ? g_mc - g_om : 0, gn = p.nv_in ? g_x * p.sx : 0;
    for (int c = 0; c < 3; ++c) {
      if (gbase) gbase[c * n + i] = gb[c];
      if (girr) girr[c * n + i] = gi[c];
      if (gspec) gspec[c * n + i] = gsp[c];
    }
    if (gmat) gmat[i] = gm0, gmat[n + i] = gm1;
    if (gnv) gnv[i] = gn;
    const real ux = 1 - p.tx, uy = 1 - p.ty;
    const real w[4] = {ux * uy, ux * p.ty, p.tx * uy, p.tx * p.ty};
    const int at[4] = {p.x0 * tn + p.y0, p.x0 * tn + p.y0 + 1, (p.x0 + 1) * tn + p.y0, (p.x0 + 1) * tn + p.y0 + 1};
    for (int q = 0; q < 4; ++q) {
      const real term[2] = {w[q] * gA, w[q] * gB};
      for (int e = 0; e < 2; ++e) {
        if (terms) terms[(size_t)(4 * e + q) * n + i] = term[e];
        if (gsum) gsum[2 * at[q] + e] += (double)term[e], gabs[2 * at[q] + e] += fabs((double)term[e]), count[2 * at[q] + e] += 1u;
      }
    }
    if (cell) cell[i] = p.x0, cell[n + i] = p.y0;
  }
}
/* cls: [n] OWNED 1 | R_LOW 2 (r <= RMIN, or a NaN) | R_HIGH 4 (r >= 1) | M_LOW 8 | M_HIGH 16 | NV_LOW 32 (nv <= 0, or a NaN) |
 * NV_HIGH 64 (nv >= 1) | LAST_CELL 128 (x0 or y0 is n - 2 by the min, the coordinate at or beyond n - 1) */
void IB(ibl_classify)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *mat, const real *nv, int tn, uint8_t *cls) {
  for (size_t i = 0; i < n; ++i) {
    cls[i] = 0;
    if (!owned(ids[i], n_tris)) continue;
    const real r = mat[i], m = mat[n + i], v = nv[i];
    const real rc = r > RMIN ? (r < 1 ? r : 1) : RMIN, nvc = v > 0 ? (v < 1 ? v : 1) : 0;
    const real x = nvc * (real)(tn - 1), y = (rc - RMIN) * ((real)(tn - 1) / RSPAN);
    cls[i] = 1 | (!(r > RMIN) ? 2 : 0) | (r >= 1 ? 4 : 0) | (!(m > 0) ? 8 : 0) | (m >= 1 ? 16 : 0) | (!(v > 0) ? 32 : 0) | (v >= 1 ? 64 : 0) |
             ((int)FLOOR(x) > tn - 2 || (int)FLOOR(y) > tn - 2 ? 128 : 0);
  }
}
#undef IB_LOAD
#undef INV_PI
#undef RMIN
#undef RSPAN
#endif
