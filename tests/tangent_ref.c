/* The test reference of the mesh tangents and of the normal-mapping pass (tests/tangentref.py builds it with gcc -O2
 * -ffp-contract=off -fno-fast-math; no flush to zero).  It includes nothing of the library.  The rules include/srz.h states for
 * srz_mesh_tangents / _grad and srz_frameset_normal_map / _grad, with the orders of operations it fixes, are written down ONCE, below,
 * in terms of a type `real`; this file includes itself twice, so that the one text exists as binary32 (tr32_*: the rules themselves,
 * what the GPU is held to bit for bit) and as binary64 (tr64_*: the same operations carried out in double).
 *   tangents, tangents_grad:  one position set [V][3] and one uv set [V][2] over a face list and its corner lists -> [V][4]; [V][3]
 *   tangents_classify:        per vertex NAMED 1 | NORMALISED 2 | w negative 4
 *   nm_forward, nm_grad:      per pixel of a visibility buffer (owner id word) with its normal, tangent and m
 *   nm_classify:              per pixel OWNED 1 | LIT 2 | FRAME 4 (tt passed) | MAPPED 8 (rr passed: out = R / |R|) */
#ifndef TR_BODY
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

static int owned(uint32_t id, uint32_t n_tris) { return ((id & 0x7fffffffu) - 1u) < n_tris; }

#define TR_BODY
#define real float
#define TR(name) tr32_##name
#define SQRT sqrtf
#define FMA fmaf
#define REAL_MAX FLT_MAX
#include "tangent_ref.c"
#undef real
#undef TR
#undef SQRT
#undef FMA
#undef REAL_MAX
#define real double
#define TR(name) tr64_##name
#define SQRT sqrt
#define FMA fma
#define REAL_MAX DBL_MAX
#include "tangent_ref.c"

#else /* ---------------------------------------------------------------------------------------- the rules, once, in `real` */

/* ---- the mesh tangents */
static real TR(dot3)(const real *a, const real *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
typedef struct {
  real dv1, dv2, det, s;
} TR(FaceUv);
static TR(FaceUv) TR(face_uv)(const real *uv, const uint32_t *f) {
  const real *q0 = uv + 2 * (size_t)f[0], *q1 = uv + 2 * (size_t)f[1], *q2 = uv + 2 * (size_t)f[2];
  const real du1 = q1[0] - q0[0], dv1 = q1[1] - q0[1], du2 = q2[0] - q0[0], dv2 = q2[1] - q0[1];
  TR(FaceUv) r;
  r.dv1 = dv1, r.dv2 = dv2, r.det = du1 * dv2 - du2 * dv1, r.s = r.det < 0 ? (real)-1 : (real)1;
  return r;
}
static void TR(tan_sum)(const uint32_t *faces, const uint32_t *corners, uint32_t c0, uint32_t c1, const real *pos, const real *uv, real *S,
                        real *D) {
  S[0] = S[1] = S[2] = 0, *D = 0;
  for (uint32_t c = c0; c < c1; ++c) {
    const uint32_t *f = faces + 3 * (size_t)(corners[c] / 3u);
    const real *p0 = pos + 3 * (size_t)f[0], *p1 = pos + 3 * (size_t)f[1], *p2 = pos + 3 * (size_t)f[2];
    const TR(FaceUv) q = TR(face_uv)(uv, f);
    for (int i = 0; i < 3; ++i) {
      const real e1 = p1[i] - p0[i], e2 = p2[i] - p0[i];
      const real Tf = e1 * q.dv2 - e2 * q.dv1;
      S[i] = S[i] + q.s * Tf;
    }
    *D = *D + q.det;
  }
}
static int TR(scale)(const real *S, real *r) {
  const real len2 = TR(dot3)(S, S);
  const int ok = len2 > 0 && len2 <= REAL_MAX;
  *r = ok ? 1 / SQRT(len2) : 0;
  return ok;
}
void TR(tangents)(uint32_t n_verts, const uint32_t *faces, const uint32_t *corner_off, const uint32_t *corners, const real *pos, const real *uv,
                  real *tan) {
  for (uint32_t v = 0; v < n_verts; ++v) {
    real S[3], D, r;
    TR(tan_sum)(faces, corners, corner_off[v], corner_off[v + 1], pos, uv, S, &D);
    const int ok = TR(scale)(S, &r);
    for (int i = 0; i < 3; ++i) tan[4 * (size_t)v + i] = ok ? S[i] * r : 0;
    tan[4 * (size_t)v + 3] = D < 0 ? (real)-1 : (real)1;
  }
}
void TR(tangents_classify)(uint32_t n_verts, const uint32_t *faces, const uint32_t *corner_off, const uint32_t *corners, const real *pos,
                           const real *uv, uint8_t *cls) {
  for (uint32_t v = 0; v < n_verts; ++v) {
    real S[3], D, r;
    TR(tan_sum)(faces, corners, corner_off[v], corner_off[v + 1], pos, uv, S, &D);
    cls[v] = (uint8_t)((corner_off[v + 1] > corner_off[v] ? 1 : 0) | (TR(scale)(S, &r) ? 2 : 0) | (D < 0 ? 4 : 0));
  }
}
/* gtan: [V][4] (w never read); work, gpos: [V][3] */
void TR(tangents_grad)(uint32_t n_verts, const uint32_t *faces, const uint32_t *corner_off, const uint32_t *corners, const real *pos,
                       const real *uv, const real *gtan, real *work, real *gpos) {
  for (uint32_t v = 0; v < n_verts; ++v) {
    real S[3], D, r, *gS = work + 3 * (size_t)v;
    TR(tan_sum)(faces, corners, corner_off[v], corner_off[v + 1], pos, uv, S, &D);
    gS[0] = gS[1] = gS[2] = 0;
    if (TR(scale)(S, &r)) {
      const real t[3] = {S[0] * r, S[1] * r, S[2] * r}, *g = gtan + 4 * (size_t)v;
      const real d = TR(dot3)(t, g);
      for (int i = 0; i < 3; ++i) gS[i] = (g[i] - t[i] * d) * r;
    }
  }
  for (uint32_t v = 0; v < n_verts; ++v) {
    real acc[3] = {0, 0, 0};
    for (uint32_t c = corner_off[v]; c < corner_off[v + 1]; ++c) {
      const uint32_t face = corners[c] / 3u, k = corners[c] - 3u * face;
      const uint32_t *f = faces + 3 * (size_t)face;
      const TR(FaceUv) q = TR(face_uv)(uv, f);
      const real co = k == 0u ? q.s * (q.dv1 - q.dv2) : k == 1u ? q.s * q.dv2 : -(q.s * q.dv1);
      for (int i = 0; i < 3; ++i) {
        const real G = (work[3 * (size_t)f[0] + i] + work[3 * (size_t)f[1] + i]) + work[3 * (size_t)f[2] + i];
        acc[i] = acc[i] + G * co;
      }
    }
    for (int i = 0; i < 3; ++i) gpos[3 * (size_t)v + i] = acc[i];
  }
}

/* ---- the normal-mapping pass */
static real TR(dot)(const real *a, const real *b) { return FMA(a[0], b[0], FMA(a[1], b[1], a[2] * b[2])); }
static int TR(pos)(real x) { return x > 0 && x < (real)INFINITY; }
static void TR(cross)(const real *u, const real *w, real *c) {
  c[0] = u[1] * w[2] - u[2] * w[1], c[1] = u[2] * w[0] - u[0] * w[2], c[2] = u[0] * w[1] - u[1] * w[0];
}
typedef struct {
  real N[3], T[3], B[3], o[3], inl, d, it, hw, ir;
} TR(Px);
/* 0: not lit (out = 0), 1: out = N for want of a frame, 2: out = N because R has no finite positive length, 3: out = R / |R| */
static int TR(px)(const real *n, const real *t, const real *m, TR(Px) *px) {
  px->o[0] = px->o[1] = px->o[2] = 0;
  const real nn = TR(dot)(n, n);
  if (!TR(pos)(nn)) return 0;
  px->inl = 1 / SQRT(nn);
  for (int i = 0; i < 3; ++i) px->N[i] = n[i] * px->inl, px->o[i] = px->N[i];
  px->d = TR(dot)(px->N, t);
  real Tp[3], C[3], R[3];
  for (int i = 0; i < 3; ++i) Tp[i] = t[i] - px->N[i] * px->d;
  const real tt = TR(dot)(Tp, Tp);
  if (!TR(pos)(tt)) return 1;
  px->it = 1 / SQRT(tt), px->hw = t[3] < 0 ? (real)-1 : (real)1;
  for (int i = 0; i < 3; ++i) px->T[i] = Tp[i] * px->it;
  TR(cross)(px->N, px->T, C);
  for (int i = 0; i < 3; ++i) px->B[i] = C[i] * px->hw, R[i] = FMA(m[0], px->T[i], FMA(m[1], px->B[i], m[2] * px->N[i]));
  const real rr = TR(dot)(R, R);
  if (!TR(pos)(rr)) return 2;
  px->ir = 1 / SQRT(rr);
  for (int i = 0; i < 3; ++i) px->o[i] = R[i] * px->ir;
  return 3;
}
#define TR_LOAD(i)                                                                                                              \
  const real nk[3] = {nrm[i], nrm[n + i], nrm[2 * n + i]}, tk[4] = {tan[i], tan[n + i], tan[2 * n + i], tan[3 * n + i]}, \
             mk[3] = {m[i], m[n + i], m[2 * n + i]}
/* planes: nrm, m [3][n], tan [4][n]; out [3][n], written at owned pixels, and at nobody's (zeros) when fused */
void TR(nm_forward)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *tan, const real *m, int fused, real *out) {
  for (size_t i = 0; i < n; ++i) {
    if (!owned(ids[i], n_tris)) {
      if (fused) out[i] = out[n + i] = out[2 * n + i] = 0;
      continue;
    }
    TR_LOAD(i);
    TR(Px) px;
    TR(px)(nk, tk, mk, &px);
    for (int c = 0; c < 3; ++c) out[c * n + i] = px.o[c];
  }
}
void TR(nm_classify)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *tan, const real *m, uint8_t *cls) {
  static const uint8_t bits[4] = {1, 1 | 2, 1 | 2 | 4, 1 | 2 | 4 | 8};
  for (size_t i = 0; i < n; ++i) {
    cls[i] = 0;
    if (!owned(ids[i], n_tris)) continue;
    TR_LOAD(i);
    TR(Px) px;
    cls[i] = bits[TR(px)(nk, tk, mk, &px)];
  }
}
/* gnrm, gm: [3][n] or null; gtan: [4][n] or null */
void TR(nm_grad)(size_t n, uint32_t n_tris, const uint32_t *ids, const real *nrm, const real *tan, const real *m, const real *gout, int fused,
                 real *gnrm, real *gtan, real *gm) {
  for (size_t i = 0; i < n; ++i) {
    if (!owned(ids[i], n_tris)) {
      if (fused) {
        if (gnrm) gnrm[i] = gnrm[n + i] = gnrm[2 * n + i] = 0;
        if (gtan) gtan[i] = gtan[n + i] = gtan[2 * n + i] = gtan[3 * n + i] = 0;
        if (gm) gm[i] = gm[n + i] = gm[2 * n + i] = 0;
      }
      continue;
    }
    TR_LOAD(i);
    const real g[3] = {gout[i], gout[n + i], gout[2 * n + i]};
    real gn[3] = {0, 0, 0}, gt[4] = {0, 0, 0, 0}, gmk[3] = {0, 0, 0};
    TR(Px) px;
    const int mode = TR(px)(nk, tk, mk, &px);
    if (mode != 0) {
      real gN[3] = {g[0], g[1], g[2]};
      if (mode == 3) {
        const real dq = TR(dot)(g, px.o);
        real gR[3], gT[3], gC[3], X[3], Y[3], gTp[3];
        for (int c = 0; c < 3; ++c) gR[c] = (g[c] - px.o[c] * dq) * px.ir;
        gmk[0] = TR(dot)(gR, px.T), gmk[1] = TR(dot)(gR, px.B), gmk[2] = TR(dot)(gR, px.N);
        for (int c = 0; c < 3; ++c) gT[c] = mk[0] * gR[c], gC[c] = (mk[1] * gR[c]) * px.hw, gN[c] = mk[2] * gR[c];
        TR(cross)(px.T, gC, X), TR(cross)(gC, px.N, Y);
        for (int c = 0; c < 3; ++c) gN[c] = gN[c] + X[c], gT[c] = gT[c] + Y[c];
        const real dT = TR(dot)(gT, px.T);
        for (int c = 0; c < 3; ++c) gTp[c] = (gT[c] - px.T[c] * dT) * px.it;
        const real gd = -TR(dot)(gTp, px.N);
        for (int c = 0; c < 3; ++c) {
          gN[c] = (gN[c] - gTp[c] * px.d) + gd * tk[c];
          gt[c] = gTp[c] + gd * px.N[c];
        }
      }
      const real dn = TR(dot)(gN, px.N);
      for (int c = 0; c < 3; ++c) gn[c] = (gN[c] - px.N[c] * dn) * px.inl;
    }
    for (int c = 0; c < 3; ++c) {
      if (gnrm) gnrm[c * n + i] = gn[c];
      if (gm) gm[c * n + i] = gmk[c];
    }
    if (gtan)
      for (int c = 0; c < 4; ++c) gtan[c * n + i] = gt[c];
  }
}
#undef TR_LOAD
#endif
