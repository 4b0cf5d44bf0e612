/* The silhouette antialiasing pass's test reference (tests/antialiasref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math).
 * It includes nothing of the library.  The rule is the one include/srz.h states at SILHOUETTE ANTIALIASING, restated here from the
 * text: per pair of 4-neighbours (A = the left or upper pixel, B = the right or lower one) of a visibility buffer, in float32, fmaf
 * where written and nothing else fused:
 *   owner: (id & 0x7fffffff) - 1 < n_tris; a pair of two nobodies or of one triangle index does nothing
 *   N (nearer) = B iff A is nobody, or both have owners and zB < zA; else A.  F = the other.  s = +1 iff F is B
 *   per vertex v of N's triangle: horizontal u = s * (v.x - xN), n = v.y - yN; vertical u = s * (v.y - yN), n = v.x - xN
 *   the first edge (a,b), (b,c), (c,a) with (n0 <= 0 && n1 > 0) || (n1 <= 0 && n0 > 0) and, d = n0 - n1, k = n0 / d,
 *   t = u0 + k * (u1 - u0), 0 <= t <= 1; none: nothing.  F an owner whose corners hold both v0 and v1 word for word: nothing
 *   a = t - 0.5f:  a > 0: target F, source N, w = a;  a < 0: target N, source F, w = -a;  a == 0: nothing
 * Forward and gin in float (bit for bit); gpos in DOUBLE (the sum of the float32 terms), with the sum of |term| and the count of
 * contributing pairs per element, from which the tests derive their bound.  aa_forward64 restates the forward in double as a
 * function of double positions, owners and z held fixed, for finite differences. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

enum { C_DIFFER, C_TGT_N, C_TGT_F, C_HORIZ, C_VERT, C_INTERIOR, C_F_NOBODY, C_NO_EDGE, C_N };

typedef struct {
  int tgt;           /* 0: nothing, 1: A, 2: B */
  int n_is_b, edge;  /* N, and the edge's first corner 0..2 */
  uint32_t n_idx;    /* N's triangle index */
  float w, a, s, k, d, n0, n1, u0, u1;
} pair_t;

static uint32_t word_of(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

static int same_vertex(const float *p, const float *q) {
  return word_of(p[0]) == word_of(q[0]) && word_of(p[1]) == word_of(q[1]) && word_of(p[2]) == word_of(q[2]);
}

/* A at (xa, ya); B at (xa + 1, ya) when horiz, else (xa, ya + 1) */
static pair_t pair_eval(const float *pos, uint32_t n_tris, uint32_t ida, uint32_t idb, float za, float zb, int xa, int ya, int horiz,
                        uint64_t *counters) {
  pair_t r;
  memset(&r, 0, sizeof r);
  const uint32_t ia = (ida & 0x7fffffffu) - 1u, ib = (idb & 0x7fffffffu) - 1u;
  const int oa = ia < n_tris, ob = ib < n_tris;
  if ((!oa && !ob) || (oa && ob && ia == ib)) return r;
  if (counters) counters[C_DIFFER]++;
  r.n_is_b = !oa || (ob && zb < za);
  const int f_owner = r.n_is_b ? oa : ob;
  r.n_idx = r.n_is_b ? ib : ia;
  const uint32_t f_idx = r.n_is_b ? ia : ib;
  r.s = r.n_is_b ? -1.0f : 1.0f;
  const float xn = (float)(xa + (horiz && r.n_is_b)), yn = (float)(ya + (!horiz && r.n_is_b));
  const float *P = pos + (size_t)r.n_idx * 9u;
  float u[3], n[3];
  for (int v = 0; v < 3; ++v) {
    const float dx = P[3 * v] - xn, dy = P[3 * v + 1] - yn;
    u[v] = horiz ? r.s * dx : r.s * dy;
    n[v] = horiz ? dy : dx;
  }
  int found = 0;
  float t = 0.0f;
  for (int e = 0; e < 3 && !found; ++e) {
    const int e1 = (e + 1) % 3;
    const float n0 = n[e], n1 = n[e1];
    if (!((n0 <= 0.0f && n1 > 0.0f) || (n1 <= 0.0f && n0 > 0.0f))) continue;
    const float d = n0 - n1, k = n0 / d;
    t = u[e] + k * (u[e1] - u[e]);
    if (!(0.0f <= t && t <= 1.0f)) continue;
    found = 1, r.edge = e, r.k = k, r.d = d, r.n0 = n0, r.n1 = n1, r.u0 = u[e], r.u1 = u[e1];
  }
  if (!found) {
    if (counters) counters[C_NO_EDGE]++;
    return r;
  }
  if (f_owner) {
    const float *Q = pos + (size_t)f_idx * 9u, *v0 = P + 3 * r.edge, *v1 = P + 3 * ((r.edge + 1) % 3);
    const int has0 = same_vertex(v0, Q) || same_vertex(v0, Q + 3) || same_vertex(v0, Q + 6);
    const int has1 = same_vertex(v1, Q) || same_vertex(v1, Q + 3) || same_vertex(v1, Q + 6);
    if (has0 && has1) {
      if (counters) counters[C_INTERIOR]++;
      return r;
    }
  }
  r.a = t - 0.5f;
  if (r.a > 0.0f)
    r.tgt = r.n_is_b ? 1 : 2, r.w = r.a; /* F */
  else if (r.a < 0.0f)
    r.tgt = r.n_is_b ? 2 : 1, r.w = -r.a; /* N */
  if (r.tgt && counters) {
    counters[r.a > 0.0f ? C_TGT_F : C_TGT_N]++;
    counters[horiz ? C_HORIZ : C_VERT]++;
    if (!f_owner) counters[C_F_NOBODY]++;
  }
  return r;
}

/* the pair of pixel p = (x, y) with its neighbour j (0: x - 1, 1: x + 1, 2: y - 1, 3: y + 1); *q the neighbour's index; *p_is_a */
static pair_t pair_of(const float *pos, uint32_t n_tris, int rows, int W, const uint32_t *id, const float *z, int x, int y, int j,
                      size_t *q, int *p_is_a) {
  const int qx = x + (j == 0 ? -1 : j == 1 ? 1 : 0), qy = y + (j == 2 ? -1 : j == 3 ? 1 : 0);
  pair_t none;
  memset(&none, 0, sizeof none);
  *q = 0, *p_is_a = 0;
  if (qx < 0 || qx >= W || qy < 0 || qy >= rows) return none;
  const size_t p = (size_t)y * W + x;
  *q = (size_t)qy * W + qx;
  *p_is_a = j == 1 || j == 3;
  const size_t a = *p_is_a ? p : *q, b = *p_is_a ? *q : p;
  return pair_eval(pos, n_tris, id[a], id[b], z[a], z[b], (int)(a % W), (int)(a / W), j < 2, NULL);
}

/* pos: [n_tris or more][9]; z, id: planes 0 and 1 of the frame's visibility buffer, rows x W words each; in: n_ch planes; out: n_ch
 * planes, every word written */
void aa_forward(const float *pos, uint32_t n_tris, int rows, int W, const float *z, const uint32_t *id, const float *in, int n_ch,
                float *out) {
  const size_t plane = (size_t)rows * W;
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t p = (size_t)y * W + x;
      pair_t pr[4];
      size_t q[4];
      for (int j = 0; j < 4; ++j) {
        int p_is_a;
        pr[j] = pair_of(pos, n_tris, rows, W, id, z, x, y, j, &q[j], &p_is_a);
        if (pr[j].tgt != (p_is_a ? 1 : 2)) pr[j].tgt = 0; /* only pairs whose target is p */
      }
      for (int ch = 0; ch < n_ch; ++ch) {
        const float *c = in + ch * plane;
        float acc = c[p];
        for (int j = 0; j < 4; ++j)
          if (pr[j].tgt) acc = fmaf(pr[j].w, c[q[j]] - c[p], acc);
        out[ch * plane + p] = acc;
      }
    }
}

/* gin: n_ch planes or null; ginabs: n_ch planes of doubles (sum of |term| per word) or null.  gpos, gabs: [..][9] doubles, added
 * into; count: [..][9] contributing pairs per element, added into (any of the three may be null).  counters: C_N words, added into,
 * or null */
void aa_backward(const float *pos, uint32_t n_tris, int rows, int W, const float *z, const uint32_t *id, const float *in,
                 const float *gout, int n_ch, float *gin, double *ginabs, double *gpos, double *gabs, uint32_t *count, uint64_t *counters) {
  const size_t plane = (size_t)rows * W;
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t p = (size_t)y * W + x;
      pair_t pr[4];
      size_t q[4];
      int p_is_a[4];
      for (int j = 0; j < 4; ++j) pr[j] = pair_of(pos, n_tris, rows, W, id, z, x, y, j, &q[j], &p_is_a[j]);
      if (gin)
        for (int ch = 0; ch < n_ch; ++ch) {
          const float *g = gout + ch * plane;
          float acc = g[p];
          double mag = fabs((double)g[p]);
          for (int j = 0; j < 4; ++j) {
            if (!pr[j].tgt) continue;
            if (pr[j].tgt == (p_is_a[j] ? 1 : 2))
              acc = fmaf(-pr[j].w, g[p], acc), mag += fabs((double)pr[j].w * (double)g[p]);
            else
              acc = fmaf(pr[j].w, g[q[j]], acc), mag += fabs((double)pr[j].w * (double)g[q[j]]);
          }
          gin[ch * plane + p] = acc;
          if (ginabs) ginabs[ch * plane + p] = mag;
        }
      /* each pair once: from its left or upper pixel */
      for (int j = 1; j < 4; j += 2) {
        const int qx = x + (j == 1), qy = y + (j == 3);
        if (qx >= W || qy >= rows) continue;
        const size_t b = (size_t)qy * W + qx;
        const pair_t r = pair_eval(pos, n_tris, id[p], id[b], z[p], z[b], x, y, j == 1, counters);
        if (!r.tgt) continue;
        const size_t tgt = r.tgt == 1 ? p : b, src = r.tgt == 1 ? b : p;
        float D = 0.0f;
        for (int ch = 0; ch < n_ch; ++ch) D = fmaf(gout[ch * plane + tgt], in[ch * plane + src] - in[ch * plane + tgt], D);
        const float g = r.a > 0.0f ? D : -D;
        const float e = r.u1 - r.u0;
        const float qq = (g * e) / (r.d * r.d);
        const float g_u0 = g * (1.0f - r.k), g_u1 = g * r.k;
        const float g_n0 = qq * (-r.n1), g_n1 = qq * r.n0;
        const int c0 = r.edge, c1 = (r.edge + 1) % 3, horiz = j == 1;
        const size_t slot[4] = {(size_t)r.n_idx * 9u + 3 * c0 + 0, (size_t)r.n_idx * 9u + 3 * c1 + 0, (size_t)r.n_idx * 9u + 3 * c0 + 1,
                                (size_t)r.n_idx * 9u + 3 * c1 + 1}; /* x of v0, x of v1, y of v0, y of v1 */
        const float term[4] = {horiz ? r.s * g_u0 : g_n0, horiz ? r.s * g_u1 : g_n1, horiz ? g_n0 : r.s * g_u0, horiz ? g_n1 : r.s * g_u1};
        for (int i = 0; i < 4; ++i) {
          if (gpos) gpos[slot[i]] += (double)term[i];
          if (gabs) gabs[slot[i]] += fabs((double)term[i]);
          if (count) count[slot[i]] += 1u;
        }
      }
    }
}

/* The forward restated in double as a function of double positions pos64 [..][9]; owners, z (plane 0) and the pixel grid held fixed.
 * The interior-edge rule compares the doubles.  out: n_ch planes of doubles.  decision (may be null): 2 planes of bytes, [0] the
 * pair of (x, y) with (x + 1, y), [1] with (x, y + 1): 0 nothing (no pair, no edge, interior, a == 0), else 1 + 2 * edge + (a > 0),
 * + 8 when N is B — what a finite-difference test compares between the two ends of its step */
void aa_forward64(const double *pos, uint32_t n_tris, int rows, int W, const float *z, const uint32_t *id, const double *in, int n_ch,
                  double *out, uint8_t *decision) {
  const size_t plane = (size_t)rows * W;
  for (size_t i = 0; i < plane * (size_t)n_ch; ++i) out[i] = in[i];
  if (decision) memset(decision, 0, 2 * plane);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < W; ++x)
      for (int horiz = 1; horiz >= 0; --horiz) {
        const int qx = x + horiz, qy = y + !horiz;
        if (qx >= W || qy >= rows) continue;
        const size_t a = (size_t)y * W + x, b = (size_t)qy * W + qx;
        const uint32_t ia = (id[a] & 0x7fffffffu) - 1u, ib = (id[b] & 0x7fffffffu) - 1u;
        const int oa = ia < n_tris, ob = ib < n_tris;
        if ((!oa && !ob) || (oa && ob && ia == ib)) continue;
        const int n_is_b = !oa || (ob && z[b] < z[a]);
        const int f_owner = n_is_b ? oa : ob;
        const uint32_t n_idx = n_is_b ? ib : ia, f_idx = n_is_b ? ia : ib;
        const double s = n_is_b ? -1.0 : 1.0;
        const double xn = x + (horiz && n_is_b), yn = y + (!horiz && n_is_b);
        const double *P = pos + (size_t)n_idx * 9u;
        double u[3], n[3];
        for (int v = 0; v < 3; ++v) {
          const double dx = P[3 * v] - xn, dy = P[3 * v + 1] - yn;
          u[v] = horiz ? s * dx : s * dy, n[v] = horiz ? dy : dx;
        }
        int edge = -1;
        double t = 0.0;
        for (int e = 0; e < 3 && edge < 0; ++e) {
          const int e1 = (e + 1) % 3;
          if (!((n[e] <= 0.0 && n[e1] > 0.0) || (n[e1] <= 0.0 && n[e] > 0.0))) continue;
          t = u[e] + n[e] / (n[e] - n[e1]) * (u[e1] - u[e]);
          if (0.0 <= t && t <= 1.0) edge = e;
        }
        if (edge < 0) continue;
        if (f_owner) {
          const double *Q = pos + (size_t)f_idx * 9u;
          int has[2] = {0, 0};
          for (int i = 0; i < 2; ++i) {
            const double *v = P + 3 * ((edge + i) % 3);
            for (int c = 0; c < 3; ++c) has[i] |= v[0] == Q[3 * c] && v[1] == Q[3 * c + 1] && v[2] == Q[3 * c + 2];
          }
          if (has[0] && has[1]) continue;
        }
        const double aa = t - 0.5;
        if (aa == 0.0) continue;
        const size_t nn = n_is_b ? b : a, ff = n_is_b ? a : b;
        const size_t tgt = aa > 0.0 ? ff : nn, src = aa > 0.0 ? nn : ff;
        const double w = fabs(aa);
        for (int ch = 0; ch < n_ch; ++ch) out[ch * plane + tgt] += w * (in[ch * plane + src] - in[ch * plane + tgt]);
        if (decision) decision[(horiz ? 0 : plane) + a] = (uint8_t)(1 + 2 * edge + (aa > 0.0) + 8 * n_is_b);
      }
}
