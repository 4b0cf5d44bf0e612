/* The visibility buffer's test reference (tests/visref.py builds it with gcc -O2 -ffp-contract=off).  It never reads the
 * oracle's internals: the owner of a pixel is DECODED from the oracle's NORMAL-shaded colour, every triangle carrying a flat
 * normal of its own, chosen so that any two triangles whose bounding boxes overlap differ by >= SEP levels of 255 in some
 * channel; alpha / beta / z of that owner are then recomputed here with the shaders' operations (cover_v / cover_s of the
 * kernels, the oracle's V / S semantics), with fmaf where they fuse and nothing else fused. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define TILE 32

static float minf3(float a, float b, float c) { float m = a; if (b < m) m = b; if (c < m) m = c; return m; }
static float maxf3(float a, float b, float c) { float m = a; if (m < b) m = b; if (m < c) m = c; return m; }
static float clampf_(float v, float lo, float hi) { return (v < lo) ? lo : (hi < v) ? hi : v; }
static long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (hi < v ? hi : v); }

/* Triangle::calcBoundingBox as the rasterisers clip it; box[4 i] = {sx, sy, ex, ey}, sx > ex: no box (non-finite) */
void vr_boxes(const float *pos, int n, int W, int H, int32_t *box) {
  for (int i = 0; i < n; ++i) {
    const float *p = pos + 9 * (size_t)i;
    int32_t *b = box + 4 * (size_t)i;
    int ok = 1;
    for (int k = 0; k < 9; ++k) ok &= isfinite(p[k]) != 0;
    if (!ok) { b[0] = 1, b[1] = 1, b[2] = 0, b[3] = 0; continue; }
    const float BIG = 1099511627776.0f;
    float mnx = clampf_(minf3(p[0], p[3], p[6]), -BIG, BIG), mxx = clampf_(maxf3(p[0], p[3], p[6]), -BIG, BIG);
    float mny = clampf_(minf3(p[1], p[4], p[7]), -BIG, BIG), mxy = clampf_(maxf3(p[1], p[4], p[7]), -BIG, BIG);
    b[0] = (int32_t)clampll((long long)mnx, 0, W - 1), b[1] = (int32_t)clampll((long long)mny, 0, H - 1);
    b[2] = (int32_t)clampll((long long)mxx, 0, W - 1), b[3] = (int32_t)clampll((long long)mxy, 0, H - 1);
  }
}

/* CSR of the triangles whose box reaches each 32x32 tile, in index order */
static int tiles_csr(const int32_t *box, int n, int W, int H, int **off_out, int **lst_out) {
  const int tx = (W + TILE - 1) / TILE, ty = (H + TILE - 1) / TILE;
  int *off = calloc((size_t)tx * ty + 1, sizeof(int));
  if (!off) return -1;
  for (int i = 0; i < n; ++i) {
    const int32_t *b = box + 4 * (size_t)i;
    if (b[0] > b[2]) continue;
    for (int y = b[1] / TILE; y <= b[3] / TILE; ++y)
      for (int x = b[0] / TILE; x <= b[2] / TILE; ++x) off[y * tx + x + 1]++;
  }
  for (int t = 0; t < tx * ty; ++t) off[t + 1] += off[t];
  int *lst = malloc(sizeof(int) * (size_t)(off[tx * ty] ? off[tx * ty] : 1)), *fill = malloc(sizeof(int) * (size_t)tx * ty);
  if (!lst || !fill) return -1;
  for (int t = 0; t < tx * ty; ++t) fill[t] = off[t];
  for (int i = 0; i < n; ++i) {
    const int32_t *b = box + 4 * (size_t)i;
    if (b[0] > b[2]) continue;
    for (int y = b[1] / TILE; y <= b[3] / TILE; ++y)
      for (int x = b[0] / TILE; x <= b[2] / TILE; ++x) lst[fill[y * tx + x]++] = i;
  }
  free(fill);
  *off_out = off, *lst_out = lst;
  return 0;
}

static int overlap(const int32_t *a, const int32_t *b) { return a[0] <= b[2] && b[0] <= a[2] && a[1] <= b[3] && b[1] <= a[3]; }

/* Greedy: triangle i takes the first candidate colour (lev: m x 3 levels, from start (i * 7919) % m on) that differs by >= sep in some
 * channel from every earlier triangle whose box overlaps its own.  choice[i] = candidate, or -1 (no box).  Returns the number of
 * triangles no candidate fits (must be 0). */
int vr_assign(const int32_t *box, int n, int W, int H, const double *lev, int m, double sep, int32_t *choice) {
  int *off, *lst;
  if (tiles_csr(box, n, W, H, &off, &lst)) return -1;
  const int tx = (W + TILE - 1) / TILE;
  int *nb = malloc(sizeof(int) * (size_t)(n ? n : 1)), *seen = calloc((size_t)(n ? n : 1), sizeof(int)), failed = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t *b = box + 4 * (size_t)i;
    choice[i] = -1;
    if (b[0] > b[2]) continue;
    int nn = 0;
    for (int y = b[1] / TILE; y <= b[3] / TILE; ++y)
      for (int x = b[0] / TILE; x <= b[2] / TILE; ++x)
        for (int j = off[y * tx + x]; j < off[y * tx + x + 1] && lst[j] < i; ++j) {
          const int k = lst[j];
          if (seen[k] != i + 1 && overlap(b, box + 4 * (size_t)k)) seen[k] = i + 1, nb[nn++] = k;
        }
    for (int t = 0; t < m && choice[i] < 0; ++t) {
      const int c = (int)(((long long)i * 7919 + t) % m);
      int ok = 1;
      for (int q = 0; q < nn && ok; ++q) {
        const double *u = lev + 3 * (size_t)c, *v = lev + 3 * (size_t)choice[nb[q]];
        ok = fabs(u[0] - v[0]) >= sep || fabs(u[1] - v[1]) >= sep || fabs(u[2] - v[2]) >= sep;
      }
      if (ok) choice[i] = c;
    }
    if (choice[i] < 0) failed++, choice[i] = 0;
  }
  free(nb), free(seen), free(off), free(lst);
  return failed;
}

/* owner[p] of every pixel the oracle changed (owned[p] != 0): the triangle whose box contains the pixel and whose colour (tlev: n x 3 levels) is within
 * tol of the pixel's colour in every channel — exactly one of them, else the pixel is AMBIGUOUS (owner -2, counted in the return
 * value).  Other pixels: -1. */
int vr_decode(const int32_t *box, int n, int W, int H, const double *tlev, double tol, const uint8_t *owned, const float *c0, const float *c1,
              const float *c2, int32_t *owner) {
  int *off, *lst;
  if (tiles_csr(box, n, W, H, &off, &lst)) return -1;
  const int tx = (W + TILE - 1) / TILE;
  int bad = 0;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t p = (size_t)y * W + x;
      owner[p] = -1;
      if (!owned[p]) continue;
      const int t = (y / TILE) * tx + x / TILE;
      int hit = -2, hits = 0;
      for (int j = off[t]; j < off[t + 1]; ++j) {
        const int k = lst[j];
        const int32_t *b = box + 4 * (size_t)k;
        if (x < b[0] || x > b[2] || y < b[1] || y > b[3]) continue;
        const double *u = tlev + 3 * (size_t)k;
        if (fabs(c0[p] - u[0]) <= tol && fabs(c1[p] - u[1]) <= tol && fabs(c2[p] - u[2]) <= tol) hit = k, hits++;
      }
      owner[p] = hits == 1 ? hit : -2;
      bad += hits != 1;
    }
  free(off), free(lst);
  return bad;
}

/* class (0 V, 1 S), alpha, beta and z of every owned pixel (owner >= 0) of rows [0, H), as the shaders compute them:
 * V (x < sx + (width of the box rounded down to 8), every x when unified): cover_v; S: cover_s */
void vr_bary(const float *pos, const int32_t *box, int W, int H, int unified, const int32_t *owner, uint8_t *cls, float *alpha,
             float *beta, float *zo) {
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t p = (size_t)y * W + x;
      cls[p] = 0, alpha[p] = beta[p] = 0.0f, zo[p] = INFINITY;
      if (owner[p] < 0) continue;
      const float *t = pos + 9 * (size_t)owner[p];
      const int32_t *b = box + 4 * (size_t)owner[p];
      const float ax = t[0], ay = t[1], z0 = t[2], bx = t[3], by = t[4], z1 = t[5], cx = t[6], cy = t[7], z2 = t[8];
      const float fx = (float)x, fy = (float)y;
      const long long bw = b[2] - b[0] + 1, vend = unified ? (long long)b[2] + 1 : b[0] + ((bw >> 3) << 3);
      const float ABx = bx - ax, ABy = by - ay, ACx = cx - ax, ACy = cy - ay;
      if (x < vend) {
        const float v_inv = 1.0f / fmaf(ABx, ACy, -(ACx * ABy));
        const float PBx = bx - fx, PBy = by - fy, PCx = cx - fx, PCy = cy - fy, PAx = ax - fx, PAy = ay - fy;
        const float aPBC = fmaf(PBx, PCy, -(PCx * PBy)), aPCA = fmaf(PCx, PAy, -(PAx * PCy));
        const float a = aPBC * v_inv, be = aPCA * v_inv, g = 1.0f - (a + be);
        alpha[p] = a, beta[p] = be, zo[p] = fmaf(a, z0, fmaf(be, z1, g * z2));
      } else {
        const float s_area = ABx * ACy - ABy * ACx;
        const float PAx = ax - fx, PAy = ay - fy, PBx = bx - fx, PBy = by - fy, PCx = cx - fx, PCy = cy - fy;
        const float aPBC = PBx * PCy - PBy * PCx, aPCA = PCx * PAy - PCy * PAx;
        const float a = aPBC / s_area, be = aPCA / s_area, g = 1.0f - a - be;
        cls[p] = 1, alpha[p] = a, beta[p] = be, zo[p] = a * z0 + be * z1 + g * z2;
      }
    }
}
