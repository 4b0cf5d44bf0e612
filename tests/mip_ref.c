/* The mip passes' test reference (tests/mipref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math).  It includes nothing of the
 * library and restates what include/srz.h states for srz_texture_mip_levels / _bytes / _build / _fold, srz_frameset_interpolate_deriv
 * and srz_frameset_texture_mip / _texture_mip_grad:
 *   the pyramid: level l + 1 exists iff (w > 1 or h > 1) and w is even or 1 and h is even or 1; w' = max(1, w / 2), h' likewise;
 *     build, each level from the one above: ((t00 + t01) + (t10 + t11)) * 0.25f, or (t0 + t1) * 0.5f along the one extent left;
 *     fold: acc = g_(L-1); for l = L - 2 .. 1: acc = fmaf(k_(l+1), acc, g_l); gtex = fmaf(k_1, acc, gtex)
 *   the derivatives: area, r = 1.0f / area, gax = (by - cy) * r, gay = (cx - bx) * r, gbx = (cy - ay) * r, gby = (ax - cx) * r;
 *     da = a - c, db = b - c; d/dx = fmaf(da, gax, db * gbx), d/dy = fmaf(da, gay, db * gby)
 *   the level: fin, ax = ux * W, ay = vx * H, bx = uy * W, by = vy * H, rx = fmaf(ax, ax, ay * ay), ry = fmaf(bx, bx, by * by),
 *     r2 = rx > ry ? rx : ry; not fin or not r2 < inf: (L - 1, 0); rho = sqrtf(r2); not rho > 1: (0, 0); m = frexpf(rho, &e),
 *     l = e - 1, f = fmaf(2, m, -1); l >= L - 1: (L - 1, 0), else (l, f)
 *   the sample: the bilinear rule of tests/tex_ref.c per level (restated here, not shared); out = c_l0, or fmaf(f, c_l1 - c_l0, c_l0)
 *   the backward: the float32 products (w_rc * lw) * g summed in DOUBLE per level with the counts of contributing adds and the sums
 *     of |product|; guv in float, blended by f as the samples are.
 * A texture frame's pyramid here is that of ONE frame: [h_l][w_l][C] per level, the levels one after another. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

enum { MR_CLAMP = 0, MR_WRAP = 1, MR_MAX_SIZE = 16384 };

static int half_ok(int n) { return n % 2 == 0 || n == 1; }
static int halve(int n) { return n / 2 > 1 ? n / 2 : 1; }

uint32_t mr_levels(int w, int h) {
  if (w < 1 || h < 1 || w > MR_MAX_SIZE || h > MR_MAX_SIZE) return 0;
  uint32_t n = 1;
  while ((w > 1 || h > 1) && half_ok(w) && half_ok(h)) w = halve(w), h = halve(h), ++n;
  return n;
}
/* the extents of level l (by halving, not by shifting) and the build's factor into it (level >= 1) */
void mr_level(int w, int h, uint32_t l, int *wl, int *hl, float *factor) {
  float k = 0.0f;
  for (uint32_t i = 0; i < l; ++i) {
    k = w > 1 && h > 1 ? 0.25f : 0.5f;
    w = halve(w), h = halve(h);
  }
  *wl = w, *hl = h, *factor = k;
}
/* floats of one frame's levels 1 .. l - 1 */
static size_t level_off(int w, int h, uint32_t C, uint32_t l) {
  size_t s = 0;
  for (uint32_t i = 1; i < l; ++i) {
    int wl, hl;
    float k;
    mr_level(w, h, i, &wl, &hl, &k);
    s += (size_t)wl * hl * C;
  }
  return s;
}

/* tex [F][H][W][C] -> mip: level-major, level l [F][h_l][w_l][C] */
void mr_build(const float *tex, int W, int H, uint32_t C, uint32_t F, uint32_t L, float *mip) {
  const float *src = tex;
  float *dst = mip;
  int sw = W, sh = H;
  for (uint32_t l = 1; l < L; ++l) {
    const int dw = halve(sw), dh = halve(sh);
    for (uint32_t f = 0; f < F; ++f)
      for (int y = 0; y < dh; ++y)
        for (int x = 0; x < dw; ++x)
          for (uint32_t ch = 0; ch < C; ++ch) {
            const float *s = src + (size_t)f * sh * sw * C + ch;
            float v;
            if (sw > 1 && sh > 1) {
              const float t00 = s[((size_t)(2 * y) * sw + 2 * x) * C], t01 = s[((size_t)(2 * y) * sw + 2 * x + 1) * C];
              const float t10 = s[((size_t)(2 * y + 1) * sw + 2 * x) * C], t11 = s[((size_t)(2 * y + 1) * sw + 2 * x + 1) * C];
              v = ((t00 + t01) + (t10 + t11)) * 0.25f;
            } else if (sw > 1) {
              v = (s[(size_t)(2 * x) * C] + s[(size_t)(2 * x + 1) * C]) * 0.5f;
            } else {
              v = (s[(size_t)(2 * y) * C] + s[(size_t)(2 * y + 1) * C]) * 0.5f;
            }
            dst[(((size_t)f * dh + y) * dw + x) * C + ch] = v;
          }
    src = dst, dst += (size_t)F * dh * dw * C, sw = dw, sh = dh;
  }
}

/* gmip (mr_build's layout) folded into gtex [F][H][W][C], added into */
void mr_fold(const float *gmip, int W, int H, uint32_t C, uint32_t F, uint32_t L, float *gtex) {
  if (L < 2) return;
  for (uint32_t f = 0; f < F; ++f)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        for (uint32_t ch = 0; ch < C; ++ch) {
          float acc = 0.0f;
          for (uint32_t l = L - 1; l >= 1; --l) {
            int wl, hl, wu, hu;
            float k, ku;
            mr_level(W, H, l, &wl, &hl, &k);
            const float g = gmip[level_off(W, H, C, l) * F + (((size_t)f * hl + (y >> l)) * wl + (x >> l)) * C + ch];
            if (l == L - 1) {
              acc = g;
            } else {
              mr_level(W, H, l + 1, &wu, &hu, &ku);
              acc = fmaf(ku, acc, g);
            }
          }
          int w1, h1;
          float k1;
          mr_level(W, H, 1, &w1, &h1, &k1);
          float *d = gtex + (((size_t)f * H + y) * W + x) * C + ch;
          *d = fmaf(k1, acc, *d);
        }
}

static int owned(uint32_t id, uint32_t n_tris) { return (id & 0x7fffffffu) - 1u < n_tris; }

/* attr [T][3][C], pos [T][9] (ax ay z0 bx by z1 cx cy z2), id: plane 1 of the frame's visibility buffer; out: 2 C planes of n_px */
void mr_deriv(const float *attr, uint32_t C, const float *pos, uint32_t n_tris, size_t n_px, const uint32_t *id, int fused, float *out) {
  for (size_t p = 0; p < n_px; ++p) {
    if (!owned(id[p], n_tris)) {
      if (fused)
        for (uint32_t k = 0; k < 2 * C; ++k) out[k * n_px + p] = 0.0f;
      continue;
    }
    const uint32_t t = (id[p] & 0x7fffffffu) - 1u;
    const float *P = pos + (size_t)t * 9;
    const float ax = P[0], ay = P[1], bx = P[3], by = P[4], cx = P[6], cy = P[7];
    const float area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    const float r = 1.0f / area;
    const float gax = (by - cy) * r, gay = (cx - bx) * r, gbx = (cy - ay) * r, gby = (ax - cx) * r;
    for (uint32_t ch = 0; ch < C; ++ch) {
      const float a = attr[((size_t)t * 3 + 0) * C + ch], b = attr[((size_t)t * 3 + 1) * C + ch], c = attr[((size_t)t * 3 + 2) * C + ch];
      const float da = a - c, db = b - c;
      out[(2 * ch) * n_px + p] = fmaf(da, gax, db * gbx);
      out[(2 * ch + 1) * n_px + p] = fmaf(da, gay, db * gby);
    }
  }
}

static void lod(float ux, float uy, float vx, float vy, int W, int H, uint32_t L, uint32_t *l0, float *f) {
  *l0 = L - 1, *f = 0.0f;
  const int fin = fabsf(ux) < INFINITY && fabsf(uy) < INFINITY && fabsf(vx) < INFINITY && fabsf(vy) < INFINITY;
  if (!fin) return;
  const float ax = ux * (float)W, ay = vx * (float)H, bx = uy * (float)W, by = vy * (float)H;
  const float rx = fmaf(ax, ax, ay * ay), ry = fmaf(bx, bx, by * by), r2 = rx > ry ? rx : ry;
  if (!(r2 < INFINITY)) return;
  const float rho = sqrtf(r2);
  if (!(rho > 1.0f)) {
    *l0 = 0;
    return;
  }
  int e;
  const float m = frexpf(rho, &e);
  const int l = e - 1;
  if (l >= (int)L - 1) return;
  *l0 = (uint32_t)l, *f = fmaf(2.0f, m, -1.0f);
}

/* uvd: 4 planes of n_px (ux, uy, vx, vy) -> l0 and f per pixel (every pixel: owners play no part here) */
void mr_lod(int W, int H, uint32_t L, size_t n_px, const float *uvd, uint32_t *l0, float *f) {
  for (size_t p = 0; p < n_px; ++p) lod(uvd[p], uvd[n_px + p], uvd[2 * n_px + p], uvd[3 * n_px + p], W, H, L, l0 + p, f + p);
}

typedef struct {
  int x0, x1, y0, y1;
  float tx, ty;
  int in_x, in_y;
} Tap;
static void axis(float u, int n, int mode, int *i0, int *i1, float *t, int *in) {
  if (mode == MR_WRAP) u = u - floorf(u);
  float fx = u * (float)n - 0.5f;
  *in = 1;
  if (mode == MR_CLAMP) {
    *in = fx > 0.0f && fx < (float)(n - 1);
    fx = fminf(fmaxf(fx, 0.0f), (float)(n - 1));
  }
  const float f0 = floorf(fx);
  *t = fx - f0;
  *i0 = (int)f0, *i1 = *i0 + 1;
  if (mode == MR_CLAMP) {
    if (*i1 > n - 1) *i1 = n - 1;
  } else {
    if (*i0 < 0) *i0 += n;
    if (*i1 >= n) *i1 -= n;
  }
}
static void tap_of(float u, float v, int w, int h, int mode, Tap *p) {
  axis(u, w, mode, &p->x0, &p->x1, &p->tx, &p->in_x);
  axis(v, h, mode, &p->y0, &p->y1, &p->ty, &p->in_y);
}
/* level l of one frame: level 0 is tex, the others lie in mip */
static const float *level_of(const float *tex, const float *mip, int W, int H, uint32_t C, uint32_t l) {
  return l == 0 ? tex : mip + level_off(W, H, C, l);
}
static float bilinear(const float *t, int w, uint32_t C, const Tap *p, uint32_t ch) {
  const float t00 = t[((size_t)p->y0 * w + p->x0) * C + ch], t01 = t[((size_t)p->y0 * w + p->x1) * C + ch];
  const float t10 = t[((size_t)p->y1 * w + p->x0) * C + ch], t11 = t[((size_t)p->y1 * w + p->x1) * C + ch];
  const float top = fmaf(p->tx, t01 - t00, t00), bot = fmaf(p->tx, t11 - t10, t10);
  return fmaf(p->ty, bot - top, top);
}
static int sampled(float u, float v) { return fabsf(u) < INFINITY && fabsf(v) < INFINITY; }

/* tex [H][W][C], mip: its one-frame pyramid (null with L == 1, like uvd); out: C planes of n_px */
void mr_forward(const float *tex, const float *mip, int W, int H, uint32_t C, int mode, uint32_t L, uint32_t n_tris, size_t n_px,
                const uint32_t *id, const float *u, const float *v, const float *uvd, int fused, float *out) {
  for (size_t p = 0; p < n_px; ++p) {
    if (!owned(id[p], n_tris)) {
      if (fused)
        for (uint32_t ch = 0; ch < C; ++ch) out[ch * n_px + p] = 0.0f;
      continue;
    }
    if (!sampled(u[p], v[p])) {
      for (uint32_t ch = 0; ch < C; ++ch) out[ch * n_px + p] = 0.0f;
      continue;
    }
    uint32_t l0 = 0;
    float f = 0.0f;
    if (L > 1) lod(uvd[p], uvd[n_px + p], uvd[2 * n_px + p], uvd[3 * n_px + p], W, H, L, &l0, &f);
    int w0, h0, w1, h1;
    float k;
    Tap t0, t1;
    mr_level(W, H, l0, &w0, &h0, &k);
    tap_of(u[p], v[p], w0, h0, mode, &t0);
    const float *s0 = level_of(tex, mip, W, H, C, l0), *s1 = 0;
    if (f != 0.0f) {
      mr_level(W, H, l0 + 1, &w1, &h1, &k);
      tap_of(u[p], v[p], w1, h1, mode, &t1);
      s1 = level_of(tex, mip, W, H, C, l0 + 1);
    }
    for (uint32_t ch = 0; ch < C; ++ch) {
      const float c0 = bilinear(s0, w0, C, &t0, ch);
      out[ch * n_px + p] = f != 0.0f ? fmaf(f, bilinear(s1, w1, C, &t1, ch) - c0, c0) : c0;
    }
  }
}

/* one level's share of a pixel's backward: the adds into the level's doubles, du_l and dv_l */
static void level_grad(const float *s, int w, int h, uint32_t C, const Tap *t, float lw, size_t n_px, size_t p, const float *gout, double *g,
                       double *gabs, uint32_t *count, int want_uv, float *du, float *dv) {
  const size_t at[4] = {(size_t)t->y0 * w + t->x0, (size_t)t->y0 * w + t->x1, (size_t)t->y1 * w + t->x0, (size_t)t->y1 * w + t->x1};
  const float wk[4] = {(1.0f - t->tx) * (1.0f - t->ty), t->tx * (1.0f - t->ty), (1.0f - t->tx) * t->ty, t->tx * t->ty};
  for (int k = 0; k < 4; ++k) {
    if (count) count[at[k]] += 1u;
    const float wl = wk[k] * lw;
    for (uint32_t ch = 0; ch < C; ++ch) {
      const float prod = wl * gout[ch * n_px + p]; /* the float32 product the pass adds */
      if (g) g[at[k] * C + ch] += (double)prod;
      if (gabs) gabs[at[k] * C + ch] += fabs((double)prod);
    }
  }
  if (want_uv) {
    float au = 0.0f, av = 0.0f;
    for (uint32_t ch = 0; ch < C; ++ch) {
      const float gg = gout[ch * n_px + p];
      const float t00 = s[at[0] * C + ch], t01 = s[at[1] * C + ch], t10 = s[at[2] * C + ch], t11 = s[at[3] * C + ch];
      const float top = fmaf(t->tx, t01 - t00, t00), bot = fmaf(t->tx, t11 - t10, t10);
      au = fmaf(gg, fmaf(t->ty, (t11 - t10) - (t01 - t00), t01 - t00), au);
      av = fmaf(gg, bot - top, av);
    }
    *du = t->in_x ? au * (float)w : 0.0f;
    *dv = t->in_y ? av * (float)h : 0.0f;
  }
}

/* g, gabs: doubles of one frame's WHOLE pyramid, level 0 first ([H][W][C], then mip's layout), added into; count: per texel of the
 * whole pyramid likewise (any of the three may be null).  guv: 2 planes of n_px (null: not wanted; needs tex and mip). */
void mr_grad(const float *tex, const float *mip, int W, int H, uint32_t C, int mode, uint32_t L, uint32_t n_tris, size_t n_px,
             const uint32_t *id, const float *u, const float *v, const float *uvd, const float *gout, int fused, double *g, double *gabs,
             uint32_t *count, float *guv) {
  const size_t lvl0 = (size_t)W * H;
  for (size_t p = 0; p < n_px; ++p) {
    if (!owned(id[p], n_tris)) {
      if (fused && guv) guv[p] = 0.0f, guv[n_px + p] = 0.0f;
      continue;
    }
    if (!sampled(u[p], v[p])) {
      if (guv) guv[p] = 0.0f, guv[n_px + p] = 0.0f;
      continue;
    }
    uint32_t l0 = 0;
    float f = 0.0f;
    if (L > 1) lod(uvd[p], uvd[n_px + p], uvd[2 * n_px + p], uvd[3 * n_px + p], W, H, L, &l0, &f);
    float du[2] = {0, 0}, dv[2] = {0, 0};
    for (uint32_t j = 0; j < (f != 0.0f ? 2u : 1u); ++j) {
      const uint32_t l = l0 + j;
      int w, h;
      float k;
      Tap t;
      mr_level(W, H, l, &w, &h, &k);
      tap_of(u[p], v[p], w, h, mode, &t);
      const size_t texel_off = l == 0 ? 0 : lvl0 + level_off(W, H, 1, l);
      level_grad(guv ? level_of(tex, mip, W, H, C, l) : 0, w, h, C, &t, j == 0 ? 1.0f - f : f, n_px, p, gout, g ? g + texel_off * C : 0,
                 gabs ? gabs + texel_off * C : 0, count ? count + texel_off : 0, guv != 0, &du[j], &dv[j]);
    }
    if (guv) {
      guv[p] = f != 0.0f ? fmaf(f, du[1] - du[0], du[0]) : du[0];
      guv[n_px + p] = f != 0.0f ? fmaf(f, dv[1] - dv[0], dv[0]) : dv[0];
    }
  }
}
