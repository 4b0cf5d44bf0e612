/* The shadow-map lookup's test reference (tests/shadowref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math; no flush to
 * zero).  It includes nothing of the library.  The rule include/srz.h states for srz_frameset_shadow and the order of operations it
 * fixes for srz_frameset_shadow_grad are written down ONCE, below, in terms of a type `real`; this file includes itself twice, so
 * that the one text exists as binary32 (sr32_*: the rule itself, what the GPU is held to bit for bit) and as binary64 (sr64_*: the
 * same operations carried out in double, what the binary32 build's error is measured against).  Per pixel of a visibility buffer
 * (owner id word) with its coordinates sx, sy, sd, over one map [H][W]:
 *   forward:  the lit fraction;
 *   grad:     the gradient planes gsx, gsy, gsd, and per MOVING corner the term d_rc ACCUMULATED IN DOUBLE into gmap, with the sum of
 *             |term| and the count of adds per texel, from which the tests derive their bound;
 *   taps:     per pixel x0, y0, tx, ty and the four corners' ramp values q (NaN: the corner is outside the map, or the test is hard);
 *   classify: per pixel owned / sampled / a moving corner / a corner outside the map. */
#ifndef SR_BODY
#include <math.h>
#include <stddef.h>
#include <stdint.h>

static int owned(uint32_t id, uint32_t n_tris) { return ((id & 0x7fffffffu) - 1u) < n_tris; }

#define SR_BODY
#define real float
#define SR(name) sr32_##name
#define FMA fmaf
#define FMIN fminf
#define FMAX fmaxf
#define FLOOR floorf
#define FABS fabsf
#include "shadow_ref.c"
#undef real
#undef SR
#undef FMA
#undef FMIN
#undef FMAX
#undef FLOOR
#undef FABS
#define real double
#define SR(name) sr64_##name
#define FMA fma
#define FMIN fmin
#define FMAX fmax
#define FLOOR floor
#define FABS fabs
#include "shadow_ref.c"

#else /* ---------------------------------------------------------------------------------------- the rule, once, in `real` */

typedef struct {
  real v[4], q[4], tx, ty; /* corner r * 2 + c is texel (y0 + r, x0 + c) */
  int x0, y0, in_x, in_y;
  unsigned inside, moving; /* one bit per corner */
} SR(Px);
static int SR(finite)(real s) { return FABS(s) < (real)INFINITY; }
static void SR(axis)(real s, int n, int *i0, real *t, int *in) {
  const real nf = (real)n;
  *in = s > (real)-1 && s < nf;
  const real fx = FMIN(FMAX(s, (real)-1), nf);
  const real f0 = FLOOR(fx);
  *t = fx - f0;
  *i0 = (int)f0;
}
/* 0: not sampled */
static int SR(px)(const real *map, int W, int H, real sx, real sy, real sd, real bias, real width, SR(Px) *p) {
  if (!SR(finite)(sx) || !SR(finite)(sy) || !SR(finite)(sd)) return 0;
  SR(axis)(sx, W, &p->x0, &p->tx, &p->in_x);
  SR(axis)(sy, H, &p->y0, &p->ty, &p->in_y);
  p->inside = p->moving = 0u;
  for (int r = 0; r < 2; ++r)
    for (int c = 0; c < 2; ++c) {
      const int k = r * 2 + c, x = p->x0 + c, y = p->y0 + r;
      real v = 1;
      p->q[k] = (real)NAN;
      if (!(x < 0 || x >= W || y < 0 || y >= H)) {
        const real m = map[(size_t)y * (size_t)W + (size_t)x];
        const real e = (m + bias) - sd;
        p->inside |= 1u << k;
        if (width > 0) {
          const real q = e / width + (real)0.5;
          v = FMIN(FMAX(q, (real)0), (real)1);
          if (q > 0 && q < 1) p->moving |= 1u << k;
          p->q[k] = q;
        } else {
          v = e >= 0 ? (real)1 : (real)0;
        }
      }
      p->v[k] = v;
    }
  return 1;
}

void SR(forward)(const real *map, int W, int H, uint32_t n_tris, size_t n_px, const uint32_t *ids, const real *sx, const real *sy,
                 const real *sd, real bias, real width, int fused, real *out) {
  for (size_t i = 0; i < n_px; ++i) {
    SR(Px) p;
    if (!owned(ids[i], n_tris)) {
      if (fused) out[i] = 0;
      continue;
    }
    if (!SR(px)(map, W, H, sx[i], sy[i], sd[i], bias, width, &p)) {
      out[i] = 1;
      continue;
    }
    const real top = FMA(p.tx, p.v[1] - p.v[0], p.v[0]), bot = FMA(p.tx, p.v[3] - p.v[2], p.v[2]);
    out[i] = FMA(p.ty, bot - top, top);
  }
}

/* gsc: [3][n_px] (gsx, gsy, gsd) or null; gmap / gabs: [H][W] doubles, count: [H][W], all three or none */
void SR(grad)(const real *map, int W, int H, uint32_t n_tris, size_t n_px, const uint32_t *ids, const real *sx, const real *sy, const real *sd,
              const real *gout, real bias, real width, int fused, double *gmap, double *gabs, uint32_t *count, real *gsc) {
  for (size_t i = 0; i < n_px; ++i) {
    SR(Px) p;
    if (!owned(ids[i], n_tris)) {
      if (fused && gsc) gsc[i] = gsc[n_px + i] = gsc[2 * n_px + i] = 0;
      continue;
    }
    if (!SR(px)(map, W, H, sx[i], sy[i], sd[i], bias, width, &p)) {
      if (gsc) gsc[i] = gsc[n_px + i] = gsc[2 * n_px + i] = 0;
      continue;
    }
    const real g = gout[i];
    const real top = FMA(p.tx, p.v[1] - p.v[0], p.v[0]), bot = FMA(p.tx, p.v[3] - p.v[2], p.v[2]);
    const real w[4] = {((real)1 - p.tx) * ((real)1 - p.ty), p.tx * ((real)1 - p.ty), ((real)1 - p.tx) * p.ty, p.tx * p.ty};
    real d[4];
    for (int k = 0; k < 4; ++k) {
      d[k] = (p.moving >> k & 1u) ? (w[k] * g) / width : (real)0;
      if ((p.moving >> k & 1u) && gmap) {
        const size_t at = (size_t)(p.y0 + (k >> 1)) * (size_t)W + (size_t)(p.x0 + (k & 1));
        gmap[at] += (double)d[k], gabs[at] += fabs((double)d[k]), count[at] += 1u;
      }
    }
    if (gsc) {
      gsc[i] = p.in_x ? g * FMA(p.ty, (p.v[3] - p.v[2]) - (p.v[1] - p.v[0]), p.v[1] - p.v[0]) : (real)0;
      gsc[n_px + i] = p.in_y ? g * (bot - top) : (real)0;
      gsc[2 * n_px + i] = -(((d[0] + d[1]) + d[2]) + d[3]);
    }
  }
}

/* xy0: [n_px][2] int32, frac: [n_px][2], q: [n_px][4]; an unsampled pixel: x0 = y0 = INT32_MIN, NaNs */
void SR(taps)(const real *map, int W, int H, size_t n_px, const real *sx, const real *sy, const real *sd, real bias, real width, int32_t *xy0,
              real *frac, real *q) {
  for (size_t i = 0; i < n_px; ++i) {
    SR(Px) p;
    if (!SR(px)(map, W, H, sx[i], sy[i], sd[i], bias, width, &p)) {
      xy0[2 * i] = xy0[2 * i + 1] = INT32_MIN;
      frac[2 * i] = frac[2 * i + 1] = (real)NAN;
      for (int k = 0; k < 4; ++k) q[4 * i + k] = (real)NAN;
      continue;
    }
    xy0[2 * i] = p.x0, xy0[2 * i + 1] = p.y0;
    frac[2 * i] = p.tx, frac[2 * i + 1] = p.ty;
    for (int k = 0; k < 4; ++k) q[4 * i + k] = p.q[k];
  }
}

/* cls: 1 owned | 2 sampled | 4 a moving corner | 8 a corner outside the map */
void SR(classify)(const real *map, int W, int H, uint32_t n_tris, size_t n_px, const uint32_t *ids, const real *sx, const real *sy,
                  const real *sd, real bias, real width, uint8_t *cls) {
  for (size_t i = 0; i < n_px; ++i) {
    SR(Px) p;
    cls[i] = 0;
    if (!owned(ids[i], n_tris)) continue;
    cls[i] = 1;
    if (!SR(px)(map, W, H, sx[i], sy[i], sd[i], bias, width, &p)) continue;
    cls[i] |= 2;
    if (p.moving) cls[i] |= 4;
    if (p.inside != 15u) cls[i] |= 8;
  }
}

#endif
