/* The cube lookup's test reference (tests/cuberef.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math; no flush to zero: a
 * subnormal is a number, as in the library's build).  It includes nothing of the library: per pixel of a visibility buffer (owner id
 * word) with its direction (dx, dy, dz), a float cube map [face][row][column][channel] of N x N faces sampled bilinearly and
 * seamlessly by the rule include/srz.h states for srz_frameset_texture_cube, restated here —
 *   unsampled: a component not finite, or max(|dx|, |dy|, |dz|) == 0 -> out 0, gdir (0, 0, 0), no add
 *   major axis: x if ax >= ay && ax >= az; else y if ay >= az; else z;  face = 2 * axis + (component > 0 ? 0 : 1)
 *   ma = fabsf(major component);  sc, tc = the signed components the face's su, sv name;  s = sc / ma;  t = tc / ma
 *   per axis (x with s, y with t):  u = fmaf(s, 0.5f, 0.5f);  fx = u * (float)N - 0.5f;  x0f = floorf(fx), tx = fx - x0f, x0 = (int)x0f,
 *     x1 = x0 + 1;  a corner with x or y in {-1, N} is RESOLVED onto the neighbouring face by the 24-row table below
 *   top = fmaf(tx, t01 - t00, t00);  bot = fmaf(tx, t11 - t10, t10);  out = fmaf(ty, bot - top, top)
 * — fmaf where the rule fuses and nothing else fused; and the backward of that: the gradient with respect to the direction in float
 * (one fmaf per channel and axis, ascending, then the chain through s = sc / ma, t = tc / ma), the gradient with respect to the
 * texels in DOUBLE (the sum of the float32 products w_rc * g), with the count of contributing adds per texel and the sum of
 * |w_rc * g| per element, from which the tests derive their bound.  cr_* entries with `force` >= 0 sample through THAT face instead
 * of the selected one (ma = the component along its normal, which must be positive, and |s|, |t| <= 1: else unsampled). */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

/* face -> the axis of its normal is face / 2, its sign + for even faces; su and sv: axis and sign */
static const int SU_AXIS[6] = {2, 2, 0, 0, 0, 0}, SU_SIGN[6] = {-1, 1, 1, 1, 1, -1};
static const int SV_AXIS[6] = {1, 1, 2, 2, 1, 1}, SV_SIGN[6] = {-1, -1, 1, -1, -1, -1};
/* [face][side: x = -1, x = N, y = -1, y = N] -> {neighbour face, which index of the neighbour is fixed (0: x, 1: y), fixed at
 * N - 1 (else 0), the index along the edge mirrored (N - 1 - i, else i)} */
static const uint8_t SEAM[6][4][4] = {
    {{4, 0, 1, 0}, {5, 0, 0, 0}, {2, 0, 1, 1}, {3, 0, 1, 0}},
    {{5, 0, 1, 0}, {4, 0, 0, 0}, {2, 0, 0, 0}, {3, 0, 0, 1}},
    {{1, 1, 0, 0}, {0, 1, 0, 1}, {5, 1, 0, 1}, {4, 1, 0, 0}},
    {{1, 1, 1, 1}, {0, 1, 1, 0}, {4, 1, 1, 0}, {5, 1, 1, 1}},
    {{1, 0, 1, 0}, {0, 0, 0, 0}, {2, 1, 1, 0}, {3, 1, 0, 0}},
    {{0, 0, 1, 0}, {1, 0, 0, 0}, {2, 1, 0, 1}, {3, 1, 1, 1}}};

typedef struct {
  int face, x0, y0;
  float s, t, ma, tx, ty;
  int major_pos;     /* the major component is positive */
  size_t at[4];      /* resolved texels (face * N + y) * N + x of the corners (y0, x0), (y0, x1), (y1, x0), (y1, x1) */
  int crossed, both; /* a corner went to another face; a corner lay outside in both axes */
} Tap;

/* texel (x, y) of face f, x and y in [-1, N] -> out3 = {face, x, y} resolved; returns 1 when the texel lay outside in both axes */
int cr_resolve(int N, int f, int x, int y, int *out3) {
  int both = 0;
  if ((x < 0 || x >= N) && (y < 0 || y >= N)) both = 1, y = y < 0 ? 0 : N - 1;
  int side = -1, along = 0;
  if (x < 0) side = 0, along = y;
  else if (x >= N) side = 1, along = y;
  else if (y < 0) side = 2, along = x;
  else if (y >= N) side = 3, along = x;
  if (side < 0) {
    out3[0] = f, out3[1] = x, out3[2] = y;
    return 0;
  }
  const uint8_t *r = SEAM[f][side];
  const int a = r[3] ? N - 1 - along : along, e = r[2] ? N - 1 : 0;
  out3[0] = r[0], out3[1] = r[1] == 0 ? e : a, out3[2] = r[1] == 0 ? a : e;
  return both;
}

static void axis(float s, int N, int *i0, float *t) {
  const float u = fmaf(s, 0.5f, 0.5f), fx = u * (float)N - 0.5f;
  const float f0 = floorf(fx);
  *t = fx - f0;
  *i0 = (int)f0;
}

static int finite_(float c) { return fabsf(c) < INFINITY; }

/* 0: the direction is not sampled */
static int tap_of(const float d[3], int N, int force, Tap *p) {
  if (!finite_(d[0]) || !finite_(d[1]) || !finite_(d[2])) return 0;
  const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
  if (fmaxf(ax, fmaxf(ay, az)) == 0.0f) return 0;
  int f;
  if (force < 0) {
    const int m = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    f = 2 * m + (d[m] > 0.0f ? 0 : 1);
    p->ma = fabsf(d[m]);
    p->major_pos = d[m] > 0.0f;
  } else {
    f = force;
    const float c = (f & 1) ? -d[f / 2] : d[f / 2];
    if (!(c > 0.0f)) return 0;
    p->ma = c;
    p->major_pos = !(f & 1);
  }
  const float sc = SU_SIGN[f] < 0 ? -d[SU_AXIS[f]] : d[SU_AXIS[f]], tc = SV_SIGN[f] < 0 ? -d[SV_AXIS[f]] : d[SV_AXIS[f]];
  p->face = f, p->s = sc / p->ma, p->t = tc / p->ma;
  if (!(fabsf(p->s) <= 1.0f) || !(fabsf(p->t) <= 1.0f)) return 0; /* (a forced face only) */
  axis(p->s, N, &p->x0, &p->tx);
  axis(p->t, N, &p->y0, &p->ty);
  p->crossed = p->both = 0;
  for (int k = 0; k < 4; ++k) {
    int r[3];
    p->both |= cr_resolve(N, f, p->x0 + (k & 1), p->y0 + (k >> 1), r);
    p->crossed |= r[0] != f;
    p->at[k] = ((size_t)r[0] * N + r[2]) * N + r[1];
  }
  return 1;
}

static int owned(uint32_t id, uint32_t n_tris) { return (id & 0x7fffffffu) - 1u < n_tris; }

/* n directions [n][3] -> face (-1: unsampled), st [n][2], x0y0 [n][2], frac [n][2] (tx, ty), at [n][4] (uint32), w [n][4] */
void cr_taps(int N, int force, size_t n, const float *dirs, int32_t *face, float *st, int32_t *x0y0, float *frac, uint32_t *at, float *w) {
  for (size_t i = 0; i < n; ++i) {
    Tap t;
    face[i] = -1;
    if (!tap_of(dirs + 3 * i, N, force, &t)) continue;
    face[i] = t.face, st[2 * i] = t.s, st[2 * i + 1] = t.t, x0y0[2 * i] = t.x0, x0y0[2 * i + 1] = t.y0;
    frac[2 * i] = t.tx, frac[2 * i + 1] = t.ty;
    const float wk[4] = {(1.0f - t.tx) * (1.0f - t.ty), t.tx * (1.0f - t.ty), (1.0f - t.tx) * t.ty, t.tx * t.ty};
    for (int k = 0; k < 4; ++k) at[4 * i + k] = (uint32_t)t.at[k], w[4 * i + k] = wk[k];
  }
}

/* per pixel: bit 0 owned, bit 1 sampled, bit 2 (sampled) a corner on another face, bit 3 (sampled) a corner outside in both axes;
 * face: the face of a sampled pixel, else 255 */
void cr_classify(int N, uint32_t n_tris, size_t n_px, const uint32_t *id, const float *dx, const float *dy, const float *dz, uint8_t *cls,
                 uint8_t *face) {
  for (size_t p = 0; p < n_px; ++p) {
    Tap t;
    const float d[3] = {dx[p], dy[p], dz[p]};
    cls[p] = 0, face[p] = 255;
    if (!owned(id[p], n_tris)) continue;
    cls[p] = 1;
    if (!tap_of(d, N, -1, &t)) continue;
    cls[p] |= 2 | (t.crossed ? 4 : 0) | (t.both ? 8 : 0);
    face[p] = (uint8_t)t.face;
  }
}

/* tex: [6][N][N][n_ch]; id: plane 1 of the frame's visibility buffer; dx, dy, dz: the three direction planes, n_px words each; out:
 * n_ch planes of n_px.  A pixel nobody owns: 0 when fused, else its words stay. */
void cr_forward(const float *tex, int N, uint32_t n_ch, uint32_t n_tris, size_t n_px, const uint32_t *id, const float *dx, const float *dy,
                const float *dz, int fused, int force, float *out) {
  for (size_t p = 0; p < n_px; ++p) {
    Tap t;
    const float d[3] = {dx[p], dy[p], dz[p]};
    if (!owned(id[p], n_tris)) {
      if (fused)
        for (uint32_t ch = 0; ch < n_ch; ++ch) out[ch * n_px + p] = 0.0f;
      continue;
    }
    if (!tap_of(d, N, force, &t)) {
      for (uint32_t ch = 0; ch < n_ch; ++ch) out[ch * n_px + p] = 0.0f;
      continue;
    }
    for (uint32_t ch = 0; ch < n_ch; ++ch) {
      const float t00 = tex[t.at[0] * n_ch + ch], t01 = tex[t.at[1] * n_ch + ch], t10 = tex[t.at[2] * n_ch + ch], t11 = tex[t.at[3] * n_ch + ch];
      const float top = fmaf(t.tx, t01 - t00, t00), bot = fmaf(t.tx, t11 - t10, t10);
      out[ch * n_px + p] = fmaf(t.ty, bot - top, top);
    }
  }
}

/* gout: n_ch planes of n_px (words at nobody's pixels are never read).  gtex, gabs: [6][N][N][n_ch] doubles, added into; count:
 * [6][N][N] contributing adds per texel, added into (any of the three may be null).  gdir: 3 planes of n_px (null: not wanted; needs
 * tex). */
void cr_grad(const float *tex, int N, uint32_t n_ch, uint32_t n_tris, size_t n_px, const uint32_t *id, const float *dx, const float *dy,
             const float *dz, const float *gout, int fused, int force, double *gtex, double *gabs, uint32_t *count, float *gdir) {
  for (size_t p = 0; p < n_px; ++p) {
    Tap t;
    const float d[3] = {dx[p], dy[p], dz[p]};
    if (!owned(id[p], n_tris)) {
      if (fused && gdir) gdir[p] = 0.0f, gdir[n_px + p] = 0.0f, gdir[2 * n_px + p] = 0.0f;
      continue;
    }
    if (!tap_of(d, N, force, &t)) {
      if (gdir) gdir[p] = 0.0f, gdir[n_px + p] = 0.0f, gdir[2 * n_px + p] = 0.0f;
      continue;
    }
    const float wk[4] = {(1.0f - t.tx) * (1.0f - t.ty), t.tx * (1.0f - t.ty), (1.0f - t.tx) * t.ty, t.tx * t.ty};
    for (int k = 0; k < 4; ++k) {
      if (count) count[t.at[k]] += 1u;
      for (uint32_t ch = 0; ch < n_ch; ++ch) {
        const float prod = wk[k] * gout[ch * n_px + p]; /* the float32 product the pass adds */
        if (gtex) gtex[t.at[k] * n_ch + ch] += (double)prod;
        if (gabs) gabs[t.at[k] * n_ch + ch] += fabs((double)prod);
      }
    }
    if (gdir) {
      float au = 0.0f, av = 0.0f;
      for (uint32_t ch = 0; ch < n_ch; ++ch) {
        const float g = gout[ch * n_px + p];
        const float t00 = tex[t.at[0] * n_ch + ch], t01 = tex[t.at[1] * n_ch + ch], t10 = tex[t.at[2] * n_ch + ch], t11 = tex[t.at[3] * n_ch + ch];
        const float top = fmaf(t.tx, t01 - t00, t00), bot = fmaf(t.tx, t11 - t10, t10);
        au = fmaf(g, fmaf(t.ty, (t11 - t10) - (t01 - t00), t01 - t00), au);
        av = fmaf(g, bot - top, av);
      }
      const float gs = au * (0.5f * (float)N), gt = av * (0.5f * (float)N), inv = 1.0f / t.ma;
      const float g_sc = gs * inv, g_tc = gt * inv, g_ma = -(fmaf(gs, t.s, gt * t.t) * inv);
      const int f = t.face;
      float g3[3] = {0.0f, 0.0f, 0.0f};
      g3[SU_AXIS[f]] = SU_SIGN[f] < 0 ? -g_sc : g_sc;
      g3[SV_AXIS[f]] = SV_SIGN[f] < 0 ? -g_tc : g_tc;
      g3[f / 2] = t.major_pos ? g_ma : -g_ma;
      gdir[p] = g3[0], gdir[n_px + p] = g3[1], gdir[2 * n_px + p] = g3[2];
    }
  }
}
