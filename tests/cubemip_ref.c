/* The mipmapped cube lookup's test reference (tests/cubemipref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math, once as
 * binary32 — `real` is float: the arithmetic the library is held to, bit for bit — and once with -DCMR_DOUBLE — `real` is double: the
 * same text as a binary64 function, for the comparisons against float64 autograd and central differences).  It includes
 * tests/cube_ref.c unchanged for the faces' axes, the 24-row seam table and cr_resolve, and nothing of the library.  Per pixel of a
 * visibility buffer (owner id word) with its direction and its level of detail lam, a cube's mip pyramid — one frame's levels
 * 0 .. L - 1 one after another, level l [6][N >> l][N >> l][n_ch] — sampled by the rule include/srz.h states for
 * srz_frameset_texture_cube_mip, restated here:
 *   unsampled, the face, ma, s = sc / ma, t = tc / ma: the flat lookup's (cube_ref.c), independent of the level
 *   the level:  !(lam > 0) -> l0 = 0, f = 0;  lam >= L - 1 -> l0 = L - 1, f = 0;  else lf = floor(lam), l0 = (int)lf, f = lam - lf
 *   c_l: the flat lookup's sample of level l — per axis u = fma(s, 0.5, 0.5); fx = u * N_l - 0.5; x0 = floor(fx), tx = fx - x0; the
 *     corners resolved by the seam table with N = N_l;  top = fma(tx, t01 - t00, t00);  bot = fma(tx, t11 - t10, t10);
 *     c = fma(ty, bot - top, top)
 *   out = c_l0 when f == 0, else fma(f, c_(l0+1) - c_l0, c_l0)
 * and its backward: the texel adds (w_rc * lw) * gout in DOUBLE sums with the count of contributing adds per texel and the sum of
 * |product| per element; gdir = gdir_l0 or fma(f, gdir_(l0+1) - gdir_l0, gdir_l0) per component, gdir_l the flat backward at level l;
 * glam = the fma chain of gout[ch] over c_(l0+1)[ch] - c_l0[ch] where 0 <= lam < L - 1, else 0; and srz_frameset_cube_level's
 * level from the derivative planes of the direction. */
#include "cube_ref.c"

#ifdef CMR_DOUBLE
typedef double real;
#define R_FMA fma
#define R_FLOOR floor
#define R_FABS fabs
#define R_SQRT sqrt
#define R_FREXP frexp
#define R_FMAX fmax
#else
typedef float real;
#define R_FMA fmaf
#define R_FLOOR floorf
#define R_FABS fabsf
#define R_SQRT sqrtf
#define R_FREXP frexpf
#define R_FMAX fmaxf
#endif
#define R(x) ((real)(x))

int cmr_real_bytes(void) { return (int)sizeof(real); }

typedef struct {
  int face, major_pos;
  real s, t, ma;
} CmFace;
typedef struct {
  real tx, ty;
  size_t at[4]; /* resolved texels (face * N + y) * N + x of the corners (y0, x0), (y0, x1), (y1, x0), (y1, x1), within the level */
  int crossed;  /* a corner went to another face */
} CmCorners;

static int cm_finite(real c) { return R_FABS(c) < (real)INFINITY; }

/* 0: the direction is not sampled */
static int cm_face(const real d[3], CmFace *p) {
  if (!cm_finite(d[0]) || !cm_finite(d[1]) || !cm_finite(d[2])) return 0;
  const real ax = R_FABS(d[0]), ay = R_FABS(d[1]), az = R_FABS(d[2]);
  if (R_FMAX(ax, R_FMAX(ay, az)) == R(0)) return 0;
  const int m = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
  const int f = 2 * m + (d[m] > R(0) ? 0 : 1);
  p->ma = R_FABS(d[m]), p->major_pos = d[m] > R(0);
  const real sc = SU_SIGN[f] < 0 ? -d[SU_AXIS[f]] : d[SU_AXIS[f]], tc = SV_SIGN[f] < 0 ? -d[SV_AXIS[f]] : d[SV_AXIS[f]];
  p->face = f, p->s = sc / p->ma, p->t = tc / p->ma;
  return 1;
}

static void cm_axis(real s, int N, int *i0, real *t) {
  const real u = R_FMA(s, R(0.5), R(0.5)), fx = u * (real)N - R(0.5);
  const real f0 = R_FLOOR(fx);
  *t = fx - f0;
  *i0 = (int)f0;
  /* (binary64 only: s = +-1 exactly gives fx = N - 0.5 or -0.5 as in binary32; nothing to clamp) */
}

static void cm_corners(const CmFace *c, int N, CmCorners *p) {
  int x0, y0;
  cm_axis(c->s, N, &x0, &p->tx);
  cm_axis(c->t, N, &y0, &p->ty);
  p->crossed = 0;
  for (int k = 0; k < 4; ++k) {
    int r[3];
    cr_resolve(N, c->face, x0 + (k & 1), y0 + (k >> 1), r);
    p->crossed |= r[0] != c->face;
    p->at[k] = ((size_t)r[0] * N + r[2]) * N + r[1];
  }
}

static void cm_lod(real lam, int L, int *l0, real *f) {
  *l0 = 0, *f = R(0);
  if (!(lam > R(0))) return;
  if (lam >= (real)(L - 1)) {
    *l0 = L - 1;
    return;
  }
  const real lf = R_FLOOR(lam);
  *l0 = (int)lf, *f = lam - lf;
}

/* the texels of one frame's levels 0 .. l - 1 */
static size_t cm_before(int N, int l) {
  size_t s = 0;
  for (int k = 0; k < l; ++k) s += (size_t)6 * (N >> k) * (N >> k);
  return s;
}

static real cm_sample(const real *lev, const CmCorners *p, uint32_t n_ch, uint32_t ch, real *du, real *dv) {
  const real t00 = lev[p->at[0] * n_ch + ch], t01 = lev[p->at[1] * n_ch + ch], t10 = lev[p->at[2] * n_ch + ch], t11 = lev[p->at[3] * n_ch + ch];
  const real top = R_FMA(p->tx, t01 - t00, t00), bot = R_FMA(p->tx, t11 - t10, t10);
  if (du) *du = R_FMA(p->ty, (t11 - t10) - (t01 - t00), t01 - t00), *dv = bot - top;
  return R_FMA(p->ty, bot - top, top);
}

/* the flat backward's chain from au, av at a level of N x N faces to the direction */
static void cm_gdir(const CmFace *c, real au, real av, int N, real g3[3]) {
  const real gs = au * (R(0.5) * (real)N), gt = av * (R(0.5) * (real)N), inv = R(1) / c->ma;
  const real g_sc = gs * inv, g_tc = gt * inv, g_ma = -(R_FMA(gs, c->s, gt * c->t) * inv);
  const int f = c->face;
  g3[0] = g3[1] = g3[2] = R(0);
  g3[SU_AXIS[f]] = SU_SIGN[f] < 0 ? -g_sc : g_sc;
  g3[SV_AXIS[f]] = SV_SIGN[f] < 0 ? -g_tc : g_tc;
  g3[f / 2] = c->major_pos ? g_ma : -g_ma;
}

/* per pixel: bit 0 owned, bit 1 sampled, bit 2 the clamp !(lam > 0), bit 3 the clamp lam >= L - 1, bit 4 0 < f < 1, bit 5 a corner
 * of a level above 0 that the lookup reads went to another face; face: the face of a sampled pixel, else 255; l0 and f of a sampled
 * pixel.  lam may be null at L == 1 */
void cmr_classify(int N, int L, uint32_t n_tris, size_t n_px, const uint32_t *id, const real *dx, const real *dy, const real *dz, const real *lam,
                  uint8_t *cls, uint8_t *face, int32_t *l0s, real *fs) {
  for (size_t p = 0; p < n_px; ++p) {
    CmFace c;
    const real d[3] = {dx[p], dy[p], dz[p]};
    cls[p] = 0, face[p] = 255, l0s[p] = 0, fs[p] = R(0);
    if (!owned(id[p], n_tris)) continue;
    cls[p] = 1;
    if (!cm_face(d, &c)) continue;
    const real la = L > 1 ? lam[p] : R(0);
    int l0;
    real f;
    cm_lod(la, L, &l0, &f);
    cls[p] |= 2 | (!(la > R(0)) ? 4 : 0) | ((la > R(0)) && la >= (real)(L - 1) ? 8 : 0) | (f > R(0) && f < R(1) ? 16 : 0);
    for (int l = l0 > 0 ? l0 : 1; l <= l0 + (f != R(0) ? 1 : 0); ++l) {
      CmCorners k;
      cm_corners(&c, N >> l, &k);
      if (k.crossed) cls[p] |= 32;
    }
    face[p] = (uint8_t)c.face, l0s[p] = l0, fs[p] = f;
  }
}

/* pyr: one frame's levels 0 .. L - 1; id: plane 1 of the frame's visibility buffer; dx, dy, dz, lam: planes of n_px words (lam may
 * be null at L == 1); out: n_ch planes of n_px.  A pixel nobody owns: 0 when fused, else its words stay. */
void cmr_forward(const real *pyr, int N, int L, uint32_t n_ch, uint32_t n_tris, size_t n_px, const uint32_t *id, const real *dx, const real *dy,
                 const real *dz, const real *lam, int fused, real *out) {
  for (size_t p = 0; p < n_px; ++p) {
    CmFace c;
    const real d[3] = {dx[p], dy[p], dz[p]};
    if (!owned(id[p], n_tris)) {
      if (fused)
        for (uint32_t ch = 0; ch < n_ch; ++ch) out[ch * n_px + p] = R(0);
      continue;
    }
    if (!cm_face(d, &c)) {
      for (uint32_t ch = 0; ch < n_ch; ++ch) out[ch * n_px + p] = R(0);
      continue;
    }
    int l0;
    real f;
    cm_lod(L > 1 ? lam[p] : R(0), L, &l0, &f);
    CmCorners k0, k1;
    cm_corners(&c, N >> l0, &k0);
    if (f != R(0)) cm_corners(&c, N >> (l0 + 1), &k1);
    for (uint32_t ch = 0; ch < n_ch; ++ch) {
      const real c0 = cm_sample(pyr + cm_before(N, l0) * n_ch, &k0, n_ch, ch, NULL, NULL);
      if (f == R(0)) {
        out[ch * n_px + p] = c0;
      } else {
        const real c1 = cm_sample(pyr + cm_before(N, l0 + 1) * n_ch, &k1, n_ch, ch, NULL, NULL);
        out[ch * n_px + p] = R_FMA(f, c1 - c0, c0);
      }
    }
  }
}

/* gout: n_ch planes of n_px (words at nobody's pixels are never read).  gpyr, gabs: the pyramid's shape in doubles, added into;
 * count: contributing adds per texel of the pyramid, added into (any of the three may be null).  gdir: 3 planes, glam: 1 plane of
 * n_px (null: not wanted). */
void cmr_grad(const real *pyr, int N, int L, uint32_t n_ch, uint32_t n_tris, size_t n_px, const uint32_t *id, const real *dx, const real *dy,
              const real *dz, const real *lam, const real *gout, int fused, double *gpyr, double *gabs, uint32_t *count, real *gdir, real *glam) {
  for (size_t p = 0; p < n_px; ++p) {
    CmFace c;
    const real d[3] = {dx[p], dy[p], dz[p]};
    const int own = owned(id[p], n_tris);
    if (!own || !cm_face(d, &c)) {
      if (own || fused) {
        if (gdir) gdir[p] = R(0), gdir[n_px + p] = R(0), gdir[2 * n_px + p] = R(0);
        if (glam) glam[p] = R(0);
      }
      continue;
    }
    const real la = L > 1 ? lam[p] : R(0);
    int l0;
    real f;
    cm_lod(la, L, &l0, &f);
    const int rhd = la >= R(0) && la < (real)(L - 1); /* level l0 + 1 exists: the right-hand derivative */
    CmCorners k[2];
    cm_corners(&c, N >> l0, &k[0]);
    if (f != R(0) || rhd) cm_corners(&c, N >> (l0 + 1), &k[1]);
    for (int e = 0; e < (f != R(0) ? 2 : 1); ++e) {
      const real lw = e == 0 ? R(1) - f : f, tx = k[e].tx, ty = k[e].ty;
      const real wk[4] = {((R(1) - tx) * (R(1) - ty)) * lw, (tx * (R(1) - ty)) * lw, ((R(1) - tx) * ty) * lw, (tx * ty) * lw};
      const size_t base = cm_before(N, l0 + e);
      for (int q = 0; q < 4; ++q) {
        if (count) count[base + k[e].at[q]] += 1u;
        for (uint32_t ch = 0; ch < n_ch; ++ch) {
          const real prod = wk[q] * gout[ch * n_px + p]; /* the product the pass adds */
          if (gpyr) gpyr[(base + k[e].at[q]) * n_ch + ch] += (double)prod;
          if (gabs) gabs[(base + k[e].at[q]) * n_ch + ch] += fabs((double)prod);
        }
      }
    }
    if (gdir || glam) {
      real au[2] = {R(0), R(0)}, av[2] = {R(0), R(0)}, gl = R(0);
      for (uint32_t ch = 0; ch < n_ch; ++ch) {
        const real g = gout[ch * n_px + p];
        real cs[2] = {R(0), R(0)};
        for (int e = 0; e < (f != R(0) || rhd ? 2 : 1); ++e) {
          real du, dv;
          cs[e] = cm_sample(pyr + cm_before(N, l0 + e) * n_ch, &k[e], n_ch, ch, &du, &dv);
          au[e] = R_FMA(g, du, au[e]), av[e] = R_FMA(g, dv, av[e]);
        }
        if (rhd) gl = R_FMA(g, cs[1] - cs[0], gl);
      }
      if (gdir) {
        real g0[3], g1[3];
        cm_gdir(&c, au[0], av[0], N >> l0, g0);
        if (f != R(0)) {
          cm_gdir(&c, au[1], av[1], N >> (l0 + 1), g1);
          for (int i = 0; i < 3; ++i) g0[i] = R_FMA(f, g1[i] - g0[i], g0[i]);
        }
        gdir[p] = g0[0], gdir[n_px + p] = g0[1], gdir[2 * n_px + p] = g0[2];
      }
      if (glam) glam[p] = rhd ? gl : R(0);
    }
  }
}

/* srz_frameset_cube_level: dd: the six derivative planes of the direction (plane 2 c: d/dx, plane 2 c + 1: d/dy of component c) ->
 * out: one plane, lam = (real)l0 + f.  l0f (may be null): [n_px][2], l0 and f in front of that sum */
void cmr_level(int N, int L, uint32_t n_tris, size_t n_px, const uint32_t *id, const real *dx, const real *dy, const real *dz, const real *dd,
               int fused, real *out, real *l0f) {
  for (size_t p = 0; p < n_px; ++p) {
    CmFace c;
    const real d[3] = {dx[p], dy[p], dz[p]};
    if (!owned(id[p], n_tris)) {
      if (fused) out[p] = R(0);
      continue;
    }
    out[p] = R(0);
    if (l0f) l0f[2 * p] = l0f[2 * p + 1] = R(0);
    if (!cm_face(d, &c)) continue;
    const int fc = c.face;
    const real inv = R(1) / c.ma;
    real ds[2], dt[2];
    for (int e = 0; e < 2; ++e) { /* the x step, the y step */
      const real v[3] = {dd[(0 + e) * n_px + p], dd[(2 + e) * n_px + p], dd[(4 + e) * n_px + p]};
      const real dsc = SU_SIGN[fc] < 0 ? -v[SU_AXIS[fc]] : v[SU_AXIS[fc]], dtc = SV_SIGN[fc] < 0 ? -v[SV_AXIS[fc]] : v[SV_AXIS[fc]];
      const real dma = c.major_pos ? v[fc / 2] : -v[fc / 2];
      ds[e] = (dsc - c.s * dma) * inv, dt[e] = (dtc - c.t * dma) * inv;
    }
    const real half = R(0.5) * (real)N;
    const real ax = ds[0] * half, ay = dt[0] * half, bx = ds[1] * half, by = dt[1] * half;
    const int fin = cm_finite(ds[0]) && cm_finite(dt[0]) && cm_finite(ds[1]) && cm_finite(dt[1]);
    const real rx = R_FMA(ax, ax, ay * ay), ry = R_FMA(bx, bx, by * by), r2 = rx > ry ? rx : ry;
    int l0 = L - 1;
    real f = R(0);
    if (fin && r2 < (real)INFINITY) {
      const real rho = R_SQRT(r2);
      if (!(rho > R(1))) {
        l0 = 0;
      } else {
        int e;
        const real m = R_FREXP(rho, &e);
        if (e - 1 < L - 1) l0 = e - 1, f = R_FMA(R(2), m, R(-1));
      }
    }
    out[p] = (real)l0 + f;
    if (l0f) l0f[2 * p] = (real)l0, l0f[2 * p + 1] = f;
  }
}
