/* The mesh Laplacian: the test reference of srz_mesh_laplacian and srz_mesh_laplacian_grad (tests/lapref.py builds it with gcc -O2
 * -ffp-contract=off -fno-fast-math).  It includes nothing of the library; the corner lists come from tests/normalsref.py's.  BOTH
 * RULES ARE STATED ONCE, in a type `real`: this file includes itself twice, as binary32 (lr_apply_f32, lr_apply_t_f32: the bits the
 * device must give) and as binary64 (lr_apply_f64, lr_apply_t_f64: what tests/lapref.py's derived rounding bounds are held against).
 * THE RULES, nothing fused, in this order, the channels j independent:
 *   cross(u, w) = (u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x);   dot3(a, b) = (a.x b.x + a.y b.y) + a.z b.z
 *   per vertex v, list(v) its corners 3 * face + k in increasing order;  per corner c:  (i0, i1, i2) = faces[c / 3], k = c % 3,
 *   a = i[(k + 1) % 3], b = i[(k + 2) % 3];  n_v = (real)(2 * |list(v)|)
 *   UMBRELLA:  S = +0;  S = S + (x[a] + x[b]) per corner;   n_v > 0: out[v] = x[v] - S / n_v;  otherwise out[v] = +0
 *   GRAPH:     S as above;  out[v] = n_v * x[v] - S
 *   COTAN:     p = wpos, in the face's own order:  N = cross(p[i1] - p[i0], p[i2] - p[i0]);  d2 = dot3(N, N);
 *              ok = d2 > 0 && d2 <= MAX;  ia = 1 / sqrt(d2);  cot_m = dot3(p[i_(m+1)] - p[i_m], p[i_(m+2)] - p[i_m]) * ia
 *              acc = +0;  per corner whose face is ok:  acc = acc + (cot_b * (x[v] - x[a]) + cot_a * (x[v] - x[b]));  out[v] = 0.5 * acc
 *   THE TRANSPOSE:  GRAPH, COTAN: the rule itself over gout.
 *              UMBRELLA:  T = +0;  T = T + (gout[a] / n_a + gout[b] / n_b) per corner;  gx[v] = (n_v > 0 ? gout[v] : +0) - T */
#ifndef LAP_REF_BODY
#define LAP_REF_BODY
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

enum { UMBRELLA = 0, GRAPH = 1, COTAN = 2 };

#define real float
#define FN(name) name##_f32
#define REAL_MAX FLT_MAX
#define SQRT sqrtf
#include "lap_ref.c"
#undef real
#undef FN
#undef REAL_MAX
#undef SQRT

#define real double
#define FN(name) name##_f64
#define REAL_MAX DBL_MAX
#define SQRT sqrt
#include "lap_ref.c"

#else

typedef struct {
  real x, y, z;
} FN(v3);
static FN(v3) FN(ld)(const real *p) { return (FN(v3)){p[0], p[1], p[2]}; }
static FN(v3) FN(sub)(FN(v3) a, FN(v3) b) { return (FN(v3)){a.x - b.x, a.y - b.y, a.z - b.z}; }
static FN(v3) FN(cross)(FN(v3) u, FN(v3) w) {
  const real x0 = u.y * w.z, x1 = u.z * w.y, y0 = u.z * w.x, y1 = u.x * w.z, z0 = u.x * w.y, z1 = u.y * w.x;
  return (FN(v3)){x0 - x1, y0 - y1, z0 - z1};
}
static real FN(dot3)(FN(v3) a, FN(v3) b) {
  const real tx = a.x * b.x, ty = a.y * b.y, tz = a.z * b.z;
  return (tx + ty) + tz;
}

/* the three cotangents of face (i0, i1, i2) in its own order -> 1 if the face is ok */
static int FN(face_cot)(const real *wpos, uint32_t stride, const uint32_t *i, real cot[3]) {
  const FN(v3) p[3] = {FN(ld)(wpos + (size_t)i[0] * stride), FN(ld)(wpos + (size_t)i[1] * stride), FN(ld)(wpos + (size_t)i[2] * stride)};
  const FN(v3) N = FN(cross)(FN(sub)(p[1], p[0]), FN(sub)(p[2], p[0]));
  const real d2 = FN(dot3)(N, N);
  if (!(d2 > (real)0 && d2 <= REAL_MAX)) return 0;
  const real ia = (real)1 / SQRT(d2);
  for (int m = 0; m < 3; ++m) {
    const real d = FN(dot3)(FN(sub)(p[(m + 1) % 3], p[m]), FN(sub)(p[(m + 2) % 3], p[m]));
    cot[m] = d * ia;
  }
  return 1;
}

/* one field: x [n_verts] records of x_stride reals, n_ch read each -> out, records of out_stride reals, n_ch written each;
 * transpose != 0: UMBRELLA's transposed rule (the other kinds are their own transpose) */
static void FN(apply)(const real *x, uint32_t x_stride, uint32_t n_ch, uint32_t n_verts, const uint32_t *faces, const uint32_t *off,
                      const uint32_t *corners, int kind, int transpose, const real *wpos, uint32_t wpos_stride, real *out, uint32_t out_stride) {
  for (uint32_t v = 0; v < n_verts; ++v) {
    const real n_v = (real)(2u * (off[v + 1u] - off[v]));
    for (uint32_t j = 0; j < n_ch; ++j) {
      const real xv = x[(size_t)v * x_stride + j];
      real S = (real)0;
      for (uint32_t c = off[v]; c < off[v + 1u]; ++c) {
        const uint32_t *i = faces + (size_t)(corners[c] / 3u) * 3u, k = corners[c] % 3u;
        const uint32_t a = i[(k + 1u) % 3u], b = i[(k + 2u) % 3u];
        if (kind == COTAN) {
          real cot[3];
          if (!FN(face_cot)(wpos, wpos_stride, i, cot)) continue;
          const real da = xv - x[(size_t)a * x_stride + j], db = xv - x[(size_t)b * x_stride + j];
          const real ta = cot[(k + 2u) % 3u] * da, tb = cot[(k + 1u) % 3u] * db;
          const real t = ta + tb;
          S = S + t;
        } else if (transpose && kind == UMBRELLA) {
          const real n_a = (real)(2u * (off[a + 1u] - off[a])), n_b = (real)(2u * (off[b + 1u] - off[b]));
          const real qa = x[(size_t)a * x_stride + j] / n_a, qb = x[(size_t)b * x_stride + j] / n_b;
          const real t = qa + qb;
          S = S + t;
        } else {
          const real t = x[(size_t)a * x_stride + j] + x[(size_t)b * x_stride + j];
          S = S + t;
        }
      }
      real r;
      if (kind == COTAN) r = (real)0.5 * S;
      else if (kind == GRAPH) {
        const real nx = n_v * xv;
        r = nx - S;
      } else if (transpose) r = (n_v > (real)0 ? xv : (real)0) - S;
      else if (n_v > (real)0) {
        const real q = S / n_v;
        r = xv - q;
      } else r = (real)0;
      out[(size_t)v * out_stride + j] = r;
    }
  }
}

void FN(lr_apply)(const real *x, uint32_t x_stride, uint32_t n_ch, uint32_t n_verts, const uint32_t *faces, const uint32_t *off,
                  const uint32_t *corners, int kind, const real *wpos, uint32_t wpos_stride, real *out, uint32_t out_stride) {
  FN(apply)(x, x_stride, n_ch, n_verts, faces, off, corners, kind, 0, wpos, wpos_stride, out, out_stride);
}
void FN(lr_apply_t)(const real *gout, uint32_t gout_stride, uint32_t n_ch, uint32_t n_verts, const uint32_t *faces, const uint32_t *off,
                    const uint32_t *corners, int kind, const real *wpos, uint32_t wpos_stride, real *gx, uint32_t gx_stride) {
  FN(apply)(gout, gout_stride, n_ch, n_verts, faces, off, corners, kind, 1, wpos, wpos_stride, gx, gx_stride);
}

#endif
