/* The mesh edge terms: the test reference of srz_mesh_edges and srz_mesh_edges_grad (tests/edgeref.py builds it with gcc -O2
 * -ffp-contract=off -fno-fast-math).  It includes nothing of the library; the corner lists come from tests/normalsref.py's.  THE
 * RULES ARE STATED ONCE, in a type `real`: this file includes itself twice, as binary32 (er_forward_f32, er_backward_f32: the bits the
 * device must give) and as binary64 (er_forward_f64, er_backward_f64: what tests/edgeref.py's derived rounding bounds are held
 * against).  The neighbour walk has no arithmetic and is stated once for both.
 * EDGE j of a face (i0, i1, i2) lies opposite corner j: it joins a_j = i[(j + 1) % 3] and b_j = i[(j + 2) % 3].
 * THE NEIGHBOURS OF (f, j):  w = whichever of a_j, b_j has the shorter corner list, a_j on a tie;  o = the other.  Per corner c of
 *   list(w), in list order, g = c / 3, k = c % 3:  g == f: no entry;  g[(k + 1) % 3] == o: the entry (g, (k + 2) % 3);  else
 *   g[(k + 2) % 3] == o: the entry (g, (k + 1) % 3).  One entry per corner, never two.
 * THE RULES, nothing fused, in this order:
 *   cross(u, w) = (u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x);   dot3(a, b) = (a.x b.x + a.y b.y) + a.z b.z
 *   COUNT:     out[f][j] = (real)(1 + the number of entries)
 *   LENGTH:    d = p[b_j] - p[a_j];  out[f][j] = sqrt(dot3(d, d))
 *   the unit normal of a face, in its own order:  N = cross(p[i1] - p[i0], p[i2] - p[i0]);  d2 = dot3(N, N);
 *              ok = d2 > 0 && d2 <= MAX;  r = 1 / sqrt(d2);  n = N * r
 *   DIHEDRAL:  f not ok: +0.  Otherwise acc = +0;  per entry whose g is ok:  acc = acc + (1 - dot3(n_f, n_g));  out[f][j] = acc
 *   THE BACKWARD, LENGTH, per vertex v:  acc = 0;  per corner (f, k) of list(v):  j1 = (k + 1) % 3, j2 = (k + 2) % 3;  for an edge j
 *              len_j = sqrt(dot3(d_j, d_j)), live when len_j > 0 && len_j <= MAX, u_j = d_j * (1 / len_j);
 *              j1 live: acc = acc + gout[f][j1] * u_j1;  then j2 live: acc = acc - gout[f][j2] * u_j2;   gpos[v] = acc
 *   DIHEDRAL, phase 1, per face f:  not ok: gN[f] = 0.  Otherwise H = 0;  for j = 0, 1, 2, per entry (g, j') whose g is ok:
 *              s = w[f][j] + w[g][j'];  H = H - n_g * s;   then t = dot3(n_f, H);  gN[f] = (H - n_f * t) * r_f
 *   phase 2, per vertex v:  acc = 0;  per corner (f, k) of list(v):  a, b, c = p[i0], p[i1], p[i2];  G = gN[f];
 *              k == 0: acc = acc + cross(b - c, G);  k == 1: acc = acc + cross(c - a, G);  k == 2: acc = acc + cross(G, b - a) */
#ifndef EDGE_REF_BODY
#define EDGE_REF_BODY
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

enum { COUNT = 0, LENGTH = 1, DIHEDRAL = 2 };

/* the walk over the neighbours of (f, j) */
typedef struct {
  uint32_t c, end, f, o;
} walk_t;
static walk_t walk_begin(const uint32_t *faces, const uint32_t *off, uint32_t f, uint32_t j) {
  const uint32_t a = faces[(size_t)f * 3u + (j + 1u) % 3u], b = faces[(size_t)f * 3u + (j + 2u) % 3u];
  const int walk_b = off[b + 1u] - off[b] < off[a + 1u] - off[a];
  const uint32_t w = walk_b ? b : a;
  return (walk_t){off[w], off[w + 1u], f, walk_b ? a : b};
}
/* the next entry -> 1 with (*g, *jp), or 0 at the list's end */
static int walk_next(walk_t *w, const uint32_t *faces, const uint32_t *corners, uint32_t *g, uint32_t *jp) {
  while (w->c < w->end) {
    const uint32_t corner = corners[w->c++], face = corner / 3u, k = corner % 3u;
    const uint32_t *i = faces + (size_t)face * 3u;
    if (face == w->f) continue;
    if (i[(k + 1u) % 3u] == w->o) {
      *g = face, *jp = (k + 2u) % 3u;
      return 1;
    }
    if (i[(k + 2u) % 3u] == w->o) {
      *g = face, *jp = (k + 1u) % 3u;
      return 1;
    }
  }
  return 0;
}

/* the entries of (f, j), the first `cap` of them into g_out / j_out -> how many there are */
uint32_t er_entries(const uint32_t *faces, const uint32_t *off, const uint32_t *corners, uint32_t f, uint32_t j, uint32_t *g_out,
                    uint32_t *j_out, uint32_t cap) {
  walk_t w = walk_begin(faces, off, f, j);
  uint32_t n = 0, g, jp;
  while (walk_next(&w, faces, corners, &g, &jp)) {
    if (n < cap) g_out[n] = g, j_out[n] = jp;
    ++n;
  }
  return n;
}

#define real float
#define FN(name) name##_f32
#define REAL_MAX FLT_MAX
#define SQRT sqrtf
#include "edge_ref.c"
#undef real
#undef FN
#undef REAL_MAX
#undef SQRT

#define real double
#define FN(name) name##_f64
#define REAL_MAX DBL_MAX
#define SQRT sqrt
#include "edge_ref.c"

#else

typedef struct {
  real x, y, z;
} FN(v3);
static FN(v3) FN(ld)(const real *p) { return (FN(v3)){p[0], p[1], p[2]}; }
static FN(v3) FN(sub)(FN(v3) a, FN(v3) b) { return (FN(v3)){a.x - b.x, a.y - b.y, a.z - b.z}; }
static FN(v3) FN(add)(FN(v3) a, FN(v3) b) { return (FN(v3)){a.x + b.x, a.y + b.y, a.z + b.z}; }
static FN(v3) FN(cross)(FN(v3) u, FN(v3) w) {
  const real x0 = u.y * w.z, x1 = u.z * w.y, y0 = u.z * w.x, y1 = u.x * w.z, z0 = u.x * w.y, z1 = u.y * w.x;
  return (FN(v3)){x0 - x1, y0 - y1, z0 - z1};
}
static real FN(dot3)(FN(v3) a, FN(v3) b) {
  const real tx = a.x * b.x, ty = a.y * b.y, tz = a.z * b.z;
  return (tx + ty) + tz;
}

/* the unit normal of face i = (i0, i1, i2) in its own order, *r = 1 / |N| -> 1 if the face is ok */
static int FN(unit_normal)(const real *pos, uint32_t stride, const uint32_t *i, FN(v3) *n, real *r) {
  const FN(v3) p0 = FN(ld)(pos + (size_t)i[0] * stride);
  const FN(v3) N = FN(cross)(FN(sub)(FN(ld)(pos + (size_t)i[1] * stride), p0), FN(sub)(FN(ld)(pos + (size_t)i[2] * stride), p0));
  const real d2 = FN(dot3)(N, N);
  if (!(d2 > (real)0 && d2 <= REAL_MAX)) return 0;
  *r = (real)1 / SQRT(d2);
  *n = (FN(v3)){N.x * *r, N.y * *r, N.z * *r};
  return 1;
}

/* one position set -> out, records of out_stride reals, three written per face */
void FN(er_forward)(const real *pos, uint32_t pos_stride, uint32_t n_faces, const uint32_t *faces, const uint32_t *off, const uint32_t *corners,
                    int kind, real *out, uint32_t out_stride) {
  for (uint32_t f = 0; f < n_faces; ++f) {
    const uint32_t *i = faces + (size_t)f * 3u;
    FN(v3) nf;
    real rf;
    const int ok = kind == DIHEDRAL ? FN(unit_normal)(pos, pos_stride, i, &nf, &rf) : 1;
    for (uint32_t j = 0; j < 3u; ++j) {
      real r = (real)0;
      if (kind == LENGTH) {
        const FN(v3) d = FN(sub)(FN(ld)(pos + (size_t)i[(j + 2u) % 3u] * pos_stride), FN(ld)(pos + (size_t)i[(j + 1u) % 3u] * pos_stride));
        r = SQRT(FN(dot3)(d, d));
      } else if (ok) {
        walk_t w = walk_begin(faces, off, f, j);
        uint32_t g, jp, count = 1u;
        while (walk_next(&w, faces, corners, &g, &jp)) {
          FN(v3) ng;
          real rg;
          ++count;
          if (kind == DIHEDRAL && FN(unit_normal)(pos, pos_stride, faces + (size_t)g * 3u, &ng, &rg)) {
            const real t = (real)1 - FN(dot3)(nf, ng);
            r = r + t;
          }
        }
        if (kind == COUNT) r = (real)count;
      }
      out[(size_t)f * out_stride + j] = r;
    }
  }
}

/* one position set, LENGTH or DIHEDRAL: gout (records of gout_stride reals) -> gpos [n_verts][3]; work [n_faces][3] (DIHEDRAL) */
void FN(er_backward)(const real *pos, uint32_t pos_stride, uint32_t n_verts, uint32_t n_faces, const uint32_t *faces, const uint32_t *off,
                     const uint32_t *corners, int kind, const real *gout, uint32_t gout_stride, real *work, real *gpos) {
  if (kind == DIHEDRAL)
    for (uint32_t f = 0; f < n_faces; ++f) {
      const uint32_t *i = faces + (size_t)f * 3u;
      FN(v3) nf, gN = {(real)0, (real)0, (real)0};
      real rf;
      if (FN(unit_normal)(pos, pos_stride, i, &nf, &rf)) {
        FN(v3) H = {(real)0, (real)0, (real)0};
        for (uint32_t j = 0; j < 3u; ++j) {
          walk_t w = walk_begin(faces, off, f, j);
          uint32_t g, jp;
          while (walk_next(&w, faces, corners, &g, &jp)) {
            FN(v3) ng;
            real rg;
            if (!FN(unit_normal)(pos, pos_stride, faces + (size_t)g * 3u, &ng, &rg)) continue;
            const real s = gout[(size_t)f * gout_stride + j] + gout[(size_t)g * gout_stride + jp];
            const real hx = ng.x * s, hy = ng.y * s, hz = ng.z * s;
            H = (FN(v3)){H.x - hx, H.y - hy, H.z - hz};
          }
        }
        const real t = FN(dot3)(nf, H);
        const real tx = nf.x * t, ty = nf.y * t, tz = nf.z * t;
        gN = (FN(v3)){(H.x - tx) * rf, (H.y - ty) * rf, (H.z - tz) * rf};
      }
      work[(size_t)f * 3u] = gN.x, work[(size_t)f * 3u + 1u] = gN.y, work[(size_t)f * 3u + 2u] = gN.z;
    }
  for (uint32_t v = 0; v < n_verts; ++v) {
    FN(v3) acc = {(real)0, (real)0, (real)0};
    for (uint32_t c = off[v]; c < off[v + 1u]; ++c) {
      const uint32_t f = corners[c] / 3u, k = corners[c] % 3u;
      const uint32_t *i = faces + (size_t)f * 3u;
      const FN(v3) P[3] = {FN(ld)(pos + (size_t)i[0] * pos_stride), FN(ld)(pos + (size_t)i[1] * pos_stride), FN(ld)(pos + (size_t)i[2] * pos_stride)};
      if (kind == LENGTH) {
        const uint32_t j1 = (k + 1u) % 3u, j2 = (k + 2u) % 3u;
        const FN(v3) d1 = FN(sub)(P[k], P[(k + 2u) % 3u]), d2 = FN(sub)(P[(k + 1u) % 3u], P[k]); /* d_j = p[b_j] - p[a_j] */
        const real len1 = SQRT(FN(dot3)(d1, d1));
        if (len1 > (real)0 && len1 <= REAL_MAX) {
          const real inv = (real)1 / len1, g = gout[(size_t)f * gout_stride + j1];
          const real ux = d1.x * inv, uy = d1.y * inv, uz = d1.z * inv;
          const real tx = g * ux, ty = g * uy, tz = g * uz;
          acc = (FN(v3)){acc.x + tx, acc.y + ty, acc.z + tz};
        }
        const real len2 = SQRT(FN(dot3)(d2, d2));
        if (len2 > (real)0 && len2 <= REAL_MAX) {
          const real inv = (real)1 / len2, g = gout[(size_t)f * gout_stride + j2];
          const real ux = d2.x * inv, uy = d2.y * inv, uz = d2.z * inv;
          const real tx = g * ux, ty = g * uy, tz = g * uz;
          acc = (FN(v3)){acc.x - tx, acc.y - ty, acc.z - tz};
        }
      } else {
        const FN(v3) G = FN(ld)(work + (size_t)f * 3u);
        const FN(v3) term = k == 0u ? FN(cross)(FN(sub)(P[1], P[2]), G) : k == 1u ? FN(cross)(FN(sub)(P[2], P[0]), G) : FN(cross)(G, FN(sub)(P[1], P[0]));
        acc = FN(add)(acc, term);
      }
    }
    gpos[(size_t)v * 3u] = acc.x, gpos[(size_t)v * 3u + 1u] = acc.y, gpos[(size_t)v * 3u + 2u] = acc.z;
  }
}

#endif
