/* Vertex normals and per-vertex attributes: the test reference of srz_mesh_normals, srz_mesh_normals_grad, srz_sceneset_corner_attr
 * and srz_sceneset_corner_attr_grad (tests/normalsref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math).  It includes
 * nothing of the library and makes its own corner lists.  THE RULES, in float32, nothing fused, in this order:
 *   cross(u, w) = (u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x);   dot3(a, b) = (a.x b.x + a.y b.y) + a.z b.z
 * NORMALS, per vertex v, list(v) its corners 3 * face + k in increasing order:
 *   S = +0;  for c in list(v):  (i0, i1, i2) = faces[c / 3];  S = S + cross(p[i1] - p[i0], p[i2] - p[i0])
 *   len2 = dot3(S, S);   len2 > 0 && len2 <= FLT_MAX:  r = 1.0f / sqrtf(len2), n = S * r;   otherwise n = +0
 * THEIR BACKWARD, two phases:
 *   1, per vertex:  normalised:  d = dot3(n, g), gS = (g - n * d) * r;   otherwise gS = +0
 *   2, per vertex:  acc = +0;  for c in list(v):  a, b, c' = p[faces[c / 3]], G = (gS[i0] + gS[i1]) + gS[i2],
 *      c % 3 == 0: acc = acc + cross(b - c', G);  1: acc = acc + cross(c' - a, G);  2: acc = acc + cross(G, b - a)
 * CORNER ATTRIBUTES of one draw whose first frame-local triangle is `first`:  out[first + face][k][ch] = attr[faces[face][k]][ch]
 * THEIR BACKWARD:  sum[v][ch] = sum[v][ch] + gout[first + c / 3][c % 3][ch] for c in list(v), in list order (the caller starts a
 * frame's sums at +0 and calls once per draw of the mesh, in draw order) */
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

typedef struct {
  float x, y, z;
} v3;
static v3 ld(const float *p) { return (v3){p[0], p[1], p[2]}; }
static v3 sub(v3 a, v3 b) { return (v3){a.x - b.x, a.y - b.y, a.z - b.z}; }
static v3 add(v3 a, v3 b) { return (v3){a.x + b.x, a.y + b.y, a.z + b.z}; }
static v3 cross(v3 u, v3 w) {
  const float x0 = u.y * w.z, x1 = u.z * w.y, y0 = u.z * w.x, y1 = u.x * w.z, z0 = u.x * w.y, z1 = u.y * w.x;
  return (v3){x0 - x1, y0 - y1, z0 - z1};
}
static float dot3(v3 a, v3 b) {
  const float tx = a.x * b.x, ty = a.y * b.y, tz = a.z * b.z;
  return (tx + ty) + tz;
}

/* the corner lists of a face list by a counting sort: off [n_verts + 1], corners [3 * n_faces] */
void nr_corner_lists(const uint32_t *faces, uint32_t n_faces, uint32_t n_verts, uint32_t *off, uint32_t *corners, uint32_t *scratch) {
  for (uint32_t v = 0; v <= n_verts; ++v) off[v] = 0;
  for (uint32_t i = 0; i < 3u * n_faces; ++i) off[faces[i] + 1u] += 1u;
  for (uint32_t v = 0; v < n_verts; ++v) off[v + 1u] += off[v];
  for (uint32_t v = 0; v < n_verts; ++v) scratch[v] = off[v];
  for (uint32_t i = 0; i < 3u * n_faces; ++i) corners[scratch[faces[i]]++] = i;
}

static v3 normal_sum(const float *pos, uint32_t stride, const uint32_t *faces, const uint32_t *off, const uint32_t *corners, uint32_t v) {
  v3 S = {0.0f, 0.0f, 0.0f};
  for (uint32_t c = off[v]; c < off[v + 1u]; ++c) {
    const uint32_t *f = faces + (size_t)(corners[c] / 3u) * 3u;
    const v3 p0 = ld(pos + (size_t)f[0] * stride);
    S = add(S, cross(sub(ld(pos + (size_t)f[1] * stride), p0), sub(ld(pos + (size_t)f[2] * stride), p0)));
  }
  return S;
}
static int normal_scale(v3 S, float *r) {
  const float len2 = dot3(S, S);
  const int ok = len2 > 0.0f && len2 <= FLT_MAX;
  *r = ok ? 1.0f / sqrtf(len2) : 0.0f;
  return ok;
}

/* one position set: pos [n_verts] records of pos_stride floats -> nrm, records of nrm_stride floats (three floats written each);
 * normalised (null: not wanted): [n_verts] bytes, 1 where the vertex was normalised */
void nr_normals(const float *pos, uint32_t pos_stride, uint32_t n_verts, const uint32_t *faces, const uint32_t *off, const uint32_t *corners,
                float *nrm, uint32_t nrm_stride, uint8_t *normalised) {
  for (uint32_t v = 0; v < n_verts; ++v) {
    const v3 S = normal_sum(pos, pos_stride, faces, off, corners, v);
    float r;
    const int ok = normal_scale(S, &r);
    float *n = nrm + (size_t)v * nrm_stride;
    n[0] = ok ? S.x * r : 0.0f, n[1] = ok ? S.y * r : 0.0f, n[2] = ok ? S.z * r : 0.0f;
    if (normalised) normalised[v] = (uint8_t)ok;
  }
}

/* one position set: gnrm records of gnrm_stride floats -> gpos [n_verts][3], every element written; work: [n_verts][3] */
void nr_normals_grad(const float *pos, uint32_t pos_stride, uint32_t n_verts, const uint32_t *faces, const uint32_t *off,
                     const uint32_t *corners, const float *gnrm, uint32_t gnrm_stride, float *work, float *gpos) {
  for (uint32_t v = 0; v < n_verts; ++v) {
    const v3 S = normal_sum(pos, pos_stride, faces, off, corners, v);
    float r;
    v3 gS = {0.0f, 0.0f, 0.0f};
    if (normal_scale(S, &r)) {
      const v3 n = {S.x * r, S.y * r, S.z * r}, g = ld(gnrm + (size_t)v * gnrm_stride);
      const float d = dot3(n, g);
      const float px = n.x * d, py = n.y * d, pz = n.z * d;
      const float qx = g.x - px, qy = g.y - py, qz = g.z - pz;
      gS = (v3){qx * r, qy * r, qz * r};
    }
    work[(size_t)v * 3u] = gS.x, work[(size_t)v * 3u + 1u] = gS.y, work[(size_t)v * 3u + 2u] = gS.z;
  }
  for (uint32_t v = 0; v < n_verts; ++v) {
    v3 acc = {0.0f, 0.0f, 0.0f};
    for (uint32_t c = off[v]; c < off[v + 1u]; ++c) {
      const uint32_t face = corners[c] / 3u, k = corners[c] % 3u;
      const uint32_t i0 = faces[(size_t)face * 3u], i1 = faces[(size_t)face * 3u + 1u], i2 = faces[(size_t)face * 3u + 2u];
      const v3 A = ld(pos + (size_t)i0 * pos_stride), B = ld(pos + (size_t)i1 * pos_stride), C = ld(pos + (size_t)i2 * pos_stride);
      const v3 G = add(add(ld(work + (size_t)i0 * 3u), ld(work + (size_t)i1 * 3u)), ld(work + (size_t)i2 * 3u));
      const v3 term = k == 0u ? cross(sub(B, C), G) : k == 1u ? cross(sub(C, A), G) : cross(G, sub(B, A));
      acc = add(acc, term);
    }
    gpos[(size_t)v * 3u] = acc.x, gpos[(size_t)v * 3u + 1u] = acc.y, gpos[(size_t)v * 3u + 2u] = acc.z;
  }
}

/* one draw: attr [n_verts][n_ch] -> the frame's out [pos_tris][3][n_ch], the draw's triangles only */
void nr_corner_attr(const float *attr, const uint32_t *faces, uint32_t n_faces, uint32_t n_ch, uint32_t first, float *out) {
  for (uint32_t i = 0; i < 3u * n_faces; ++i)
    for (uint32_t ch = 0; ch < n_ch; ++ch) out[((size_t)first * 3u + i) * n_ch + ch] = attr[(size_t)faces[i] * n_ch + ch];
}

/* one draw: the frame's gout [pos_tris][3][n_ch] -> the running sums [n_verts][n_ch] */
void nr_corner_attr_grad(const float *gout, const uint32_t *off, const uint32_t *corners, uint32_t n_verts, uint32_t n_ch, uint32_t first,
                         float *sum) {
  for (uint32_t v = 0; v < n_verts; ++v)
    for (uint32_t ch = 0; ch < n_ch; ++ch) {
      float s = sum[(size_t)v * n_ch + ch];
      for (uint32_t c = off[v]; c < off[v + 1u]; ++c) s = s + gout[((size_t)first * 3u + corners[c]) * n_ch + ch];
      sum[(size_t)v * n_ch + ch] = s;
    }
}
