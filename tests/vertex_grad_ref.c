/* The vertex stage's backward: the test reference of srz_sceneset_vertex_grad (tests/vertexgradref.py builds it with gcc -O2
 * -ffp-contract=off -fno-fast-math).  It includes nothing of the library and makes its own corner lists.  THE RULE, in float32,
 * nothing fused but the written fmaf, IEEE divisions.  For frame f, vertex v, and each draw j of frame f that names the mesh, in draw
 * order, with `first` the draw's first frame-local triangle and m, zs the draw's ndc_mvp and zscale:
 *   GX = GY = GZ = +0;  for (face, k) in list(v), in list order:  p = gpos[f][first + face] + 3k;  GX = GX + p[0]; GY = GY + p[1]; GZ = GZ + p[2]
 *   GX == 0 && GY == 0 && GZ == 0:  this draw contributes nothing for v            (a NaN is not 0 and goes on)
 *   (x, y, z) = verts[v].pos;   r_i = (m[i]*x + m[4+i]*y) + (m[8+i]*z + m[12+i]), i = 0..3      (k_vertex's own expression)
 *   X = r0/r3;  Y = r1/r3;  Q = r2/r3;  inv = 1.0f/r3;  gq = GZ*zs
 *   g0 = GX*inv;  g1 = GY*inv;  g2 = gq*inv;  s = gq*Q;  s = fmaf(GY, Y, s);  s = fmaf(GX, X, s);  g3 = (-s)*inv
 *   c = 0..2:  t = m[4c]*g0;  t = fmaf(m[4c+1], g1, t);  t = fmaf(m[4c+2], g2, t);  t = fmaf(m[4c+3], g3, t);
 *              gverts[f][v][c] = gverts[f][v][c] + t            (one add per contributing draw, draw order: DETERMINISTIC, bit for bit)
 *   gdraw[f][j][4c+i] += g_i * (x, y, z)[c]  (c = 3: g_i);   gdraw[f][j][16] += GZ*Q;   gdraw[f][j][17] += GZ
 * gverts in float32, bit for bit; gdraw in DOUBLE (the sum of the float32 terms), with the sum of |term| per element and the count
 * of contributing vertices, from which the test derives its bound. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

/* the corner lists of a face list by a counting sort: off [n_verts + 1], corners [3 * n_faces]; vertex v's corners 3 * face + k come
 * in increasing order */
void vg_corner_lists(const uint32_t *faces, uint32_t n_faces, uint32_t n_verts, uint32_t *off, uint32_t *corners, uint32_t *scratch) {
  for (uint32_t v = 0; v <= n_verts; ++v) off[v] = 0;
  for (uint32_t i = 0; i < 3u * n_faces; ++i) off[faces[i] + 1u] += 1u;
  for (uint32_t v = 0; v < n_verts; ++v) off[v + 1u] += off[v];
  for (uint32_t v = 0; v < n_verts; ++v) scratch[v] = off[v];
  for (uint32_t i = 0; i < 3u * n_faces; ++i) corners[scratch[faces[i]]++] = i;
}

/* ONE draw of one frame.  verts8: [n_verts][8] (the position is the first three floats); off, corners: vg_corner_lists' lists;
 * gpos: the frame's [pos_tris][9]; first: the draw's first frame-local triangle; m: the draw's 16 floats; zs: its zscale.
 * gverts: [n_verts][3] float32, added into by the rule (null: not wanted).  gdraw, gabs: [18] doubles, added into; count: [1], the
 * contributing vertices, added into (null: not wanted, all three). */
void vg_draw(const float *verts8, uint32_t n_verts, const uint32_t *off, const uint32_t *corners, const float *gpos, uint32_t first,
             const float *m, float zs, float *gverts, double *gdraw, double *gabs, uint32_t *count) {
  for (uint32_t v = 0; v < n_verts; ++v) {
    float GX = 0.0f, GY = 0.0f, GZ = 0.0f;
    for (uint32_t c = off[v]; c < off[v + 1u]; ++c) {
      const uint32_t face = corners[c] / 3u, k = corners[c] % 3u;
      const float *p = gpos + (size_t)(first + face) * 9u + 3u * k;
      GX = GX + p[0], GY = GY + p[1], GZ = GZ + p[2];
    }
    if (GX == 0.0f && GY == 0.0f && GZ == 0.0f) continue;
    const float P[3] = {verts8[(size_t)v * 8u], verts8[(size_t)v * 8u + 1u], verts8[(size_t)v * 8u + 2u]};
    float r[4], g[4];
    for (int i = 0; i < 4; ++i) {
      const float add0 = m[i] * P[0] + m[4 + i] * P[1];
      const float add1 = m[8 + i] * P[2] + m[12 + i];
      r[i] = add0 + add1;
    }
    const float X = r[0] / r[3], Y = r[1] / r[3], Q = r[2] / r[3], inv = 1.0f / r[3], gq = GZ * zs;
    g[0] = GX * inv, g[1] = GY * inv, g[2] = gq * inv;
    float s = gq * Q;
    s = fmaf(GY, Y, s), s = fmaf(GX, X, s);
    g[3] = (-s) * inv;
    if (gverts)
      for (int c = 0; c < 3; ++c) {
        float t = m[4 * c] * g[0];
        t = fmaf(m[4 * c + 1], g[1], t), t = fmaf(m[4 * c + 2], g[2], t), t = fmaf(m[4 * c + 3], g[3], t);
        gverts[(size_t)v * 3u + c] = gverts[(size_t)v * 3u + c] + t;
      }
    if (gdraw) {
      float term[18];
      for (int c = 0; c < 4; ++c)
        for (int i = 0; i < 4; ++i) term[4 * c + i] = c < 3 ? g[i] * P[c] : g[i];
      term[16] = GZ * Q, term[17] = GZ;
      for (int e = 0; e < 18; ++e) gdraw[e] += (double)term[e], gabs[e] += fabs((double)term[e]);
      count[0] += 1u;
    }
  }
}
