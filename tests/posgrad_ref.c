/* The position gradient's test reference (tests/posgradref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math).  It includes
 * nothing of the library.  Per owned pixel of a visibility buffer (owner id word, alpha, beta), with P the owner's nine position
 * floats ax ay z0 bx by z1 cx cy z2 and w = (alpha, beta, gamma), gamma = 1 - (alpha + beta) for a V pixel and 1 - alpha - beta for
 * an S pixel, in float32, fmaf where written and nothing else fused:
 *   area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);  r = 1.0f / area
 *   da = gbary ? dalpha : 0, db likewise;  with gz: da = fmaf(gz, z0 - z2, da), db = fmaf(gz, z1 - z2, db)
 *   gx = (da * (by - cy) + db * (cy - ay)) * r;  gy = (da * (cx - bx) + db * (ax - cx)) * r          -> gpix
 *   corner k: terms (-w[k]) * gx, (-w[k]) * gy and, with gz, w[k] * gz                                -> gpos[t][3k .. 3k + 2]
 * gpix in float; gpos in DOUBLE (the sum of the float32 terms, added exactly enough to stand for the exact sum), with the sum of
 * |term| per element and the count of contributing pixels per triangle, from which the test derives its bound. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

/* pos: [n_tris or more][9]; id, al, be: planes 1, 2, 3 of the frame's visibility buffer, n_px words each; gbary: 2 planes of n_px or
 * null; gz: 1 plane or null (words at nobody's pixels are never read).  gpos, gabs: [..][9] doubles, added into; count: [..] pixels
 * owned, added into (any of the three may be null).  gpix: 2 planes of n_px (null: not wanted); a pixel nobody owns (id 0, the bare
 * class bit, an index outside the n_tris triangles): 0 when fused, else its words stay. */
void pg_grad(const float *pos, uint32_t n_tris, size_t n_px, const uint32_t *id, const float *al, const float *be, const float *gbary,
             const float *gz, int fused, double *gpos, double *gabs, uint32_t *count, float *gpix) {
  for (size_t p = 0; p < n_px; ++p) {
    const uint32_t word = id[p], idx = (word & 0x7fffffffu) - 1u;
    if (idx >= n_tris) {
      if (fused && gpix) gpix[p] = 0.0f, gpix[n_px + p] = 0.0f;
      continue;
    }
    const float *P = pos + (size_t)idx * 9u;
    const float ax = P[0], ay = P[1], z0 = P[2], bx = P[3], by = P[4], z1 = P[5], cx = P[6], cy = P[7], z2 = P[8];
    const float alpha = al[p], beta = be[p];
    const float gamma = (word >> 31) ? 1.0f - alpha - beta : 1.0f - (alpha + beta);
    const float w[3] = {alpha, beta, gamma};
    const float area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    const float r = 1.0f / area;
    float da = gbary ? gbary[p] : 0.0f, db = gbary ? gbary[n_px + p] : 0.0f;
    const float g = gz ? gz[p] : 0.0f;
    if (gz) da = fmaf(g, z0 - z2, da), db = fmaf(g, z1 - z2, db);
    const float gx = (da * (by - cy) + db * (cy - ay)) * r;
    const float gy = (da * (cx - bx) + db * (ax - cx)) * r;
    if (gpix) gpix[p] = gx, gpix[n_px + p] = gy;
    if (count) count[idx] += 1u;
    for (int k = 0; k < 3; ++k) {
      const float term[3] = {(-w[k]) * gx, (-w[k]) * gy, w[k] * g}; /* the float32 terms the pass adds */
      for (int c = 0; c < (gz ? 3 : 2); ++c) {
        if (gpos) gpos[(size_t)idx * 9u + 3 * k + c] += (double)term[c];
        if (gabs) gabs[(size_t)idx * 9u + 3 * k + c] += fabs((double)term[c]);
      }
    }
  }
}
