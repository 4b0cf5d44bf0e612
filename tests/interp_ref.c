/* The attribute interpolation's test reference (tests/interpref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math).  It
 * includes nothing of the library: per pixel of a visibility buffer (owner id word, alpha, beta) and per channel, the owner's three
 * corner values under those barycentrics as the reference's two fragment paths interpolate uv,
 *   V (processFragByAVX2): gamma = 1 - (alpha + beta); fmaf(alpha, a, fmaf(beta, b, gamma * c));
 *   S (processFragByScalar): gamma = 1 - alpha - beta; alpha * a + beta * b + gamma * c, left to right;
 * fmaf where the reference fuses and nothing else fused; and the backward of that: the gradient with respect to alpha and beta in
 * float (one fmaf per channel, ascending, on the rounded differences), the gradient with respect to the attributes in DOUBLE (the sum
 * of the float32 products w * g, added exactly enough to stand for the exact sum), with the count of contributing pixels and the sum
 * of |w * g| per element, from which the test derives its bound. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

/* attr: [n_tris][3][n_ch]; id, al, be: planes 1, 2, 3 of the frame's visibility buffer, n_px words each; out: n_ch planes of n_px.
 * A pixel nobody owns (id 0, the bare class bit, an index outside the n_tris triangles): 0 when fused, else its words stay. */
void ir_forward(const float *attr, uint32_t n_ch, uint32_t n_tris, size_t n_px, const uint32_t *id, const float *al, const float *be,
                int fused, float *out) {
  for (size_t p = 0; p < n_px; ++p) {
    const uint32_t w = id[p], idx = (w & 0x7fffffffu) - 1u;
    if (idx >= n_tris) {
      if (fused)
        for (uint32_t ch = 0; ch < n_ch; ++ch) out[ch * n_px + p] = 0.0f;
      continue;
    }
    const float *t = attr + (size_t)idx * 3u * n_ch;
    const float alpha = al[p], beta = be[p];
    if (!(w >> 31)) {
      const float gamma = 1.0f - (alpha + beta);
      for (uint32_t ch = 0; ch < n_ch; ++ch) out[ch * n_px + p] = fmaf(alpha, t[ch], fmaf(beta, t[n_ch + ch], gamma * t[2u * n_ch + ch]));
    } else {
      const float gamma = 1.0f - alpha - beta;
      for (uint32_t ch = 0; ch < n_ch; ++ch) out[ch * n_px + p] = alpha * t[ch] + beta * t[n_ch + ch] + gamma * t[2u * n_ch + ch];
    }
  }
}

/* gout: n_ch planes of n_px (words at nobody's pixels are never read).  gattr, gabs: [n_tris][3][n_ch] doubles, added into; count:
 * [n_tris] pixels owned, added into (any of the three may be null).  gbary: 2 planes of n_px (null: not wanted; needs attr). */
void ir_grad(const float *attr, uint32_t n_ch, uint32_t n_tris, size_t n_px, const uint32_t *id, const float *al, const float *be,
             const float *gout, int fused, double *gattr, double *gabs, uint32_t *count, float *gbary) {
  for (size_t p = 0; p < n_px; ++p) {
    const uint32_t w = id[p], idx = (w & 0x7fffffffu) - 1u;
    if (idx >= n_tris) {
      if (fused && gbary) gbary[p] = 0.0f, gbary[n_px + p] = 0.0f;
      continue;
    }
    const float alpha = al[p], beta = be[p];
    const float gamma = (w >> 31) ? 1.0f - alpha - beta : 1.0f - (alpha + beta);
    const float wk[3] = {alpha, beta, gamma};
    if (count) count[idx] += 1u;
    for (uint32_t ch = 0; ch < n_ch; ++ch) {
      const float g = gout[ch * n_px + p];
      for (int k = 0; k < 3; ++k) {
        const float prod = wk[k] * g; /* the float32 product the pass adds */
        if (gattr) gattr[((size_t)idx * 3u + k) * n_ch + ch] += (double)prod;
        if (gabs) gabs[((size_t)idx * 3u + k) * n_ch + ch] += fabs((double)prod);
      }
    }
    if (gbary) {
      const float *t = attr + (size_t)idx * 3u * n_ch;
      float da = 0.0f, db = 0.0f;
      for (uint32_t ch = 0; ch < n_ch; ++ch) {
        const float g = gout[ch * n_px + p], c = t[2u * n_ch + ch];
        const float ac = t[ch] - c, bc = t[n_ch + ch] - c;
        da = fmaf(g, ac, da), db = fmaf(g, bc, db);
      }
      gbary[p] = da, gbary[n_px + p] = db;
    }
  }
}
