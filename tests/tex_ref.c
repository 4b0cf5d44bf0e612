/* The texture pass's test reference (tests/texref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math).  It includes nothing of
 * the library: per pixel of a visibility buffer (owner id word) with its u and v, a float texture [row][column][channel] sampled
 * bilinearly by the rule include/srz.h states for srz_frameset_texture, restated here —
 *   unsampled: u or v not finite -> out 0, guv (0, 0), no add
 *   per axis (x with u and W; y with v and H):  WRAP: u = u - floorf(u);  fx = u * (float)W - 0.5f;
 *     CLAMP: in_x = fx > 0 && fx < W - 1, fx = fminf(fmaxf(fx, 0), W - 1);  x0f = floorf(fx), tx = fx - x0f, x0 = (int)x0f, x1 = x0 + 1;
 *     CLAMP: x1 = min(x1, W - 1);  WRAP: x0 < 0 -> x0 += W, x1 >= W -> x1 -= W
 *   top = fmaf(tx, t01 - t00, t00);  bot = fmaf(tx, t11 - t10, t10);  out = fmaf(ty, bot - top, top)
 * — fmaf where the rule fuses and nothing else fused; and the backward of that: the gradient with respect to u and v in float (one
 * fmaf per channel and axis, ascending), the gradient with respect to the texels in DOUBLE (the sum of the float32 products
 * w_rc * g, added exactly enough to stand for the exact sum), with the count of contributing adds per texel and the sum of
 * |w_rc * g| per element, from which the test derives its bound. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

enum { TR_CLAMP = 0, TR_WRAP = 1 };
typedef struct {
  int x0, x1, y0, y1;
  float tx, ty;
  int in_x, in_y;
  int wrapped; /* WRAP: x1 or y1 went past the last texel and came back to 0 */
} Tap;

static void axis(float u, int n, int mode, int *i0, int *i1, float *t, int *in, int *wrapped) {
  if (mode == TR_WRAP) u = u - floorf(u);
  float fx = u * (float)n - 0.5f;
  *in = 1;
  if (mode == TR_CLAMP) {
    *in = fx > 0.0f && fx < (float)(n - 1);
    fx = fminf(fmaxf(fx, 0.0f), (float)(n - 1));
  }
  const float f0 = floorf(fx);
  *t = fx - f0;
  *i0 = (int)f0, *i1 = *i0 + 1;
  if (mode == TR_CLAMP) {
    if (*i1 > n - 1) *i1 = n - 1;
  } else {
    if (*i0 < 0) *i0 += n;
    if (*i1 >= n) *i1 -= n, *wrapped = 1;
  }
}

/* 0: the pixel is not sampled */
static int tap_of(float u, float v, int W, int H, int mode, Tap *p) {
  if (!(fabsf(u) < INFINITY) || !(fabsf(v) < INFINITY)) return 0;
  p->wrapped = 0;
  axis(u, W, mode, &p->x0, &p->x1, &p->tx, &p->in_x, &p->wrapped);
  axis(v, H, mode, &p->y0, &p->y1, &p->ty, &p->in_y, &p->wrapped);
  return 1;
}

static int owned(uint32_t id, uint32_t n_tris) { return (id & 0x7fffffffu) - 1u < n_tris; }

/* per pixel: bit 0 owned, bit 1 sampled, bit 2 (sampled) in_x or in_y false, bit 3 (sampled) x1 or y1 wrapped */
void tr_classify(int W, int H, int mode, uint32_t n_tris, size_t n_px, const uint32_t *id, const float *u, const float *v, uint8_t *cls) {
  for (size_t p = 0; p < n_px; ++p) {
    Tap t;
    cls[p] = 0;
    if (!owned(id[p], n_tris)) continue;
    cls[p] = 1;
    if (!tap_of(u[p], v[p], W, H, mode, &t)) continue;
    cls[p] |= 2 | ((!t.in_x || !t.in_y) ? 4 : 0) | (t.wrapped ? 8 : 0);
  }
}

/* tex: [H][W][n_ch]; id: plane 1 of the frame's visibility buffer; u, v: the two uv planes, n_px words each; out: n_ch planes of n_px.
 * A pixel nobody owns (id 0, the bare class bit, an index outside the n_tris triangles): 0 when fused, else its words stay. */
void tr_forward(const float *tex, int W, int H, uint32_t n_ch, int mode, uint32_t n_tris, size_t n_px, const uint32_t *id, const float *u,
                const float *v, int fused, float *out) {
  for (size_t p = 0; p < n_px; ++p) {
    Tap t;
    if (!owned(id[p], n_tris)) {
      if (fused)
        for (uint32_t ch = 0; ch < n_ch; ++ch) out[ch * n_px + p] = 0.0f;
      continue;
    }
    if (!tap_of(u[p], v[p], W, H, mode, &t)) {
      for (uint32_t ch = 0; ch < n_ch; ++ch) out[ch * n_px + p] = 0.0f;
      continue;
    }
    const float *r0 = tex + (size_t)t.y0 * W * n_ch, *r1 = tex + (size_t)t.y1 * W * n_ch;
    for (uint32_t ch = 0; ch < n_ch; ++ch) {
      const float t00 = r0[(size_t)t.x0 * n_ch + ch], t01 = r0[(size_t)t.x1 * n_ch + ch];
      const float t10 = r1[(size_t)t.x0 * n_ch + ch], t11 = r1[(size_t)t.x1 * n_ch + ch];
      const float top = fmaf(t.tx, t01 - t00, t00), bot = fmaf(t.tx, t11 - t10, t10);
      out[ch * n_px + p] = fmaf(t.ty, bot - top, top);
    }
  }
}

/* gout: n_ch planes of n_px (words at nobody's pixels are never read).  gtex, gabs: [H][W][n_ch] doubles, added into; count: [H][W]
 * contributing adds per texel, added into (any of the three may be null).  guv: 2 planes of n_px (null: not wanted; needs tex). */
void tr_grad(const float *tex, int W, int H, uint32_t n_ch, int mode, uint32_t n_tris, size_t n_px, const uint32_t *id, const float *u,
             const float *v, const float *gout, int fused, double *gtex, double *gabs, uint32_t *count, float *guv) {
  for (size_t p = 0; p < n_px; ++p) {
    Tap t;
    if (!owned(id[p], n_tris)) {
      if (fused && guv) guv[p] = 0.0f, guv[n_px + p] = 0.0f;
      continue;
    }
    if (!tap_of(u[p], v[p], W, H, mode, &t)) {
      if (guv) guv[p] = 0.0f, guv[n_px + p] = 0.0f;
      continue;
    }
    const size_t at[4] = {(size_t)t.y0 * W + t.x0, (size_t)t.y0 * W + t.x1, (size_t)t.y1 * W + t.x0, (size_t)t.y1 * W + t.x1};
    const float wk[4] = {(1.0f - t.tx) * (1.0f - t.ty), t.tx * (1.0f - t.ty), (1.0f - t.tx) * t.ty, t.tx * t.ty};
    for (int k = 0; k < 4; ++k) {
      if (count) count[at[k]] += 1u;
      for (uint32_t ch = 0; ch < n_ch; ++ch) {
        const float prod = wk[k] * gout[ch * n_px + p]; /* the float32 product the pass adds */
        if (gtex) gtex[at[k] * n_ch + ch] += (double)prod;
        if (gabs) gabs[at[k] * n_ch + ch] += fabs((double)prod);
      }
    }
    if (guv) {
      float au = 0.0f, av = 0.0f;
      for (uint32_t ch = 0; ch < n_ch; ++ch) {
        const float g = gout[ch * n_px + p];
        const float t00 = tex[at[0] * n_ch + ch], t01 = tex[at[1] * n_ch + ch], t10 = tex[at[2] * n_ch + ch], t11 = tex[at[3] * n_ch + ch];
        const float top = fmaf(t.tx, t01 - t00, t00), bot = fmaf(t.tx, t11 - t10, t10);
        au = fmaf(g, fmaf(t.ty, (t11 - t10) - (t01 - t00), t01 - t00), au);
        av = fmaf(g, bot - top, av);
      }
      guv[p] = t.in_x ? au * (float)W : 0.0f;
      guv[n_px + p] = t.in_y ? av * (float)H : 0.0f;
    }
  }
}
