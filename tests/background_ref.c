/* The background pass's test reference (tests/backgroundref.py builds it like tests/cube_ref.c: gcc -O2 -ffp-contract=off
 * -fno-fast-math; no flush to zero).  It includes nothing of the library.  The cube lookup — the face, s and t, the 24 seam rows, the
 * three fmafs, gdir — is tests/cube_ref.c's, INCLUDED below, not copied: tap_of, owned and the tables are the very ones the cube
 * tests pin.  What this file restates is what include/srz.h adds for srz_frameset_background:
 *   the pass's pixels: with where == 0 those nobody owns (!owned(id)), with where == 1 every pixel (id is not read, may be null)
 *   the direction of pixel (x, y), y the frame's row:  d_c = fmaf((float)y, ry_c, fmaf((float)x, rx_c, r0_c)),  ray = r0[3] rx[3] ry[3]
 *   from d on: cube_ref.c.  An unsampled pixel of the pass writes zeros and contributes nothing.
 *   owned pixels (where == 0): 0 when fused, else their words stay
 *   backward: gtex as cr_grad adds it (double sums of the float32 products, counts, sums of magnitudes); the nine float32 terms of a
 *   sampled pixel gdir_c, (float)x * gdir_c, (float)y * gdir_c, their exact sums in double with the sums of magnitudes and the count,
 *   and their sum in the FIXED tree: a pixel (x, y) of a 32 x 32 tile belongs to lane (y % 8) * 8 + x % 32 / 4 of wave y % 32 / 8; a
 *   lane adds its up to four pixels' terms left to right, from +0; the 64 lanes of a wave by the butterfly v = v + v[lane ^ o], o =
 *   32, 16, 8, 4, 2, 1; the four waves as ((w0 + w1) + w2) + w3; a frame's tiles in tile order (bands, then columns), from +0; and
 *   (br_fold) rows in order, from +0. */
#include "cube_ref.c"

static void ray_dir(const float *ray, int x, int y, float d[3]) {
  for (int c = 0; c < 3; ++c) d[c] = fmaf((float)y, ray[6 + c], fmaf((float)x, ray[3 + c], ray[c]));
}
static int in_pass(const uint32_t *id, uint32_t n_tris, int where, size_t p) { return where == 1 || !owned(id[p], n_tris); }

/* the direction planes [3][H][W] the rule computes at every pixel of a W x H frame */
void br_dirs(const float *ray, int W, int H, float *dirs) {
  const size_t n_px = (size_t)W * H;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      float d[3];
      ray_dir(ray, x, y, d);
      for (int c = 0; c < 3; ++c) dirs[c * n_px + (size_t)y * W + x] = d[c];
    }
}

/* per pixel: bit 0 a pixel of the pass, bit 1 sampled, bit 2 a corner on another face, bit 3 a corner outside in both axes; face: of a
 * sampled pixel, else 255; at: [H][W][4] the resolved texels of a sampled pixel */
void br_classify(int N, uint32_t n_tris, int W, int H, const uint32_t *id, const float *ray, int where, uint8_t *cls, uint8_t *face,
                 uint32_t *at) {
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t p = (size_t)y * W + x;
      Tap t;
      float d[3];
      cls[p] = 0, face[p] = 255;
      if (!in_pass(id, n_tris, where, p)) continue;
      cls[p] = 1;
      ray_dir(ray, x, y, d);
      if (!tap_of(d, N, -1, &t)) continue;
      cls[p] |= 2 | (t.crossed ? 4 : 0) | (t.both ? 8 : 0);
      face[p] = (uint8_t)t.face;
      for (int k = 0; k < 4; ++k) at[4 * p + k] = (uint32_t)t.at[k];
    }
}

/* tex: [6][N][N][n_ch]; id: plane 1 of the frame's visibility buffer (where == 1: not read); out: n_ch planes of W * H */
void br_forward(const float *tex, int N, uint32_t n_ch, uint32_t n_tris, int W, int H, const uint32_t *id, const float *ray, int where,
                int fused, float *out) {
  const size_t n_px = (size_t)W * H;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t p = (size_t)y * W + x;
      Tap t;
      float d[3];
      if (!in_pass(id, n_tris, where, p)) {
        if (fused)
          for (uint32_t ch = 0; ch < n_ch; ++ch) out[ch * n_px + p] = 0.0f;
        continue;
      }
      ray_dir(ray, x, y, d);
      if (!tap_of(d, N, -1, &t)) {
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

/* the fixed tree over one frame: term [9][H][W] float32, smp [H][W] (a pixel contributes) -> row[9] */
void br_tree(int W, int H, const float *term, const uint8_t *smp, float *row) {
  const size_t n_px = (size_t)W * H;
  for (int j = 0; j < 9; ++j) {
    float frame = 0.0f;
    for (int ty = 0; ty < H; ty += 32)
      for (int tx = 0; tx < W; tx += 32) {
        float wave[4];
        for (int w = 0; w < 4; ++w) {
          float v[64], n[64];
          for (int l = 0; l < 64; ++l) {
            const int y = ty + w * 8 + l / 8, x4 = tx + (l % 8) * 4;
            v[l] = 0.0f;
            for (int k = 0; k < 4; ++k)
              if (y < H && x4 + k < W && smp[(size_t)y * W + x4 + k]) v[l] = v[l] + term[j * n_px + (size_t)y * W + x4 + k];
          }
          for (int o = 32; o > 0; o >>= 1) {
            for (int l = 0; l < 64; ++l) n[l] = v[l] + v[l ^ o];
            for (int l = 0; l < 64; ++l) v[l] = n[l];
          }
          wave[w] = v[0];
        }
        frame = frame + (((wave[0] + wave[1]) + wave[2]) + wave[3]);
      }
    row[j] = frame;
  }
}

/* rows [n][9] in order, from +0 -> out[9]: a shared block's frames */
void br_fold(int n, const float *rows, float *out) {
  for (int j = 0; j < 9; ++j) {
    float s = 0.0f;
    for (int i = 0; i < n; ++i) s = s + rows[9 * i + j];
    out[j] = s;
  }
}

/* gout: n_ch planes of W * H (words at pixels outside the pass are never read).  gtex, gabs: [6][N][N][n_ch] doubles, added into;
 * count: [6][N][N], added into (any of the three may be null).  With `term` ([9][H][W] float32, written: 0 where a pixel does not
 * contribute; needs tex): smp [H][W] (written), and the exact sums of the terms gsum[9], of their magnitudes gmag[9] (doubles, added
 * into) and the count of contributing pixels *n_smp (added into). */
static void grad_window(const float *tex, int N, uint32_t n_ch, uint32_t n_tris, int W, int H, const uint32_t *id, const float *ray, int where,
                        const float *gout, double *gtex, double *gabs, uint32_t *count, float *term, uint8_t *smp, double *gsum,
                        double *gmag, uint64_t *n_smp, int x0, int y0, int x1, int y1) {
  const size_t n_px = (size_t)W * H;
  for (int y = y0; y < y1; ++y)
    for (int x = x0; x < x1; ++x) {
      const size_t p = (size_t)y * W + x;
      Tap t;
      float d[3];
      if (term) {
        smp[p] = 0;
        for (int j = 0; j < 9; ++j) term[j * n_px + p] = 0.0f;
      }
      if (!in_pass(id, n_tris, where, p)) continue;
      ray_dir(ray, x, y, d);
      if (!tap_of(d, N, -1, &t)) continue;
      const float wk[4] = {(1.0f - t.tx) * (1.0f - t.ty), t.tx * (1.0f - t.ty), (1.0f - t.tx) * t.ty, t.tx * t.ty};
      for (int k = 0; k < 4; ++k) {
        if (count) count[t.at[k]] += 1u;
        for (uint32_t ch = 0; ch < n_ch; ++ch) {
          const float prod = wk[k] * gout[ch * n_px + p]; /* the float32 product the pass adds */
          if (gtex) gtex[t.at[k] * n_ch + ch] += (double)prod;
          if (gabs) gabs[t.at[k] * n_ch + ch] += fabs((double)prod);
        }
      }
      if (!term) continue;
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
      smp[p] = 1;
      *n_smp += 1u;
      for (int c = 0; c < 3; ++c) {
        const float tm[3] = {g3[c], (float)x * g3[c], (float)y * g3[c]};
        for (int r = 0; r < 3; ++r) {
          term[(3 * r + c) * n_px + p] = tm[r];
          gsum[3 * r + c] += (double)tm[r], gmag[3 * r + c] += fabs((double)tm[r]);
        }
      }
    }
}
void br_grad(const float *tex, int N, uint32_t n_ch, uint32_t n_tris, int W, int H, const uint32_t *id, const float *ray, int where,
             const float *gout, double *gtex, double *gabs, uint32_t *count, float *term, uint8_t *smp, double *gsum, double *gmag,
             uint64_t *n_smp) {
  grad_window(tex, N, n_ch, n_tris, W, H, id, ray, where, gout, gtex, gabs, count, term, smp, gsum, gmag, n_smp, 0, 0, W, H);
}
/* the cube's share of the pixels x0 <= x < x1, y0 <= y < y1 alone (one tile's): gtex, gabs, count as br_grad adds them */
void br_grad_box(const float *tex, int N, uint32_t n_ch, uint32_t n_tris, int W, int H, const uint32_t *id, const float *ray, int where,
                 const float *gout, double *gtex, double *gabs, uint32_t *count, int x0, int y0, int x1, int y1) {
  grad_window(tex, N, n_ch, n_tris, W, H, id, ray, where, gout, gtex, gabs, count, NULL, NULL, NULL, NULL, NULL, x0, y0, x1, y1);
}
