/* The motion pass's test reference (tests/motionref.py builds it with gcc -O2 -ffp-contract=off -fno-fast-math).  It includes nothing
 * of the library: per pixel of a visibility buffer (owner id word, alpha, beta) the point of the owner's triangle IN THE TARGET FRAME
 * under those barycentrics, each component interpolated as the reference's two fragment paths interpolate z,
 *   V (processFragByAVX2, src/Rasterizer.cpp:310-326): gamma = 1 - (alpha + beta); fmaf(alpha, a, fmaf(beta, b, gamma * c));
 *   S (processFragByScalar, src/Rasterizer.cpp:473): gamma = 1 - alpha - beta; alpha * a + beta * b + gamma * c, left to right;
 * fmaf where the reference fuses and nothing else fused.  The flow is that point minus the pixel's corner, the target the words of the
 * target frame's id and z planes at the nearest sample (rintf: round half even), decided inside or outside in float before any
 * conversion to an integer.
 * With -DMOTION_REF_MAIN the same function behind a small program (file in, file out) that tests/test_motion_ref.py runs under
 * AddressSanitizer and UBSan: an index formed from a NaN or a huge coordinate, or a read outside a plane, is a report there. */
#include <math.h>
#include <stdint.h>
#include <stddef.h>

static uint32_t bits(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }

/* out: 5 planes of W * H words — dx dy | z' | tid tz.  A pixel nobody owns (id 0, or an index outside the n_tris triangles): zeros when
 * fused, else its words stay.  pos: n_tris x 9 floats (ax ay z0 bx by z1 cx cy z2) of the TARGET frame; id, al, be: planes 1, 2, 3 of
 * the frame's visibility buffer; tid_plane, tz_plane: planes 1 and 0 of the target frame's, as raw words. */
void mr_motion(const float *pos, uint32_t n_tris, int W, int H, const uint32_t *id, const float *al, const float *be,
               const uint32_t *tid_plane, const uint32_t *tz_plane, int fused, uint32_t *out) {
  const size_t n_px = (size_t)W * (size_t)H;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t p = (size_t)y * W + x;
      const uint32_t w = id[p], idx = (w & 0x7fffffffu) - 1u;
      if (idx >= n_tris) {
        if (fused)
          for (int k = 0; k < 5; ++k) out[k * n_px + p] = 0u;
        continue;
      }
      const float *t = pos + 9 * (size_t)idx;
      const float alpha = al[p], beta = be[p];
      float q[3];
      if (!(w >> 31)) {
        const float gamma = 1.0f - (alpha + beta);
        for (int c = 0; c < 3; ++c) q[c] = fmaf(alpha, t[c], fmaf(beta, t[3 + c], gamma * t[6 + c]));
      } else {
        const float gamma = 1.0f - alpha - beta;
        for (int c = 0; c < 3; ++c) q[c] = alpha * t[c] + beta * t[3 + c] + gamma * t[6 + c];
      }
      const float tx = rintf(q[0]), ty = rintf(q[1]);
      uint32_t tid = 0u, tz = bits(INFINITY);
      if (tx >= 0.0f && tx <= (float)(W - 1) && ty >= 0.0f && ty <= (float)(H - 1)) {
        const size_t at = (size_t)(int)ty * W + (size_t)(int)tx;
        tid = tid_plane[at], tz = tz_plane[at];
      }
      out[0 * n_px + p] = bits(q[0] - (float)x), out[1 * n_px + p] = bits(q[1] - (float)y);
      out[2 * n_px + p] = bits(q[2]);
      out[3 * n_px + p] = tid, out[4 * n_px + p] = tz;
    }
}

#ifdef MOTION_REF_MAIN
/* motion_ref_main IN OUT — IN: uint32 n_tris, W, H, fused; float pos[9 n_tris]; uint32 id, al, be, tid, tz planes [W H] each; uint32
 * prefill[5 W H].  OUT: the 5 planes.  Every array is a heap block of exactly its size. */
#include <stdio.h>
#include <stdlib.h>
static void *take(FILE *f, size_t bytes) {
  void *p = malloc(bytes ? bytes : 1);
  if (!p || fread(p, 1, bytes, f) != bytes) exit(2);
  return p;
}
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t *h = take(f, 16);
  const uint32_t n_tris = h[0];
  const int W = (int)h[1], H = (int)h[2], fused = (int)h[3];
  const size_t plane = sizeof(uint32_t) * (size_t)W * (size_t)H;
  float *pos = take(f, sizeof(float) * 9 * (size_t)n_tris);
  uint32_t *id = take(f, plane);
  float *al = take(f, plane), *be = take(f, plane);
  uint32_t *tid = take(f, plane), *tz = take(f, plane), *out = take(f, 5 * plane);
  fclose(f);
  mr_motion(pos, n_tris, W, H, id, al, be, tid, tz, fused, out);
  FILE *o = fopen(argv[2], "wb");
  if (!o || fwrite(out, 1, 5 * plane, o) != 5 * plane || fclose(o)) return 2;
  free(h), free(pos), free(id), free(al), free(be), free(tid), free(tz), free(out);
  return 0;
}
#endif
