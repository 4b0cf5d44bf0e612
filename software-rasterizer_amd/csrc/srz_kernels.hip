// srz_kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the raster + fragment-shade stage.
//
// Replaces, on the device, the hot loops of TraditionalRasterizer::draw (src/Rasterizer.cpp:183-499 of
// Liupeter01/Software-Rasterizer) and the fragment shaders they call (src/Shader.cpp, include/shader/Shader.hpp).
// Not a translation of the AVX2 code: the reference walks triangles serially and rows in parallel; here
//
//   k_vertex  one thread per face          (optional) the vertex stage, Scene::loadTriangleStream: meshes + matrices → srz_tri
//                                          + the dense copy of its positions
//   k_setup   one thread per triangle      reads the dense positions (36 bytes): bbox (Triangle::calcBoundingBox) + backface
//                                          test → 8-byte BBox, and — per group of 512 triangles, in LDS — the triangles
//                                          sorted by the 32-row bands they reach: binning is O(triangles)
//   k_bin     one WORKGROUP per 32-row band count / scan / fill of the band's own entries into UNORDERED per-tile lists of 4-byte
//                                          triangle indices, LDS atomics only, assembled in LDS and stored as one coalesced run;
//                                          the lists come from a pool sized by what renders need
//   k_clear   ~64 persistent workgroups    on a second stream beside k_raster / k_shade: the fused clear of every tile no
//                                          bbox reaches (16-byte non-temporal stores of +inf / 0), throttled by its grid
//   k_raster  one WAVE per touched tile    VISIBILITY, order-independent: one 64-bit key (depth | tie-break) per pixel in
//                                          LDS, every fragment is a ds_min_u64; the tile's (triangle, pixel) candidates are
//                                          flattened into items (8 pixels of a bbox row / one scalar-tail pixel) and dealt
//                                          densely to the 64 lanes.  Touched tiles nobody owns leave as the fused clear;
//                                          owned tiles write z + owner ids — 16 bits per pixel: the owner's POSITION in the tile's
//                                          triangle list, which rides in the key's tie-break below the triangle index — and append
//                                          themselves (with their list's length and offset) to their frame's work list.
//   k_raster_slow  one wave per listed tile the reference's ORDERED algorithm for what the keys cannot express (NaN / ±0
//                                          depths), for bands that did not fit the pool, and for counting runs.
//   k_peel    one wave per touched tile    (srz_frameset_peel_visibility, in k_raster's place) DEPTH PEELING: per pixel the first
//                                          fragment strictly behind the previous layer's in the visibility order, fed from the
//                                          tile's list or, for bands that did not fit the pool, from the frame's stream.
//   k_shade   one WORKGROUP per owned tile VISIBILITY-FIRST SHADING: each pixel's final owner is shaded exactly once (the
//                                          reference's shaders are pure functions of (triangle,pixel) and its write is an
//                                          overwrite), pixels compacted by semantics class into dense 64-lane chunks; the tile's
//                                          listed triangles are staged in LDS once per tile (LDS-DMA) and read from there by list
//                                          position; 16-byte stores of the 3 colour planes.
//   k_resolve8                             (optional) display(): planes → BGR8.
//
// Numerics: every float op is the oracle's op in the oracle's order (oracle/srz_oracle.c): contraction is OFF,
// fused ops are explicit fmaf(), division and sqrt are the correctly rounded ones (the compiler's IEEE expansions, or
// short sequences proven / checked on the device to return the same bits), pow is evaluated in binary64 and rounded
// once.  The framebuffer is therefore expected to be bit-identical to the oracle's.
#include "srz_device.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#pragma clang fp contract(off)

namespace srz {

// Read-only inputs are read through the CONSTANT address space: wave-uniform addresses become scalar (s_load)
// loads, per-lane ones become invariant loads that never have to be ordered against the framebuffer stores.
#define SRZ_CAS __attribute__((address_space(4)))
template <typename T> __device__ __forceinline__ const SRZ_CAS T *as_const(const T *p) { return (const SRZ_CAS T *)(p); }
// native vector types (HIP's float4/uint2 classes cannot be loaded through an address-space-qualified pointer)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---- operand-order-exact min/max (SSE / std:: semantics, see oracle) ------------------------------------------
__device__ __forceinline__ float sse_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float sse_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float std_max(float a, float b) { return (a < b) ? b : a; }
__device__ __forceinline__ float std_clamp(float v, float lo, float hi) { return (v < lo) ? lo : (hi < v) ? hi : v; }
__device__ __forceinline__ float fmsubf(float a, float b, float c) { return __builtin_fmaf(a, b, -c); }
__device__ __forceinline__ float fmaf_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// ---- exact reciprocal / square root without the compiler's scaling + fix-up scaffolding --------------------------
// For a normal operand with 2^-100 <= |x| <= 2^100 the short sequences below return EXACTLY the correctly rounded
// 1/x and sqrt(x) — verified on MI355X against the IEEE expansions for every one of the 3.37e9 binary32 values in that
// range (k_verify_fastmath, run by tests/test_gpu_fastmath.py).  Operands outside the range (zero, denormal, huge,
// inf, NaN) take the compiler's full IEEE path, so the functions are drop-in equal to `1.0f/x` and `sqrtf(x)`.
__device__ __forceinline__ uint32_t f2u_(float f) { return __builtin_bit_cast(uint32_t, f); }
// (by-value helpers: __builtin_bit_cast applied directly to an ext-vector element reads element 0)
__device__ __forceinline__ float u2f_(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ bool fast_range(float x) { return (((f2u_(x) >> 23) & 0xffu) - 27u) <= 200u; }
__device__ __forceinline__ float rcp_core(float x) { // v_rcp_f32 + one Newton step
  float r = __builtin_amdgcn_rcpf(x);
  return __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
}
__device__ __forceinline__ float sqrt_core(float x) { // x * v_rsq_f32(x) corrected by the exact residual
  float r = __builtin_amdgcn_rsqf(x), s = x * r, h = 0.5f * r; // (one transcendental: they issue at ~0.57x the FMA rate)
  return __builtin_fmaf(__builtin_fmaf(-s, s, x), h, s);
}
// The slow (full IEEE) variants are out-of-line and entered only when SOME lane of the wave has an out-of-range
// operand (wave-uniform branch: no if-conversion, the long expansions are not even fetched in the common case).
__device__ __attribute__((noinline)) float rcp_ieee(float x) { return 1.0f / x; }
__device__ __attribute__((noinline)) float sqrt_ieee(float x) { return __builtin_sqrtf(x); }
__device__ __attribute__((noinline)) float rsqrt2_ieee(float d) { return 1.0f / __builtin_sqrtf(d); }
__device__ __forceinline__ float rcp_rn(float x) {
  if (__ballot(!fast_range(x)) == 0ull) return rcp_core(x);
  return rcp_ieee(x);
}
__device__ __forceinline__ float sqrt_rn(float x) {
  if (__ballot(!(fast_range(x) && x > 0.0f)) == 0ull) return sqrt_core(x);
  return sqrt_ieee(x);
}
// 1.0f / sqrtf(d) with both roundings (sqrt, then reciprocal), as glm::inversesqrt / rcp_ps(sqrt_ps()) compute it
__device__ __forceinline__ float rsqrt2_rn(float d) {
  if (__ballot(!(fast_range(d) && d > 0.0f)) == 0ull) return rcp_core(sqrt_core(d)); // sqrt(d) in [2^-50,2^50]: fast range
  return rsqrt2_ieee(d);
}

// ---- math policies of the shading code ---------------------------------------------------------------------------
// The shaders are written once against a policy M that supplies the correctly rounded 1/x, sqrt(x), 1/sqrt(x):
//   BranchMath  a wave-uniform branch per operation (k_setup / k_raster: one or two operations per thread)
//   FastMath    OPTIMISTIC: always the short exact sequence, the operand checks only accumulate into `bad`; k_shade
//               re-shades the (in practice never taken) chunk with IeeeMath when any lane saw an out-of-range operand.
//               No branches inside the shader, so the independent normalisations of one pixel interleave.
//   IeeeMath    the compiler's full IEEE expansions.
// All three return identical bits wherever FastMath's checks pass (tests/test_gpu_fastmath.py).
__device__ __forceinline__ bool fast_pos(float x) { return ((f2u_(x) >> 23) - 27u) <= 200u; } // fast_range and x > 0
// a / b from y = RN(1/b) (Markstein): q0 = a*y is refined twice with the exact residual a - b*q.  With y correctly rounded
// and q1 within one ulp, RN(q1 + r*y) is the correctly rounded quotient, i.e. exactly what the IEEE division returns,
// PROVIDED nothing under- or overflows on the way: callers guarantee 2^-40 <= |b| <= 2^40 and a == +0 or
// 2^-60 <= |a| <= 2^60 (a -0 numerator would come out as +0).  Checked on device against a / b in tests/test_gpu_fastmath.py.
__device__ __forceinline__ float div_by_rcp(float a, float b, float y) {
  float q = a * y;
  q = __builtin_fmaf(__builtin_fmaf(-b, q, a), y, q);
  return __builtin_fmaf(__builtin_fmaf(-b, q, a), y, q);
}
__device__ __forceinline__ bool div_num_ok(float a) { // (int |, &: no short-circuit branches)
  return ((int)(f2u_(a) == 0u) | (int)((((f2u_(a) >> 23) & 0xffu) - 67u) <= 120u)) != 0;
}
__device__ __forceinline__ bool div_den_ok(float b) { return ((f2u_(b) >> 23) - 87u) <= 80u; } // 2^-40 <= b <= 2^40, b > 0
// sqrt(a^2 + b^2) as the scalar Blinn-Phong computes its attenuation distance (src/Shader.cpp:516-523: std::pow(x, 2) and std::sqrt
// in binary64, rounded once)
__device__ __forceinline__ float len2d_f64(float a, float b) {
  const double dx = (double)a, dy = (double)b;
  return (float)__builtin_sqrt(dx * dx + dy * dy);
}
// The same value without the compiler's binary64 square root (v_rsq_f64 + three refinements + range scaling: ~22 binary64-rate
// instructions per light in every S pixel): two Heron steps in binary64 from the binary32 root,
//   s   = RN64(a^2 + b^2) exactly as the reference has it (both squares are exact in binary64: one fma);
//   r   = the binary32 square root of RN32(s) (sqrt_core: |r - sqrt(s)| < 2^-23.4 r), h = v_rsq_f32 / 2 (|2 h r - 1| < 2^-21.5);
//   R1  = r + (s - r^2) h    : r^2 is exact (48 bits); |R1 - sqrt(s)| < (2^-21.5 * 2^-23.4 + 2^-47.8 + 2^-52) R1 < 2^-44.7 R1
//   R2  = R1 + (s - R1^2) h  : the residual is one fma (a single rounding of the exact s - R1^2); h's error now contributes 2^-66,
//         the dropped second-order term 2^-90: R2 = sqrt(s) up to ITS OWN rounding, i.e. RN64(sqrt(s)) or a neighbour of it.
// RN32(R2) is therefore the reference's RN32(RN64(sqrt(s))) unless a binary32 rounding boundary (the 29 dropped bits =
// 0x10000000) lies within an ulp of R2: `amb` is set within 8 ulps — 3e-8 of the operands — and k_shade hands that tile to the
// generic build like any operand outside FastMath's range.  `sbits` returns the bits of RN32(s) for the range tracking: inside
// [2^-100, 2^101) everything above is normal.  Checked on the device against len2d_f64 (k_verify_fastlen, tests/test_gpu_fastmath.py).
__device__ __forceinline__ float len2d_fast(float a, float b, bool &amb, uint32_t &sbits) {
  const double dx = (double)a, dy = (double)b;
  const double s = __builtin_fma(dx, dx, dy * dy);
  const float sf = (float)s;
  sbits = f2u_(sf);
  const float rs = __builtin_amdgcn_rsqf(sf), r0 = sf * rs, h = 0.5f * rs;
  const float r = __builtin_fmaf(__builtin_fmaf(-r0, r0, sf), h, r0);
  const double R = (double)r, H = (double)h;
  const double R1 = __builtin_fma(__builtin_fma(-R, R, s), H, R);
  const double R2 = __builtin_fma(__builtin_fma(-R1, R1, s), H, R1);
  const uint32_t lo = (uint32_t)__builtin_bit_cast(uint64_t, R2) & 0x1fffffffu;
  amb |= (lo - 0x0ffffff8u) <= 16u; // within 8 binary64 ulps of the binary32 midpoint pattern
  return (float)R2;
}
struct BranchMath {
  __device__ __forceinline__ float rcp(float x) { return rcp_rn(x); }
  __device__ __forceinline__ float sqrt(float x) { return sqrt_rn(x); }
  __device__ __forceinline__ float rsqrt2(float d) { return rsqrt2_rn(d); }
};
struct IeeeMath {
  __device__ __forceinline__ float div255(float a) { return a / 255.0f; }
  __device__ __forceinline__ void div3(float a0, float a1, float a2, float b, float &q0, float &q1, float &q2) {
    q0 = a0 / b, q1 = a1 / b, q2 = a2 / b;
  }
  __device__ __forceinline__ float rcp(float x) { return 1.0f / x; }
  __device__ __forceinline__ float sqrt(float x) { return __builtin_sqrtf(x); }
  __device__ __forceinline__ float rsqrt2(float d) { return 1.0f / __builtin_sqrtf(d); }
  __device__ __forceinline__ float len2d(float a, float b) { return len2d_f64(a, b); }
};
struct FastMath {
  bool bad = false; // (the rare checks: division operands, pow_fast's rounding flag)
  // The operands of the reciprocals / square roots are tracked as the running unsigned minimum and maximum of their bit patterns
  // (two instructions per operand instead of shift + subtract + compare + or; magnitudes for the signed ones) and tested ONCE per
  // pixel: all inside [2^-100, 2^101) <=> lo >= 0x0d800000 and hi <= 0x71ffffff — the criterion of fast_range / fast_pos (a
  // negative, NaN, infinite, zero or denormal operand of a positive-only operation breaks one of the two bounds)
  uint32_t lo = 0x0d800000u, hi = 0x0d800000u;
  __device__ __forceinline__ void track(uint32_t bits) { lo = lo < bits ? lo : bits, hi = hi > bits ? hi : bits; }
  __device__ __forceinline__ bool is_bad() const { return bad | (lo < 0x0d800000u) | (hi > 0x71ffffffu); }
  // texel / 255.0f for texel = 0..255: numerator and divisor are always inside div_by_rcp's range
  __device__ __forceinline__ float div255(float a) { return div_by_rcp(a, 255.0f, __builtin_bit_cast(float, 0x3b808081u)); }
  // three numerators (wave-uniform light intensities) over one positive per-pixel divisor: one reciprocal
  __device__ __forceinline__ void div3(float a0, float a1, float a2, float b, float &q0, float &q1, float &q2) {
    bad |= ((int)div_den_ok(b) & (int)div_num_ok(a0) & (int)div_num_ok(a1) & (int)div_num_ok(a2)) == 0;
    const float y = rcp_core(b);
    q0 = div_by_rcp(a0, b, y), q1 = div_by_rcp(a1, b, y), q2 = div_by_rcp(a2, b, y);
  }
  __device__ __forceinline__ float rcp(float x) {
    track(f2u_(x) & 0x7fffffffu);
    return rcp_core(x);
  }
  __device__ __forceinline__ float sqrt(float x) {
    track(f2u_(x));
    return sqrt_core(x);
  }
  __device__ __forceinline__ float rsqrt2(float d) { // sqrt(d) lies in [2^-50, 2^50]: inside rcp_core's range
    track(f2u_(d));
    return rcp_core(sqrt_core(d));
  }
  // (the scalar path's attenuation distance: two binary64 Heron steps from the binary32 root; an ambiguous rounding → `bad`)
  __device__ __forceinline__ float len2d(float a, float b) {
    uint32_t sb;
    const float d = len2d_fast(a, b, bad, sb);
    track(sb);
    return d;
  }
};
// ApproxMath — the TOLERANCE mode (SRZ_OPT_APPROX_SHADE, opt-in; never the default): the arithmetic CLASS of the reference's own
// x86 path, which shades with approximate instructions — _mm256_rcp_ps (include/shader/Shader.hpp:131, src/Tools.cpp:19,
// include/loader/TextureLoader.hpp:99, src/Rasterizer.cpp:111: 12 bits) and SVML _mm256_pow_ps (include/shader/Shader.hpp:195) —
// on the hardware's own: bare v_rcp_f32 / v_rsq_f32 / v_sqrt_f32 (1 ulp), x^p = v_exp_f32(p * v_log_f32(x)), texel * (1/255), the
// binary64 pieces of the scalar path (the attenuation distance, std::pow) in binary32.  Only k_shade's LIGHTING arithmetic takes it
// (normalisations, attenuation, the power, the texel's scaling): k_raster stays exact, so z, coverage and ownership are
// bit-identical to the oracle in this mode too, and so do the barycentrics and everything interpolated with them.  Nothing can go out of a
// "fast range" here — no operand tracking, no re-shade.  tests/test_gpu_approx.py states the tolerance.
struct ApproxMath {
  __device__ __forceinline__ float div255(float a) { return a * (1.0f / 255.0f); }
  __device__ __forceinline__ void div3(float a0, float a1, float a2, float b, float &q0, float &q1, float &q2) {
    const float y = __builtin_amdgcn_rcpf(b);
    q0 = a0 * y, q1 = a1 * y, q2 = a2 * y;
  }
  // (the one reciprocal of the coverage arithmetic, tri_consts: EXACT — the barycentrics, hence depth, normals' and texture
  // coordinates' interpolation, are the oracle's bits in this mode too: a texture coordinate one ulp off can round to the
  // neighbouring texel, which no colour tolerance covers)
  __device__ __forceinline__ float rcp(float x) { return rcp_rn(x); }
  __device__ __forceinline__ float sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
  __device__ __forceinline__ float rsqrt2(float d) { return __builtin_amdgcn_rsqf(d); }
  __device__ __forceinline__ float len2d(float a, float b) { return __builtin_amdgcn_sqrtf(__builtin_fmaf(a, a, b * b)); }
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  float tx = ax * bx, ty = ay * by, tz = az * bz;
  return tx + ty + tz;
}
// glm::normalize: v * (1/sqrt(dot(v,v)))
template <class M> __device__ __forceinline__ void normalize3(M &m, float &x, float &y, float &z) {
  float is = m.rsqrt2(dot3(x, y, z, x, y, z));
  x = x * is, y = y * is, z = z * is;
}
// NormalSIMD::normalized (src/Tools.cpp:13-24)
template <class M> __device__ __forceinline__ void v_normalized(M &m, float &x, float &y, float &z) {
  float len = m.sqrt(fmaf_(x, x, fmaf_(y, y, z * z)));
  if (len > 0.0f) {
    float inv = m.rcp(len);
    x = x * inv, y = y * inv, z = z * inv;
  } else {
    x = y = z = 0.0f;
  }
}

// FastMath: a squared length inside the fast range has a positive, in-range square root — one check covers both steps
__device__ __forceinline__ void v_normalized(FastMath &m, float &x, float &y, float &z) {
  const float d = fmaf_(x, x, fmaf_(y, y, z * z));
  m.track(f2u_(d));
  const float inv = rcp_core(sqrt_core(d));
  x = x * inv, y = y * inv, z = z * inv;
}

// ApproxMath: one v_rsq_f32; the zero vector stays the zero vector as in NormalSIMD::normalized
__device__ __forceinline__ void v_normalized(ApproxMath &m, float &x, float &y, float &z) {
  const float d = fmaf_(x, x, fmaf_(y, y, z * z));
  const float inv = d > 0.0f ? __builtin_amdgcn_rsqf(d) : 0.0f;
  x = x * inv, y = y * inv, z = z * inv;
}

// pow evaluated in binary64 and rounded once to binary32 (== correctly rounded powf in all but ~1e-7 of cases).
// p is a per-frame constant, so the branch is wave-uniform.
__device__ __forceinline__ float pow_cr(float x, float p) {
  if (p == __builtin_truncf(p) && p >= 0.0f && p <= 1048576.0f) {
    unsigned n = (unsigned)p;
    double b = (double)x, r = 1.0;
    while (n) {
      if (n & 1u) r = r * b;
      b = b * b;
      n >>= 1;
    }
    return (float)r;
  }
  return (float)pow((double)x, (double)p);
}

// x^150 (the reference's Shader::p, src/Shader.cpp:10) as a fixed chain: the very multiplications pow_cr's loop performs
// for n = 150 = 0b10010110, in the same order (r = x^2 · x^4 · x^16 · x^128), without the loop
// x <= 0.5 gives x^150 <= 2^-150, which rounds to +0 in binary32 (2^-150 itself is the tie below the smallest denormal: to
// even = 0): when no lane of the wave is above 0.5 — the half-vector more than 60 degrees off the normal everywhere in the
// chunk, the common case away from a highlight — the chain is skipped.  (A NaN is not "<= 0.5": it takes the chain.)
__device__ __forceinline__ float pow150_cr(float x) {
  if (__ballot(!(x <= 0.5f)) == 0ull) return 0.0f;
  const double b1 = (double)x, b2 = b1 * b1, b4 = b2 * b2, b8 = b4 * b4, b16 = b8 * b8, b32 = b16 * b16, b64 = b32 * b32,
               b128 = b64 * b64;
  double r = b2 * b4;
  r = r * b16;
  r = r * b128;
  return (float)r;
}
// x^n for an integer exponent 0..256 that is the same for the whole wave (a per-frame constant): pow_cr's square-and-multiply
// chain as a SCALAR loop — the very same binary64 multiplications in the same order, no per-lane selects
// (the exponent as an integer already — k_light's host argument; n = 0 gives 1 —, or as the frame's float constant)
__device__ __forceinline__ float pow_int_cr(float x, unsigned n_) {
  unsigned n = (unsigned)__builtin_amdgcn_readfirstlane((int)n_);
  double b = (double)x, r = 1.0;
  while (n) {
    if (n & 1u) r = r * b;
    b = b * b;
    n >>= 1;
  }
  return (float)r;
}
__device__ __forceinline__ float pow_int_cr(float x, float p) { return pow_int_cr(x, (unsigned)p); }
// Compile-time knowledge a shading variant may have (k_shade picks the variant per 64-pixel chunk, wave-uniformly):
//   SH   >= 0: every pixel of the chunk uses shader type SH; -1: per-pixel type (sd.shader)
//   NL   != 0: the frame has exactly |NL| lights (1..4) (decided on the host): the light loop is unrolled, the light constants sit
//              in SGPRs;  0: run-time count.  The sign of NL selects the exponent form (pow_frame)
// x^p for a NON-INTEGER exponent 0 < p <= 4096 (wave-uniform), OPTIMISTICALLY: exp2(p * log2(x)) in binary64 — log by the
// atanh series of (m - 1) / (m + 1) on the mantissa in (sqrt(1/2), sqrt(2)], p * e kept exact, 2^r by its Taylor polynomial —
// about 45 binary64 operations where ocml's correctly rounded pow takes ~210.  Its error is below (2.4 p + 4) ulps of the binary64
// result (log2(m): 7 roundings of 2^-53 on |t| <= 0.5, times p ln 2; the two series' tails are below 2^-55; 2^r: 4 more), so the
// binary32 rounding of the result is the rounding of the exact x^p — hence of any correctly rounded or 1-ulp binary64 pow, the
// oracle's and ocml's alike — unless the result lies within 32 + 4 p binary64 ulps of a binary32 rounding boundary (for
// p = 7.5: 2.3e-7 of the operands) or in the subnormal range: then `amb` is set, and the caller hands the pixel's tile to the
// generic build (pow_cr) exactly like an operand outside FastMath's range.  x = ±0 gives +0 (p is positive and no odd integer),
// a result below 2^-151 rounds to +0; other non-positive, non-finite or NaN operands set `amb`.
// Checked on the device against pow_cr for every binary32 x in (0, 1] at several exponents (k_verify_fastpow, tests/test_gpu_fastmath.py).
__device__ __forceinline__ float pow_fast(float x, float p, bool &amb) {
  const double xd = (double)x;
  const uint64_t xb = __builtin_bit_cast(uint64_t, xd);
  int e = (int)((xb >> 52) & 0x7ffu) - 1023;
  double m = __builtin_bit_cast(double, (xb & 0x000fffffffffffffull) | 0x3ff0000000000000ull); // [1, 2)
  const bool hi = m > 1.4142135623730951;
  m = hi ? m * 0.5 : m, e += hi ? 1 : 0;
  const double f = m - 1.0, g = m + 1.0; // (exact: m has 24 significant bits)
  // s = f / g: reciprocal by Newton, then one correction of the quotient (error < 1 ulp)
  double rg = __builtin_amdgcn_rcp(g);
  rg = __builtin_fma(__builtin_fma(-g, rg, 1.0), rg, rg);
  rg = __builtin_fma(__builtin_fma(-g, rg, 1.0), rg, rg);
  double sq = f * rg;
  sq = __builtin_fma(__builtin_fma(-g, sq, f), rg, sq);
  const double z = sq * sq; // <= 0.02944
  // log(m) = 2 s (1 + z/3 + z^2/5 + ... + z^9/19): the tail is below 2^-53
  double P = 1.0 / 19.0;
  P = __builtin_fma(P, z, 1.0 / 17.0), P = __builtin_fma(P, z, 1.0 / 15.0), P = __builtin_fma(P, z, 1.0 / 13.0);
  P = __builtin_fma(P, z, 1.0 / 11.0), P = __builtin_fma(P, z, 1.0 / 9.0), P = __builtin_fma(P, z, 1.0 / 7.0);
  P = __builtin_fma(P, z, 1.0 / 5.0), P = __builtin_fma(P, z, 1.0 / 3.0), P = __builtin_fma(P, z, 1.0);
  const double t = (2.0 * sq) * P * 1.4426950408889634; // log2(m), |t| <= 0.5
  const double pd = (double)p, yh = pd * (double)e /* exact: 24 x 11 bits */, yl = pd * t;
  const double n = __builtin_rint(yh + yl), r = (yh - n) + yl; // (yh - n is exact), |r| <= 0.5 + tiny
  const double u = r * 0.6931471805599453;
  double Q = 1.0 / 6227020800.0; // exp(u), |u| <= 0.3466: Taylor to u^13 / 13!
  Q = __builtin_fma(Q, u, 1.0 / 479001600.0), Q = __builtin_fma(Q, u, 1.0 / 39916800.0), Q = __builtin_fma(Q, u, 1.0 / 3628800.0);
  Q = __builtin_fma(Q, u, 1.0 / 362880.0), Q = __builtin_fma(Q, u, 1.0 / 40320.0), Q = __builtin_fma(Q, u, 1.0 / 5040.0);
  Q = __builtin_fma(Q, u, 1.0 / 720.0), Q = __builtin_fma(Q, u, 1.0 / 120.0), Q = __builtin_fma(Q, u, 1.0 / 24.0);
  Q = __builtin_fma(Q, u, 1.0 / 6.0), Q = __builtin_fma(Q, u, 0.5), Q = __builtin_fma(Q, u, 1.0), Q = __builtin_fma(Q, u, 1.0);
  const double nc = __builtin_fmax(__builtin_fmin(n, 1000.0), -1000.0); // (keeps ldexp's exponent an int)
  const double res = __builtin_ldexp(Q, (int)nc);
  const uint32_t lo = (uint32_t)__builtin_bit_cast(uint64_t, res) & 0x1fffffffu; // the 29 bits binary32 drops
  const uint32_t dist = lo > 0x10000000u ? lo - 0x10000000u : 0x10000000u - lo; // to the rounding boundary, in binary64 ulps
  const bool zero_in = (__builtin_bit_cast(uint32_t, x) << 1) == 0u;            // x = ±0
  const bool tiny = res < 0x1p-151, normal = res >= 0x1p-120 && res < 0x1p+120;
  const bool okx = x > 0.0f && x < __builtin_inff();
  const uint32_t safe = 32u + (uint32_t)(4.0f * p); // (scalar: p is wave-uniform)
  amb |= !(zero_in | (okx & (tiny | (normal & (dist > safe)))));
  return (zero_in | tiny) ? 0.0f : (float)res;
}

// The exponent forms of the shading builds (NL = the build's compile-time light count, see k_shade):
//   NL > 0  an integer exponent 0 <= p <= 256 (decided on the host): the fixed chain for p = 150 (the value the reference ships,
//           src/Shader.cpp:10) or the scalar square-and-multiply loop
//   NL < 0  a non-integer exponent in (0, 4096] (Shader::p is a mutable static in the reference: any value is legal): pow_fast,
//           whose ambiguous cases the FastMath pass's `bad` flag takes to the generic build
//   NL = 0  the generic build, every other exponent: pow_cr
// x^p in the tolerance mode: exp2(p * log2 x) on the transcendental unit (x >= 0 here: a clamped cosine; x = 0 → log2 = -inf →
// +0 for p > 0).  p = 0 (wave-uniform) is 1 whatever x, as pow() has it
__device__ __forceinline__ float pow_approx(float x, float p) {
  if (p == 0.0f) return 1.0f;
  return __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(x));
}
template <int NL, class M> __device__ __forceinline__ float pow_frame(M &m, float x, float p) {
  if constexpr (std::is_same<M, ApproxMath>::value) {
    return pow_approx(x, p);
  } else if constexpr (NL > 0) {
    return p == 150.0f ? pow150_cr(x) : pow_int_cr(x, p); // (wave-uniform branch: p is a per-frame scalar)
  } else if constexpr (NL < 0 && std::is_same<M, FastMath>::value) {
    return pow_fast(x, p, m.bad); // (the host sends only frames with a non-integer exponent in (0, 4096] to these builds)
  } else {
    return pow_cr(x, p);
  }
}
template <int NL> constexpr int light_count() { return NL < 0 ? -NL : NL; } // lights known at compile time (0: run-time count)

__device__ __forceinline__ int32_t cvt_rne_i32(float f) {
  if (!(f >= -2147483648.0f && f < 2147483648.0f)) return INT32_MIN;
  return (int32_t)__builtin_rintf(f);
}
// (int)f as x86 has it (cvttss2si, the reference's build): truncation; NaN and everything outside int32 give INT32_MIN.  The
// device's own conversion saturates and turns a NaN into 0 — texel (0, 0) where the reference's index check says "black"
__device__ __forceinline__ int32_t cvt_trunc_i32(float f) {
  if (!(f >= -2147483648.0f && f < 2147483648.0f)) return INT32_MIN;
  return (int32_t)f;
}

// ---- per-triangle constants used by both the coverage test and the shader -----------------------------------
struct TriXY {
  float ax, ay, bx, by, cx, cy, z0, z1, z2;
  float v_inv;  // 1 / fmsub(ABx,ACy,ACx*ABy)   — "V" (8-wide) path, src/Rasterizer.cpp:111-112
  float s_area; // ABx*ACy - ABy*ACx              — "S" (scalar tail) path, src/Rasterizer.cpp:61
};
template <class M> __device__ __forceinline__ void tri_consts(M &m, TriXY &t) {
  float ABx = t.bx - t.ax, ABy = t.by - t.ay, ACx = t.cx - t.ax, ACy = t.cy - t.ay;
  t.v_inv = m.rcp(fmsubf(ABx, ACy, ACx * ABy));
  t.s_area = ABx * ACy - ABy * ACx;
}

// "V" semantics: barycentric(__m256) + inside mask + z (src/Rasterizer.cpp:89-127,310-326)
__device__ __forceinline__ bool cover_v(const TriXY &t, float fx, float fy, float &alpha, float &beta, float &gamma,
                                        float &z) {
  float PBx = t.bx - fx, PBy = t.by - fy, PCx = t.cx - fx, PCy = t.cy - fy, PAx = t.ax - fx, PAy = t.ay - fy;
  float aPBC = fmsubf(PBx, PCy, PCx * PBy), aPCA = fmsubf(PCx, PAy, PAx * PCy);
  alpha = aPBC * t.v_inv, beta = aPCA * t.v_inv, gamma = 1.0f - (alpha + beta);
  z = fmaf_(alpha, t.z0, fmaf_(beta, t.z1, gamma * t.z2));
  return alpha > 0.0f && alpha < 1.0f && beta > 0.0f && beta < 1.0f && gamma > 0.0f && gamma < 1.0f;
}
// "S" semantics: insideTriangle + barycentric(scalar) + z (src/Rasterizer.cpp:11-70,473)
__device__ __forceinline__ bool cover_s(const TriXY &t, float fx, float fy, float &alpha, float &beta, float &gamma,
                                        float &z) {
  float ABx = t.bx - t.ax, ABy = t.by - t.ay, BCx = t.cx - t.bx, BCy = t.cy - t.by, CAx = t.ax - t.cx, CAy = t.ay - t.cy;
  float APx = fx - t.ax, APy = fy - t.ay, BPx = fx - t.bx, BPy = fy - t.by, CPx = fx - t.cx, CPy = fy - t.cy;
  float e0 = ABx * APy - ABy * APx, e1 = BCx * BPy - BCy * BPx, e2 = CAx * CPy - CAy * CPx;
  bool inside = (e0 > 0 && e1 > 0 && e2 > 0) || (e0 < 0 && e1 < 0 && e2 < 0);
  float PAx = t.ax - fx, PAy = t.ay - fy, PBx = t.bx - fx, PBy = t.by - fy, PCx = t.cx - fx, PCy = t.cy - fy;
  float aPBC = PBx * PCy - PBy * PCx, aPCA = PCx * PAy - PCy * PAx;
  alpha = aPBC / t.s_area, beta = aPCA / t.s_area, gamma = 1.0f - alpha - beta;
  z = alpha * t.z0 + beta * t.z1 + gamma * t.z2;
  return inside;
}

// ================================================================================================================
// k_vertex — the vertex stage, Scene::loadTriangleStream (src/Scene.cpp:927-958): one thread per face.
//   pos' = to_vec3(NDC_MVP * (p,1)) ; pos'.z = pos'.z*scale + offset ; nrm' = to_vec3(Normal_M * (n,1)) ; uv copied
// glm's operator*(mat4,vec4) order: (m0*v.x + m1*v.y) + (m2*v.z + m3*v.w); Tools::to_vec3 divides by w (src/Tools.cpp:74-76).
// ================================================================================================================
// (the four rows before the division: k_vertex_grad differentiates them, and needs their bits)
__device__ __forceinline__ void xform_rows(const SRZ_CAS float *m, float x, float y, float z, float (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float add0 = m[0 * 4 + i] * x + m[1 * 4 + i] * y;
    const float add1 = m[2 * 4 + i] * z + m[3 * 4 + i]; // * 1.0f is exact
    r[i] = add0 + add1;
  }
}
__device__ __forceinline__ void xform_div_w(const SRZ_CAS float *m, float x, float y, float z, float &ox, float &oy, float &oz) {
  float r[4];
  xform_rows(m, x, y, z, r);
  ox = r[0] / r[3], oy = r[1] / r[3], oz = r[2] / r[3];
}

// Per triangle: finite check, backface test, bounding box (src/Triangle.cpp:147-151,243-257; Rasterizer.cpp:203) — shared by
// k_setup (uploaded streams) and k_vertex (scenesets: the triangle is still in registers).  Returns "kept"; a culled or
// non-finite triangle gets the empty box.
__device__ __forceinline__ bool setup_triangle(const float (&P)[9], int W, int H, float ex, float ey, float ez, bool live, BBox &bb) {
  const float A0 = P[0], A1 = P[1], A2 = P[2], B0 = P[3], B1 = P[4], B2 = P[5], C0 = P[6], C1 = P[7], C2 = P[8];
  bb.sx = 1, bb.sy = 1, bb.ex = 0, bb.ey = 0;
  const bool finite = live && __builtin_isfinite(A0) && __builtin_isfinite(A1) && __builtin_isfinite(A2) && __builtin_isfinite(B0) &&
                      __builtin_isfinite(B1) && __builtin_isfinite(B2) && __builtin_isfinite(C0) && __builtin_isfinite(C1) &&
                      __builtin_isfinite(C2);
  bool keep = false;
  if (finite) {
    float e1x = B0 - A0, e1y = B1 - A1, e1z = B2 - A2, e2x = C0 - A0, e2y = C1 - A1, e2z = C2 - A2;
    float nx = e1y * e2z - e2y * e1z, ny = e1z * e2x - e2z * e1x, nz = e1x * e2y - e2x * e1y;
    BranchMath bm;
    normalize3(bm, nx, ny, nz);
    keep = !(dot3(nx, ny, nz, ex, ey, ez) > 0.0f);
  }
  if (keep) {
    float mnx = A0, mxx = A0, mny = A1, mxy = A1;
    if (B0 < mnx) mnx = B0;
    if (C0 < mnx) mnx = C0;
    if (mxx < B0) mxx = B0;
    if (mxx < C0) mxx = C0;
    if (B1 < mny) mny = B1;
    if (C1 < mny) mny = C1;
    if (mxy < B1) mxy = B1;
    if (mxy < C1) mxy = C1;
    // clamp(trunc(v),0,W-1) == trunc(clamp(v,0,W-1)) for every finite v
    bb.sx = (int16_t)(int)std_clamp(mnx, 0.0f, (float)(W - 1));
    bb.ex = (int16_t)(int)std_clamp(mxx, 0.0f, (float)(W - 1));
    bb.sy = (int16_t)(int)std_clamp(mny, 0.0f, (float)(H - 1));
    bb.ey = (int16_t)(int)std_clamp(mxy, 0.0f, (float)(H - 1));
  }
  return keep;
}

// A 12-byte piece of the dense position stream (9 floats per triangle, srz_device.h), moved three floats at a time
// (global_load_dwordx3 / global_store_dwordx3 or wider: dword alignment is all they need)
struct F3 {
  float x, y, z;
};
__device__ __forceinline__ F3 ld3(const SRZ_CAS float *p) { return F3{p[0], p[1], p[2]}; } // (one global_load_dwordx3)
// the 9 position floats of triangle i (ax ay z0 bx by z1 cx cy z2)
__device__ __forceinline__ void load_pos9(const SRZ_CAS float *p, float (&P)[9]) {
  const F3 v0 = ld3(p), v1 = ld3(p + 3), v2 = ld3(p + 6);
  P[0] = v0.x, P[1] = v0.y, P[2] = v0.z, P[3] = v1.x, P[4] = v1.y, P[5] = v1.z, P[6] = v2.x, P[7] = v2.y, P[8] = v2.z;
}

// (bbox_out != null: the triangle's setup — cull + bounding box — is done here too, from the registers that hold it; k_chunks
// then only reduces the boxes to the chunks' row ranges and the 96-byte triangles are not read back by a k_setup)
__global__ __launch_bounds__(256) void k_vertex(const DrawDesc *draws, srz_tri *tris, float *tri_pos, const FrameDesc *frames, BBox *bbox_out) {
  const SRZ_CAS DrawDesc *d = as_const(draws) + blockIdx.y;
  const uint32_t n_faces = d->n_faces;
  const SRZ_CAS srz_vertex *verts = as_const(d->verts);
  const SRZ_CAS uint32_t *faces = as_const(d->faces);
  const float zs = d->zscale, zo = d->zoffset;
  for (uint32_t f = blockIdx.x * 256 + threadIdx.x; f < n_faces; f += gridDim.x * 256) {
    srz_tri t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const SRZ_CAS srz_vertex *v = verts + faces[3 * f + k];
      const float px = v->pos[0], py = v->pos[1], pz = v->pos[2], nx = v->nrm[0], ny = v->nrm[1], nz = v->nrm[2];
      float x, y, z;
      xform_div_w(d->ndc_mvp, px, py, pz, x, y, z);
      t.pos[k][0] = x, t.pos[k][1] = y, t.pos[k][2] = z * zs + zo;
      xform_div_w(d->normal_m, nx, ny, nz, x, y, z);
      t.nrm[k][0] = x, t.nrm[k][1] = y, t.nrm[k][2] = z;
      t.uv[k][0] = v->uv[0], t.uv[k][1] = v->uv[1];
    }
    const size_t ti = (size_t)d->tri_off + f;
    tris[ti] = t;
    const float P[9] = {t.pos[0][0], t.pos[0][1], t.pos[0][2], t.pos[1][0], t.pos[1][1], t.pos[1][2], t.pos[2][0], t.pos[2][1], t.pos[2][2]};
    F3 *po = reinterpret_cast<F3 *>(tri_pos + ti * TRI_POS_F); // (the dense copy of the positions: what k_setup and k_raster read)
    po[0] = F3{P[0], P[1], P[2]}, po[1] = F3{P[3], P[4], P[5]}, po[2] = F3{P[6], P[7], P[8]};
    if (bbox_out) {
      const SRZ_CAS FrameDesc *fd = as_const(frames) + d->frame;
      BBox bb;
      (void)setup_triangle(P, fd->width, fd->height, fd->eye[0], fd->eye[1], fd->eye[2], true, bb);
      bbox_out[ti] = bb;
    }
  }
}

// ================================================================================================================
// Wave-level scans on the DPP crossbar (no LDS traffic): inclusive prefix over the 64 lanes.
// row_shr:1,2,4,8 scan inside each row of 16 lanes (lanes without a source read the identity 0), row_bcast:15 / :31
// carry the row totals into the rows behind.
// ================================================================================================================
#define SRZ_DPP(v, ctrl, rmask) (uint32_t) __builtin_amdgcn_update_dpp(0, (int)(v), ctrl, rmask, 0xf, false)
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
  v += SRZ_DPP(v, 0x111, 0xf), v += SRZ_DPP(v, 0x112, 0xf), v += SRZ_DPP(v, 0x114, 0xf), v += SRZ_DPP(v, 0x118, 0xf);
  v += SRZ_DPP(v, 0x142, 0xa); // row_bcast:15 → rows 1 and 3
  v += SRZ_DPP(v, 0x143, 0xc); // row_bcast:31 → rows 2 and 3
  return v;
}
__device__ __forceinline__ uint32_t wave_scan_max(uint32_t v) {
  v = max(v, SRZ_DPP(v, 0x111, 0xf)), v = max(v, SRZ_DPP(v, 0x112, 0xf)), v = max(v, SRZ_DPP(v, 0x114, 0xf));
  v = max(v, SRZ_DPP(v, 0x118, 0xf));
  v = max(v, SRZ_DPP(v, 0x142, 0xa));
  v = max(v, SRZ_DPP(v, 0x143, 0xc));
  return v;
}
// (float32 adds over the same control words; a lane without a source adds +0: lane 63 ends up with the wave's sum, one fixed tree)
#define SRZ_DPP_F(v, ctrl, rmask) __uint_as_float(SRZ_DPP(__float_as_uint(v), ctrl, rmask))
__device__ __forceinline__ float wave_scan_addf(float v) {
  v += SRZ_DPP_F(v, 0x111, 0xf), v += SRZ_DPP_F(v, 0x112, 0xf), v += SRZ_DPP_F(v, 0x114, 0xf), v += SRZ_DPP_F(v, 0x118, 0xf);
  v += SRZ_DPP_F(v, 0x142, 0xa);
  v += SRZ_DPP_F(v, 0x143, 0xc);
  return v;
}

// ================================================================================================================
// k_positions — srz_frameset_positions: frame blockIdx.y's triangles of the dense position stream, float by float, into the caller's
// [frame][pos_tris][9]; the floats behind the frame's last triangle are +0.
// ================================================================================================================
__global__ __launch_bounds__(256) void k_positions(const FrameDesc *frames, const float *tri_pos, uint32_t pos_stride, float *out, uint32_t pos_tris) {
  const SRZ_CAS FrameDesc *fd = as_const(frames) + blockIdx.y;
  const uint32_t n_tris = fd->n_tris;
  const size_t n = (size_t)pos_tris * TRI_POS_F;
  const float *src = tri_pos + (size_t)fd->tri_off * pos_stride;
  float *dst = out + (size_t)blockIdx.y * n;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const size_t t = e / TRI_POS_F;
    dst[e] = t < n_tris ? src[t * pos_stride + (e - t * TRI_POS_F)] : 0.0f;
  }
}

// ================================================================================================================
// k_vertex_grad — srz_sceneset_vertex_grad, the backward of k_vertex for one mesh slot (include/srz.h states the rule).
// Grid (blocks of 256 vertices, frames); a thread OWNS (frame, vertex) and walks the frame's draws of the slot in draw order — the loop
// and every barrier in it are block-uniform, so a thread past the last vertex stays and contributes nothing.
//   gverts: a GATHER.  Per draw the thread sums the gpos floats of its vertex's corners in list order (3 * corner is the float's
//     index behind the draw's first triangle), differentiates the transform — xform_rows is k_vertex's own expression — and adds
//     into a register copy of its three floats, which is stored once: no atomics, bit-reproducible.
//   gdraw: 18 values per draw, reduced on chip — across the wave on the DPP crossbar, across the four waves through LDS — then ONE
//     float add per workgroup, draw and value (no-return global_atomic_add_f32), and none for a draw no vertex of the workgroup
//     contributes to.
// ================================================================================================================
__global__ __launch_bounds__(256) void k_vertex_grad(const VertexGradArgs a) {
  __shared__ float s_part[4][VG_VALS];
  __shared__ uint32_t s_any[4];
  const uint32_t f = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t v = blockIdx.x * 256 + tid;
  const bool live = v < a.n_verts;
  const SRZ_CAS FrameDesc *fd = as_const(a.frames) + f;
  const uint32_t n_draws = fd->n_batches, draw0 = fd->batch_off, tri0 = fd->tri_off;
  uint32_t c_begin = 0, c_end = 0;
  float P[3] = {0.0f, 0.0f, 0.0f};
  if (live) {
    c_begin = a.corner_off[v], c_end = a.corner_off[v + 1];
    P[0] = a.verts[v].pos[0], P[1] = a.verts[v].pos[1], P[2] = a.verts[v].pos[2];
  }
  const float *gpos_f = a.gpos + (size_t)f * a.gpos_stride;
  float *gv = a.gverts && live ? a.gverts + ((size_t)f * a.n_verts + v) * 3 : nullptr;
  float acc[3] = {0.0f, 0.0f, 0.0f};
  bool touched = false;
  for (uint32_t j = 0; j < n_draws; ++j) {
    const SRZ_CAS DrawDesc *d = as_const(a.draws) + draw0 + j;
    if (d->verts != a.verts) continue; // (another slot's draw)
    const float *gp = gpos_f + (size_t)(d->tri_off - tri0) * TRI_POS_F;
    float GX = 0.0f, GY = 0.0f, GZ = 0.0f;
    for (uint32_t c = c_begin; c < c_end; ++c) {
      const float *p = gp + (size_t)a.corners[c] * 3;
      GX = GX + p[0], GY = GY + p[1], GZ = GZ + p[2];
    }
    const bool contrib = live && !(GX == 0.0f && GY == 0.0f && GZ == 0.0f); // (a NaN is not 0 and goes on)
    float val[VG_VALS];
#pragma unroll
    for (uint32_t e = 0; e < VG_VALS; ++e) val[e] = 0.0f;
    if (contrib) {
      float r[4], g[4];
      xform_rows(d->ndc_mvp, P[0], P[1], P[2], r);
      const float X = r[0] / r[3], Y = r[1] / r[3], Q = r[2] / r[3], inv = 1.0f / r[3], gq = GZ * d->zscale;
      g[0] = GX * inv, g[1] = GY * inv, g[2] = gq * inv;
      float s = gq * Q;
      s = fmaf(GY, Y, s), s = fmaf(GX, X, s);
      g[3] = (-s) * inv;
      if (gv) {
        if (!touched) acc[0] = gv[0], acc[1] = gv[1], acc[2] = gv[2], touched = true;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float t = d->ndc_mvp[4 * c] * g[0];
          t = fmaf(d->ndc_mvp[4 * c + 1], g[1], t), t = fmaf(d->ndc_mvp[4 * c + 2], g[2], t), t = fmaf(d->ndc_mvp[4 * c + 3], g[3], t);
          acc[c] = acc[c] + t;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) val[i] = g[i] * P[0], val[4 + i] = g[i] * P[1], val[8 + i] = g[i] * P[2], val[12 + i] = g[i];
      val[16] = GZ * Q, val[17] = GZ;
    }
    if (a.gdraw) {
      const bool wave_any = __ballot(contrib) != 0ull;
#pragma unroll
      for (uint32_t e = 0; e < VG_VALS; ++e) val[e] = wave_scan_addf(val[e]);
      if (lane == 63u) {
#pragma unroll
        for (uint32_t e = 0; e < VG_VALS; ++e) s_part[wave][e] = val[e];
        s_any[wave] = wave_any ? 1u : 0u;
      }
      __syncthreads();
      if (tid < VG_VALS && (s_any[0] | s_any[1] | s_any[2] | s_any[3]) != 0u)
        unsafeAtomicAdd(a.gdraw + ((size_t)f * a.draw_stride + j) * VG_VALS + tid,
                        (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]));
      __syncthreads();
    }
  }
  if (touched) gv[0] = acc[0], gv[1] = acc[1], gv[2] = acc[2];
}

// ================================================================================================================
// k_mesh_normals / k_mesh_normals_grad — srz_mesh_normals and its backward (include/srz.h states the rules).  Grid (blocks of 256
// vertices, position sets); a thread OWNS (set, vertex) and walks the vertex's corner list: a gather, no atomics, no barrier, plain
// stores, bit-reproducible.  A face's normal is computed in the face's OWN vertex order whichever corner asks, so the three vertices
// of a face add the same bits.  The backward is two launches of one kernel: PHASE 1 recomputes S, r, n per vertex and stores
// gS = (g - n (n . g)) r (0 where the vertex was not normalised) into `work`; PHASE 2 gathers, per corner of the vertex, the
// face's G = (gS[i0] + gS[i1]) + gS[i2] crossed with the opposite edge.
// ================================================================================================================
__device__ __forceinline__ F3 ldv3(const float *p) { return F3{p[0], p[1], p[2]}; } // (ld3 for memory the pass may also write)
__device__ __forceinline__ F3 sub3(F3 a, F3 b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ F3 add3(F3 a, F3 b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ F3 cross3(F3 u, F3 w) { return F3{u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x}; }
// S of the rule: the sum over the vertex's corners, in list order, of the face normals of position set `p`
__device__ __forceinline__ F3 normal_sum(const MeshNormalsArgs &a, const float *p, uint32_t c_begin, uint32_t c_end) {
  F3 S{0.0f, 0.0f, 0.0f};
  for (uint32_t c = c_begin; c < c_end; ++c) {
    const uint32_t *f = a.faces + (size_t)(a.corners[c] / 3u) * 3;
    const F3 p0 = ldv3(p + (size_t)f[0] * a.pos_stride);
    S = add3(S, cross3(sub3(ldv3(p + (size_t)f[1] * a.pos_stride), p0), sub3(ldv3(p + (size_t)f[2] * a.pos_stride), p0)));
  }
  return S;
}
// r = 1 / sqrt(S . S) where the vertex is normalised (IeeeMath::rsqrt2's expression), else false: no face, degenerate faces only,
// NaN, overflow
__device__ __forceinline__ bool normal_scale(F3 S, float &r) {
  const float len2 = dot3(S.x, S.y, S.z, S.x, S.y, S.z);
  const bool ok = len2 > 0.0f && len2 <= __FLT_MAX__;
  r = ok ? 1.0f / __builtin_sqrtf(len2) : 0.0f;
  return ok;
}
__global__ __launch_bounds__(256) void k_mesh_normals(const MeshNormalsArgs a) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x, set = blockIdx.y;
  if (v >= a.n_verts) return;
  const size_t at = (size_t)set * a.n_verts + v;
  const F3 S = normal_sum(a, a.pos + (size_t)set * a.n_verts * a.pos_stride, a.corner_off[v], a.corner_off[v + 1]);
  float r;
  const bool ok = normal_scale(S, r);
  float *n = a.nrm + at * a.nrm_stride;
  n[0] = ok ? S.x * r : 0.0f, n[1] = ok ? S.y * r : 0.0f, n[2] = ok ? S.z * r : 0.0f;
}
template <int PHASE> __global__ __launch_bounds__(256) void k_mesh_normals_grad(const MeshNormalsArgs a) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x, set = blockIdx.y;
  if (v >= a.n_verts) return;
  const size_t at = (size_t)set * a.n_verts + v;
  const float *p = a.pos + (size_t)set * a.n_verts * a.pos_stride;
  const uint32_t c_begin = a.corner_off[v], c_end = a.corner_off[v + 1];
  if (PHASE == 1) {
    const F3 S = normal_sum(a, p, c_begin, c_end);
    float r;
    F3 gS{0.0f, 0.0f, 0.0f};
    if (normal_scale(S, r)) {
      const F3 n{S.x * r, S.y * r, S.z * r}, g = ldv3(a.gnrm + at * a.gnrm_stride);
      const float d = dot3(n.x, n.y, n.z, g.x, g.y, g.z);
      gS = F3{(g.x - n.x * d) * r, (g.y - n.y * d) * r, (g.z - n.z * d) * r};
    }
    float *w = a.work + at * 3;
    w[0] = gS.x, w[1] = gS.y, w[2] = gS.z;
  } else {
    const float *gs = a.work + (size_t)set * a.n_verts * 3;
    F3 acc{0.0f, 0.0f, 0.0f};
    for (uint32_t c = c_begin; c < c_end; ++c) {
      const uint32_t corner = a.corners[c], face = corner / 3u, k = corner - 3u * face;
      const uint32_t *f = a.faces + (size_t)face * 3;
      const uint32_t i0 = f[0], i1 = f[1], i2 = f[2];
      const F3 A = ldv3(p + (size_t)i0 * a.pos_stride), B = ldv3(p + (size_t)i1 * a.pos_stride), C = ldv3(p + (size_t)i2 * a.pos_stride);
      const F3 G = add3(add3(ldv3(gs + (size_t)i0 * 3), ldv3(gs + (size_t)i1 * 3)), ldv3(gs + (size_t)i2 * 3));
      const F3 term = k == 0u ? cross3(sub3(B, C), G) : k == 1u ? cross3(sub3(C, A), G) : cross3(G, sub3(B, A));
      acc = add3(acc, term);
    }
    float *g = a.gpos + at * 3;
    g[0] = acc.x, g[1] = acc.y, g[2] = acc.z;
  }
}

// ================================================================================================================
// k_mesh_tangents / k_mesh_tangents_grad — srz_mesh_tangents and its backward (include/srz.h states the rules): k_mesh_normals'
// shape — grid (blocks of 256 vertices, position sets), a thread OWNS (set, vertex) and walks the vertex's corner list, a gather, no
// atomics, no barrier, plain stores, bit-reproducible.  A face's uv-area-weighted tangent s * Tf and its det are computed in the
// face's OWN vertex order whichever corner asks.  The uv are ONE set shared by the position sets.  The backward goes to the
// positions only (uv, s and w are held): PHASE 1 stores gS = (g - t (t . g)) r per vertex into `work`, PHASE 2 gathers, per corner
// of the vertex, the face's G = (gS[i0] + gS[i1]) + gS[i2] times the corner's uv coefficient — no position is read there.
// ================================================================================================================
struct FaceUv {
  float dv1, dv2, det, s;
};
__device__ __forceinline__ FaceUv face_uv(const MeshTangentsArgs &a, const uint32_t *f) {
  const float *q0 = a.uv + (size_t)f[0] * a.uv_stride, *q1 = a.uv + (size_t)f[1] * a.uv_stride, *q2 = a.uv + (size_t)f[2] * a.uv_stride;
  const float u0 = q0[0], v0 = q0[1];
  const float du1 = q1[0] - u0, dv1 = q1[1] - v0, du2 = q2[0] - u0, dv2 = q2[1] - v0;
  const float det = du1 * dv2 - du2 * dv1;
  return FaceUv{dv1, dv2, det, det < 0.0f ? -1.0f : 1.0f};
}
// S and D of the rule: the sums over the vertex's corners, in list order, of s * Tf and of det, for position set `p`
__device__ __forceinline__ F3 tangent_sum(const MeshTangentsArgs &a, const float *p, uint32_t c_begin, uint32_t c_end, float &D) {
  F3 S{0.0f, 0.0f, 0.0f};
  D = 0.0f;
  for (uint32_t c = c_begin; c < c_end; ++c) {
    const uint32_t *f = a.faces + (size_t)(a.corners[c] / 3u) * 3;
    const F3 p0 = ldv3(p + (size_t)f[0] * a.pos_stride);
    const F3 e1 = sub3(ldv3(p + (size_t)f[1] * a.pos_stride), p0), e2 = sub3(ldv3(p + (size_t)f[2] * a.pos_stride), p0);
    const FaceUv q = face_uv(a, f);
    const F3 Tf{e1.x * q.dv2 - e2.x * q.dv1, e1.y * q.dv2 - e2.y * q.dv1, e1.z * q.dv2 - e2.z * q.dv1};
    S = add3(S, F3{q.s * Tf.x, q.s * Tf.y, q.s * Tf.z});
    D = D + q.det;
  }
  return S;
}
__global__ __launch_bounds__(256) void k_mesh_tangents(const MeshTangentsArgs a) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x, set = blockIdx.y;
  if (v >= a.n_verts) return;
  const size_t at = (size_t)set * a.n_verts + v;
  float D, r;
  const F3 S = tangent_sum(a, a.pos + (size_t)set * a.n_verts * a.pos_stride, a.corner_off[v], a.corner_off[v + 1], D);
  const bool ok = normal_scale(S, r);
  float *t = a.tan + at * a.tan_stride;
  t[0] = ok ? S.x * r : 0.0f, t[1] = ok ? S.y * r : 0.0f, t[2] = ok ? S.z * r : 0.0f, t[3] = D < 0.0f ? -1.0f : 1.0f;
}
template <int PHASE> __global__ __launch_bounds__(256) void k_mesh_tangents_grad(const MeshTangentsArgs a) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x, set = blockIdx.y;
  if (v >= a.n_verts) return;
  const size_t at = (size_t)set * a.n_verts + v;
  const uint32_t c_begin = a.corner_off[v], c_end = a.corner_off[v + 1];
  if (PHASE == 1) {
    float D, r;
    const F3 S = tangent_sum(a, a.pos + (size_t)set * a.n_verts * a.pos_stride, c_begin, c_end, D);
    F3 gS{0.0f, 0.0f, 0.0f};
    if (normal_scale(S, r)) {
      const F3 t{S.x * r, S.y * r, S.z * r}, g = ldv3(a.gtan + at * a.gtan_stride);
      const float d = dot3(t.x, t.y, t.z, g.x, g.y, g.z);
      gS = F3{(g.x - t.x * d) * r, (g.y - t.y * d) * r, (g.z - t.z * d) * r};
    }
    float *w = a.work + at * 3;
    w[0] = gS.x, w[1] = gS.y, w[2] = gS.z;
  } else {
    const float *gs = a.work + (size_t)set * a.n_verts * 3;
    F3 acc{0.0f, 0.0f, 0.0f};
    for (uint32_t c = c_begin; c < c_end; ++c) {
      const uint32_t corner = a.corners[c], face = corner / 3u, k = corner - 3u * face;
      const uint32_t *f = a.faces + (size_t)face * 3;
      const F3 G = add3(add3(ldv3(gs + (size_t)f[0] * 3), ldv3(gs + (size_t)f[1] * 3)), ldv3(gs + (size_t)f[2] * 3));
      const FaceUv q = face_uv(a, f);
      const float co = k == 0u ? q.s * (q.dv1 - q.dv2) : k == 1u ? q.s * q.dv2 : -(q.s * q.dv1);
      acc = add3(acc, F3{G.x * co, G.y * co, G.z * co});
    }
    float *g = a.gpos + at * 3;
    g[0] = acc.x, g[1] = acc.y, g[2] = acc.z;
  }
}

// ================================================================================================================
// k_mesh_laplacian — srz_mesh_laplacian and srz_mesh_laplacian_grad (include/srz.h states the rules): k_mesh_normals' shape — a
// thread OWNS (set, vertex) and walks the vertex's corner list, a gather, no atomics, no barrier, no LDS, plain stores,
// bit-reproducible.  Grid (blocks of 256 vertices, sets, chunks of LAP_CHUNK channels): the thread keeps its chunk's sums in
// registers; a COTAN thread recomputes the face's weights for its chunk (nine position loads the sixteen chunks of a 64-channel
// field share through the cache; no workspace, no second launch).  MODE 0 .. 2 are the kinds; MODE 3 is UMBRELLA's transpose —
// GRAPH and COTAN are symmetric, their backward is the forward kernel over gout.  corner_off, corners and faces are indexed per
// lane (nothing is wave-uniform: vector loads, as k_mesh_normals has them; neighbouring vertices share faces, so they hit L2).
// ================================================================================================================
constexpr uint32_t LAP_CHUNK = 4;
constexpr int LAP_UMBRELLA_T = 3;
struct LapV {
  float c[LAP_CHUNK];
};
// the chunk's channels of one record (the channels behind n are not read: +0)
__device__ __forceinline__ LapV lap_ld(const float *p, uint32_t n) {
  LapV r;
#pragma unroll
  for (uint32_t j = 0; j < LAP_CHUNK; ++j) r.c[j] = j < n ? p[j] : 0.0f;
  return r;
}
template <int MODE> __global__ __launch_bounds__(256) void k_mesh_laplacian(const MeshLaplacianArgs a) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x, set = blockIdx.y, ch0 = blockIdx.z * LAP_CHUNK;
  if (v >= a.n_verts) return;
  const uint32_t n = a.n_ch - ch0 < LAP_CHUNK ? a.n_ch - ch0 : LAP_CHUNK; // (the host: gridDim.z = ceil(n_ch / LAP_CHUNK), so >= 1)
  const float *x = a.x + (size_t)set * a.n_verts * a.x_stride + ch0;
  const uint32_t c_begin = a.corner_off[v], c_end = a.corner_off[v + 1];
  const float n_v = (float)(2u * (c_end - c_begin));
  const LapV xv = lap_ld(x + (size_t)v * a.x_stride, n);
  LapV S;
#pragma unroll
  for (uint32_t j = 0; j < LAP_CHUNK; ++j) S.c[j] = 0.0f;
  for (uint32_t c = c_begin; c < c_end; ++c) {
    const uint32_t corner = a.corners[c], face = corner / 3u, k = corner - 3u * face;
    const uint32_t *f = a.faces + (size_t)face * 3;
    const uint32_t i0 = f[0], i1 = f[1], i2 = f[2];
    const uint32_t ia = k == 0u ? i1 : k == 1u ? i2 : i0, ib = k == 0u ? i2 : k == 1u ? i0 : i1;
    if (MODE == SRZ_LAP_COTAN) {
      const F3 p0 = ldv3(a.wpos + (size_t)i0 * a.wpos_stride), p1 = ldv3(a.wpos + (size_t)i1 * a.wpos_stride),
               p2 = ldv3(a.wpos + (size_t)i2 * a.wpos_stride);
      const F3 e01 = sub3(p1, p0), e02 = sub3(p2, p0);
      const F3 N = cross3(e01, e02);
      const float d2 = dot3(N.x, N.y, N.z, N.x, N.y, N.z);
      if (!(d2 > 0.0f && d2 <= __FLT_MAX__)) continue; // (SKIPPED, never multiplied by zero: no x behind the face is read)
      const float inv = 1.0f / __builtin_sqrtf(d2);
      // cot_m = dot3(p[i_(m+1)] - p[i_m], p[i_(m+2)] - p[i_m]) * inv, in the face's own order
      const F3 e12 = sub3(p2, p1), e10 = sub3(p0, p1), e20 = sub3(p0, p2), e21 = sub3(p1, p2);
      const float cot0 = dot3(e01.x, e01.y, e01.z, e02.x, e02.y, e02.z) * inv, cot1 = dot3(e12.x, e12.y, e12.z, e10.x, e10.y, e10.z) * inv,
                  cot2 = dot3(e20.x, e20.y, e20.z, e21.x, e21.y, e21.z) * inv;
      const float cot_a = k == 0u ? cot1 : k == 1u ? cot2 : cot0, cot_b = k == 0u ? cot2 : k == 1u ? cot0 : cot1;
      const LapV xa = lap_ld(x + (size_t)ia * a.x_stride, n), xb = lap_ld(x + (size_t)ib * a.x_stride, n);
#pragma unroll
      for (uint32_t j = 0; j < LAP_CHUNK; ++j) S.c[j] = S.c[j] + (cot_b * (xv.c[j] - xa.c[j]) + cot_a * (xv.c[j] - xb.c[j]));
    } else {
      const LapV xa = lap_ld(x + (size_t)ia * a.x_stride, n), xb = lap_ld(x + (size_t)ib * a.x_stride, n);
      if (MODE == LAP_UMBRELLA_T) {
        const float n_a = (float)(2u * (a.corner_off[ia + 1] - a.corner_off[ia])), n_b = (float)(2u * (a.corner_off[ib + 1] - a.corner_off[ib]));
#pragma unroll
        for (uint32_t j = 0; j < LAP_CHUNK; ++j) S.c[j] = S.c[j] + (xa.c[j] / n_a + xb.c[j] / n_b);
      } else {
#pragma unroll
        for (uint32_t j = 0; j < LAP_CHUNK; ++j) S.c[j] = S.c[j] + (xa.c[j] + xb.c[j]);
      }
    }
  }
  float *o = a.out + ((size_t)set * a.n_verts + v) * a.out_stride + ch0;
#pragma unroll
  for (uint32_t j = 0; j < LAP_CHUNK; ++j) {
    float r;
    if (MODE == SRZ_LAP_UMBRELLA) r = n_v > 0.0f ? xv.c[j] - S.c[j] / n_v : 0.0f;
    else if (MODE == SRZ_LAP_GRAPH) r = n_v * xv.c[j] - S.c[j];
    else if (MODE == SRZ_LAP_COTAN) r = 0.5f * S.c[j];
    else r = (n_v > 0.0f ? xv.c[j] : 0.0f) - S.c[j];
    if (j < n) o[j] = r;
  }
}

// ================================================================================================================
// k_mesh_edges / k_mesh_edges_grad — srz_mesh_edges and its backward (include/srz.h states the rules): k_mesh_normals' shape, over
// FACES — grid (blocks of 256 faces, position sets), a thread OWNS (set, face) and stores its three floats once — and, for the
// backward's gathers, over vertices.  No atomics, no barrier, no LDS, plain stores, bit-reproducible.  The slot holds no edge table:
// the faces across edge (a, b) of f are found in the corner list of whichever end has the SHORTER list (a hub vertex of thousands of
// faces costs its spokes' other ends a walk of their own few corners, not of the hub's list).  corner_off, corners and faces are
// indexed per lane (nothing is wave-uniform: vector loads, as k_mesh_laplacian has them).  MODE of the backward: 0 LENGTH (per
// vertex), 1 DIHEDRAL's phase 1 (per face: gN into `work`), 2 DIHEDRAL's phase 2 (per vertex: srz_mesh_normals_grad's gather with
// G = gN of the corner's own face).
// ================================================================================================================
// the unit normal of face (i0, i1, i2) of position set p, in the face's own order; r = 1 / |N|.  false: the face is not ok
__device__ __forceinline__ bool edge_unit_normal(const float *p, uint32_t stride, uint32_t i0, uint32_t i1, uint32_t i2, F3 &n, float &r) {
  const F3 p0 = ldv3(p + (size_t)i0 * stride);
  const F3 N = cross3(sub3(ldv3(p + (size_t)i1 * stride), p0), sub3(ldv3(p + (size_t)i2 * stride), p0));
  const float d2 = dot3(N.x, N.y, N.z, N.x, N.y, N.z);
  const bool ok = d2 > 0.0f && d2 <= __FLT_MAX__;
  r = ok ? 1.0f / __builtin_sqrtf(d2) : 0.0f;
  n = F3{N.x * r, N.y * r, N.z * r};
  return ok;
}
// THE NEIGHBOURS of edge (va, vb) of face f: visit(g, j', g0, g1, g2) per entry, in entry order (g's three vertices come along)
template <class Visit> __device__ __forceinline__ void edge_neighbours(const MeshEdgesArgs &a, uint32_t f, uint32_t va, uint32_t vb, Visit visit) {
  const uint32_t a0 = a.corner_off[va], a1 = a.corner_off[va + 1], b0 = a.corner_off[vb], b1 = a.corner_off[vb + 1];
  const bool walk_b = b1 - b0 < a1 - a0;
  const uint32_t o = walk_b ? va : vb, end = walk_b ? b1 : a1;
  for (uint32_t c = walk_b ? b0 : a0; c < end; ++c) {
    const uint32_t corner = a.corners[c], g = corner / 3u, k = corner - 3u * g;
    if (g == f) continue;
    const uint32_t *gf = a.faces + (size_t)g * 3;
    const uint32_t g0 = gf[0], g1 = gf[1], g2 = gf[2];
    const uint32_t next = k == 0u ? g1 : k == 1u ? g2 : g0, prev = k == 0u ? g2 : k == 1u ? g0 : g1;
    if (next == o) visit(g, k == 0u ? 2u : k - 1u, g0, g1, g2);      // the edge opposite the remaining corner (k + 2) % 3
    else if (prev == o) visit(g, k == 2u ? 0u : k + 1u, g0, g1, g2); // ... (k + 1) % 3
  }
}
template <int KIND> __global__ __launch_bounds__(256) void k_mesh_edges(const MeshEdgesArgs a) {
  const uint32_t f = blockIdx.x * 256 + threadIdx.x, set = blockIdx.y;
  if (f >= a.n_faces) return;
  const float *p = a.pos + (size_t)set * a.n_verts * a.pos_stride;
  const uint32_t *fi = a.faces + (size_t)f * 3;
  const uint32_t i0 = fi[0], i1 = fi[1], i2 = fi[2];
  float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
  if (KIND == SRZ_EDGE_LENGTH) {
    const F3 P0 = ldv3(p + (size_t)i0 * a.pos_stride), P1 = ldv3(p + (size_t)i1 * a.pos_stride), P2 = ldv3(p + (size_t)i2 * a.pos_stride);
    const F3 d0 = sub3(P2, P1), d1 = sub3(P0, P2), d2 = sub3(P1, P0); // d_j = p[b_j] - p[a_j]
    r0 = __builtin_sqrtf(dot3(d0.x, d0.y, d0.z, d0.x, d0.y, d0.z));
    r1 = __builtin_sqrtf(dot3(d1.x, d1.y, d1.z, d1.x, d1.y, d1.z));
    r2 = __builtin_sqrtf(dot3(d2.x, d2.y, d2.z, d2.x, d2.y, d2.z));
  } else {
    F3 nf{0.0f, 0.0f, 0.0f};
    float rf;
    if (KIND == SRZ_EDGE_COUNT || edge_unit_normal(p, a.pos_stride, i0, i1, i2, nf, rf)) {
#pragma unroll
      for (uint32_t j = 0; j < 3u; ++j) {
        const uint32_t va = j == 0u ? i1 : j == 1u ? i2 : i0, vb = j == 0u ? i2 : j == 1u ? i0 : i1;
        uint32_t count = 1u;
        float acc = 0.0f;
        edge_neighbours(a, f, va, vb, [&](uint32_t, uint32_t, uint32_t g0, uint32_t g1, uint32_t g2) {
          if (KIND == SRZ_EDGE_COUNT) {
            ++count;
          } else {
            F3 ng;
            float rg;
            if (edge_unit_normal(p, a.pos_stride, g0, g1, g2, ng, rg)) acc = acc + (1.0f - dot3(nf.x, nf.y, nf.z, ng.x, ng.y, ng.z));
          }
        });
        const float r = KIND == SRZ_EDGE_COUNT ? (float)count : acc;
        if (j == 0u) r0 = r;
        else if (j == 1u) r1 = r;
        else r2 = r;
      }
    }
  }
  float *o = a.out + ((size_t)set * a.n_faces + f) * a.out_stride;
  o[0] = r0, o[1] = r1, o[2] = r2;
}
template <int MODE> __global__ __launch_bounds__(256) void k_mesh_edges_grad(const MeshEdgesArgs a) {
  const uint32_t id = blockIdx.x * 256 + threadIdx.x, set = blockIdx.y;
  if (id >= (MODE == 1 ? a.n_faces : a.n_verts)) return;
  const float *p = a.pos + (size_t)set * a.n_verts * a.pos_stride;
  const float *gout = a.gout + (size_t)set * a.n_faces * a.gout_stride;
  if (MODE == 1) {
    const uint32_t f = id;
    const uint32_t *fi = a.faces + (size_t)f * 3;
    const uint32_t i0 = fi[0], i1 = fi[1], i2 = fi[2];
    F3 nf, gN{0.0f, 0.0f, 0.0f};
    float rf;
    if (edge_unit_normal(p, a.pos_stride, i0, i1, i2, nf, rf)) {
      F3 H{0.0f, 0.0f, 0.0f};
#pragma unroll
      for (uint32_t j = 0; j < 3u; ++j) {
        const uint32_t va = j == 0u ? i1 : j == 1u ? i2 : i0, vb = j == 0u ? i2 : j == 1u ? i0 : i1;
        const float w_fj = gout[(size_t)f * a.gout_stride + j];
        edge_neighbours(a, f, va, vb, [&](uint32_t g, uint32_t jp, uint32_t g0, uint32_t g1, uint32_t g2) {
          F3 ng;
          float rg;
          if (!edge_unit_normal(p, a.pos_stride, g0, g1, g2, ng, rg)) return;
          const float s = w_fj + gout[(size_t)g * a.gout_stride + jp];
          H = F3{H.x - ng.x * s, H.y - ng.y * s, H.z - ng.z * s};
        });
      }
      const float t = dot3(nf.x, nf.y, nf.z, H.x, H.y, H.z);
      gN = F3{(H.x - nf.x * t) * rf, (H.y - nf.y * t) * rf, (H.z - nf.z * t) * rf};
    }
    float *w = a.work + ((size_t)set * a.n_faces + f) * 3;
    w[0] = gN.x, w[1] = gN.y, w[2] = gN.z;
  } else {
    const uint32_t v = id;
    const float *gn = MODE == 2 ? a.work + (size_t)set * a.n_faces * 3 : nullptr; // (LENGTH has no workspace)
    F3 acc{0.0f, 0.0f, 0.0f};
    for (uint32_t c = a.corner_off[v], c_end = a.corner_off[v + 1]; c < c_end; ++c) {
      const uint32_t corner = a.corners[c], face = corner / 3u, k = corner - 3u * face;
      const uint32_t *fi = a.faces + (size_t)face * 3;
      const uint32_t i0 = fi[0], i1 = fi[1], i2 = fi[2];
      const F3 A = ldv3(p + (size_t)i0 * a.pos_stride), B = ldv3(p + (size_t)i1 * a.pos_stride), C = ldv3(p + (size_t)i2 * a.pos_stride);
      if (MODE == 0) {
        // v is corner k: the b end of edge j1 = (k + 1) % 3 (from the previous corner) and the a end of j2 = (k + 2) % 3 (to the next)
        const F3 Pk = k == 0u ? A : k == 1u ? B : C, Pn = k == 0u ? B : k == 1u ? C : A, Pp = k == 0u ? C : k == 1u ? A : B;
        const uint32_t j1 = k == 2u ? 0u : k + 1u, j2 = k == 0u ? 2u : k - 1u;
        const float *g = gout + (size_t)face * a.gout_stride;
        const F3 d1 = sub3(Pk, Pp), d2 = sub3(Pn, Pk);
        const float len1 = __builtin_sqrtf(dot3(d1.x, d1.y, d1.z, d1.x, d1.y, d1.z));
        if (len1 > 0.0f && len1 <= __FLT_MAX__) {
          const float inv = 1.0f / len1, g1 = g[j1];
          acc = F3{acc.x + g1 * (d1.x * inv), acc.y + g1 * (d1.y * inv), acc.z + g1 * (d1.z * inv)};
        }
        const float len2 = __builtin_sqrtf(dot3(d2.x, d2.y, d2.z, d2.x, d2.y, d2.z));
        if (len2 > 0.0f && len2 <= __FLT_MAX__) {
          const float inv = 1.0f / len2, g2 = g[j2];
          acc = F3{acc.x - g2 * (d2.x * inv), acc.y - g2 * (d2.y * inv), acc.z - g2 * (d2.z * inv)};
        }
      } else {
        const F3 G = ldv3(gn + (size_t)face * 3);
        const F3 term = k == 0u ? cross3(sub3(B, C), G) : k == 1u ? cross3(sub3(C, A), G) : cross3(G, sub3(B, A));
        acc = add3(acc, term);
      }
    }
    float *g = a.gpos + ((size_t)set * a.n_verts + v) * 3;
    g[0] = acc.x, g[1] = acc.y, g[2] = acc.z;
  }
}

// ================================================================================================================
// k_corner_attr / k_corner_attr_grad — srz_sceneset_corner_attr and its backward (include/srz.h).  Grid (blocks of 256 (vertex,
// channel) pairs, frames); a thread OWNS (frame, vertex, channel): neighbouring lanes are neighbouring channels of one vertex, so
// the attribute row, the rows of the triangle stream and the gradient row are each read and written as runs, and the backward
// needs ONE accumulator whatever n_ch (the corner-list words are the same address across a vertex's lanes: one fetch).  The
// thread walks the frame's draws of the slot in draw order and its vertex's corners in list order: every corner has one owner, so
// the forward's stores never meet; the backward is a gather.  No atomics, no barrier.
// ================================================================================================================
template <bool GRAD> __device__ __forceinline__ void corner_attr_walk(const CornerAttrArgs &a) {
  const uint32_t f = blockIdx.y;
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t v = (e >> 32) != 0ull ? (uint32_t)(e / a.n_ch) : (uint32_t)e / a.n_ch; // (block-uniform choice)
  if (v >= a.n_verts) return;
  const uint32_t ch = (uint32_t)(e - (uint64_t)v * a.n_ch);
  const SRZ_CAS FrameDesc *fd = as_const(a.frames) + f;
  const uint32_t n_draws = fd->n_batches, draw0 = fd->batch_off, tri0 = fd->tri_off;
  const uint32_t c_begin = a.corner_off[v], c_end = a.corner_off[v + 1];
  const size_t frame_at = (size_t)f * a.pos_tris * 3u * a.n_ch + ch;
  float val = 0.0f; // the forward's value, the backward's sum
  if (!GRAD) val = a.attr[(size_t)f * a.attr_frame_stride + (size_t)v * a.n_ch + ch];
  for (uint32_t j = 0; j < n_draws; ++j) {
    const SRZ_CAS DrawDesc *d = as_const(a.draws) + draw0 + j;
    if (d->verts != a.verts) continue; // (another slot's draw)
    const size_t draw_at = frame_at + (size_t)(d->tri_off - tri0) * 3u * a.n_ch;
    for (uint32_t c = c_begin; c < c_end; ++c) {
      const size_t i = draw_at + (size_t)a.corners[c] * a.n_ch; // (corner = 3 * face + k: the stream's own order)
      if (GRAD)
        val = val + a.gout[i];
      else
        a.out[i] = val;
    }
  }
  if (GRAD) a.gattr[((size_t)f * a.n_verts + v) * a.n_ch + ch] = val;
}
__global__ __launch_bounds__(256) void k_corner_attr(const CornerAttrArgs a) { corner_attr_walk<false>(a); }
__global__ __launch_bounds__(256) void k_corner_attr_grad(const CornerAttrArgs a) { corner_attr_walk<true>(a); }

// ================================================================================================================
// Tight rectangles.  The reference tests every pixel of a triangle's bounding box; a pixel outside the triangle fails the test
// and leaves no trace, so pixels that are CERTAINLY outside need not be tested — and a tile or band the triangle certainly
// misses need not list it.  slab_extent gives the extent along u of (triangle ∩ slab lo <= w <= hi), (u, w) = (x, y) or (y, x),
// from the vertices inside the slab and the edges' crossings of its two bounds (+inf / -inf when the triangle misses it).
// CONSERVATIVE: a pixel can pass the rounded inside tests (cover_v / cover_s) only within a distance eps of the true triangle.
// With D = the vertices' extent and R = D + 1 >= every |pixel - vertex| component of a TESTED pixel (the box starts at
// trunc(min): up to one pixel before the extent, never behind it — guaranteed by the `near` test below, which sends triangles
// whose clamped box lies away from their extent, i.e. wholly off screen on an axis, to the plain box: there the operands grow
// with the distance to the screen, not with D), u = 2^-24:
//   S test (signs of AB x AP): products <= D R, |error| < 2^-22 D R; a pixel delta outside edge AB has |e| = delta |AB|, and
//       |AB| >= |area2| / (sqrt2 D) >= D / 362 under the sliver guard D^2 <= 256 |area2|, so eps < 2^-13.5 R;
//   V test (signs of alpha, beta, 1 - (alpha + beta)): aPBC = fmsub(PBx,PCy,PCx*PBy) has products <= R^2, |error| < 2^-21.7 R^2,
//       and the multiplication by v_inv keeps its sign: eps < 2^-21.7 R^2 * 362 / D = 2^-13.2 R^2 / D; for gamma the two errors
//       add and v_inv itself is off by <= 2^-13.7 relative (its operands are <= D, |area2| >= D^2 / 256):
//       eps < 2^-13.2 D + 2^-12.2 R^2 / D.
// Both stay below m = D / 512 + 1 / 64 for every D >= 2^-5 (at D = 2^-5: 2^-7.1; large D: 2^-11 D) — smaller triangles (their
// boxes are at most 2 x 2 pixels: nothing to gain), slivers, non-finite or > 2^20 coordinates keep the plain box.  m also covers
// v_rcp's error in the crossings (2^-22 of a length <= D).
// ================================================================================================================
__device__ __forceinline__ bool tight_margin(float ax, float ay, float bx, float by, float cx, float cy, float area2, int bsx, int bsy,
                                             int bex, int bey, float &m) {
  const float mnx = __builtin_fminf(__builtin_fminf(ax, bx), cx), mxx = __builtin_fmaxf(__builtin_fmaxf(ax, bx), cx);
  const float mny = __builtin_fminf(__builtin_fminf(ay, by), cy), mxy = __builtin_fmaxf(__builtin_fmaxf(ay, by), cy);
  const float D = __builtin_fmaxf(mxx - mnx, mxy - mny);
  m = __builtin_fmaf(D, 0.001953125f, 0.015625f);
  // the clamped box [bsx, bex] x [bsy, bey] lies inside [min - 1, max] of the vertices on both axes (conversions are exact)
  const bool near = ((float)bsx + 1.0f >= mnx) & ((float)bex <= mxx) & ((float)bsy + 1.0f >= mny) & ((float)bey <= mxy);
  return near && D * D <= 256.0f * __builtin_fabsf(area2) && D <= 1048576.0f && D >= 0.03125f; // (false for NaN / inf)
}
__device__ __forceinline__ void slab_extent(float au, float aw, float bu, float bw, float cu, float cw, float lo, float hi, float &mn,
                                            float &mx) {
  mn = __builtin_inff(), mx = -__builtin_inff();
  auto vertex = [&](float u, float w) {
    const bool in = (w >= lo) & (w <= hi);
    mn = in ? __builtin_fminf(mn, u) : mn, mx = in ? __builtin_fmaxf(mx, u) : mx;
  };
  auto edge = [&](float pu, float pw, float qu, float qw) {
    const float inv = __builtin_amdgcn_rcpf(pw - qw), du = qu - pu;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float bound = k ? hi : lo, dp = pw - bound, dq = qw - bound;
      const float u = __builtin_fmaf(du, dp * inv, pu); // (pw == qw: no crossing, the NaN / inf is not selected)
      const bool cross = (dp < 0.0f) != (dq < 0.0f);
      mn = cross ? __builtin_fminf(mn, u) : mn, mx = cross ? __builtin_fmaxf(mx, u) : mx;
    }
  };
  vertex(au, aw), vertex(bu, bw), vertex(cu, cw);
  edge(au, aw, bu, bw), edge(bu, bw, cu, cw), edge(cu, cw, au, aw);
}
// the integer range [i0, i1] clipped to ceil(mn - m) .. floor(mx + m) (as floats first: the conversions stay in range); an
// extent that misses the range gives i0 > i1
__device__ __forceinline__ void clip_range(int &i0, int &i1, float mn, float mx, float m) {
  const float f0 = (float)i0, f1 = (float)i1;
  i0 = (int)__builtin_fminf(__builtin_fmaxf(__builtin_ceilf(mn - m), f0), f1 + 1.0f);
  i1 = (int)__builtin_fmaxf(__builtin_fminf(__builtin_floorf(mx + m), f1), f0 - 1.0f);
}

// ================================================================================================================
// bucket_group — the O(triangles) half of the binning, shared by k_setup and k_chunks: the GROUP_TRIS triangles of one group
// (GROUP_K per thread: triangle g * GROUP_TRIS + k * 256 + tid) are sorted by the local 32-row bands their bounding boxes reach, in LDS:
//   count  one LDS atomic per (triangle, band)             scan  exclusive prefix over the bands (wave 0, DPP)
//   fill   a second LDS atomic hands out the slots; the entry {triangle, tile-x range} goes to the group's own region
// and the group's descriptor row [band] = first entry << 16 | entries.  No global atomics, no cross-workgroup state.
// A group that needs more than ENT_PER_GROUP entries (or holds a triangle more than 64 local bands tall) is marked
// DESC_RAW in every band instead: k_bin's band workgroups then walk its bounding boxes themselves.
// ================================================================================================================
__device__ __forceinline__ void bucket_group(const RenderArgs &a, const uint32_t nlb, const uint32_t group, const uint32_t t0,
                                             const bool packed, const uint32_t tri_off, const BBox (&bb)[GROUP_K],
                                             const bool (&keep)[GROUP_K], const float (*P)[9], uint32_t *s_cnt, uint32_t *s_off,
                                             uint32_t *s_fill, uint32_t *s_misc) {
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int world = a.shard_world, rank = a.shard_rank;
  for (uint32_t i = (uint32_t)tid; i < nlb; i += 256u) s_cnt[i] = 0u;
  if (tid == 0) s_misc[0] = 0u;
  __syncthreads();
  // the local bands of triangle k: lb0[k] .. lb0[k] + nb[k] - 1 (band b is local iff rank_of_band(b) == rank; local index b / world: one
  // band of every group of `world` bands, so the local indices a box reaches are consecutive)
  int lb0[GROUP_K], nb[GROUP_K];
#pragma unroll
  for (int k = 0; k < (int)GROUP_K; ++k) {
    lb0[k] = 0, nb[k] = 0;
    if (keep[k]) {
      const int b0 = (int)bb[k].sy >> 5, b1 = (int)bb[k].ey >> 5;
      int g0 = b0 / world, g1 = b1 / world;
      if (band_of(g0, rank, world) < b0) ++g0;
      if (band_of(g1, rank, world) > b1) --g1;
      if (g0 <= g1) lb0[k] = g0, nb[k] = g1 - g0 + 1;
      if (nb[k] > 64) s_misc[0] = 1u, nb[k] = 0; // (benign race: every writer stores 1)
      for (int j = 0; j < nb[k]; ++j) atomicAdd(&s_cnt[lb0[k] + j], 1u);
    }
  }
  __syncthreads();
  if (tid < 64) {
    uint32_t run = 0;
    for (uint32_t i0 = 0; i0 < nlb; i0 += 64u) {
      const uint32_t i = i0 + (uint32_t)lane, v = i < nlb ? s_cnt[i] : 0u, incl = wave_scan_add(v);
      if (i < nlb) s_off[i] = s_fill[i] = run + incl - v;
      run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (lane == 0 && run > ENT_PER_GROUP) s_misc[0] = 1u;
  }
  __syncthreads();
  const bool raw = s_misc[0] != 0u;
  // what a tile list holds of a triangle: its index in the frame — and, FD_PACKED, its batch above it (coalesced 2-byte loads here,
  // instead of a gather per staged triangle in k_shade)
  uint32_t tpk[GROUP_K];
#pragma unroll
  for (int k = 0; k < (int)GROUP_K; ++k) {
    const uint32_t t = t0 + (uint32_t)k * 256u + (uint32_t)tid;
    tpk[k] = t;
    if (packed && keep[k]) tpk[k] = t | ((uint32_t)as_const(a.tri_batch)[tri_off + t] << PACK_IDX_BITS);
  }
  uint32_t *desc = a.band_desc + (size_t)group * nlb;
  for (uint32_t i = (uint32_t)tid; i < nlb; i += 256u) desc[i] = raw ? DESC_RAW : ((s_off[i] << 16) | s_cnt[i]);
  if (!raw) {
    uint2 *ent = a.band_ent + (size_t)group * ENT_PER_GROUP;
#pragma unroll
    for (int k = 0; k < (int)GROUP_K; ++k) {
      const uint32_t xr = (uint32_t)((int)bb[k].sx >> 5) | ((uint32_t)((int)bb[k].ex >> 5) << 16);
      // (P: the positions, where the caller has them in registers) the tile range of a band is tightened to the triangle's
      // x-extent inside the band's rows (tight_margin): the tiles in the corners of a large bounding box drop out of the lists
      float m = 0.0f;
      const bool tight = P != nullptr && nb[k] > 0 &&
                         tight_margin(P[k][0], P[k][1], P[k][3], P[k][4], P[k][6], P[k][7],
                                      (P[k][3] - P[k][0]) * (P[k][7] - P[k][1]) - (P[k][4] - P[k][1]) * (P[k][6] - P[k][0]), bb[k].sx,
                                      bb[k].sy, bb[k].ex, bb[k].ey, m);
      for (int j = 0; j < nb[k]; ++j) {
        uint32_t xr_j = xr;
        if (tight) {
          const int b = band_of(lb0[k] + j, rank, world);
          int X0 = bb[k].sx, X1 = bb[k].ex;
          float mn, mx;
          slab_extent(P[k][0], P[k][1], P[k][3], P[k][4], P[k][6], P[k][7], (float)max(b * BAND, (int)bb[k].sy) - m,
                      (float)min(b * BAND + BAND - 1, (int)bb[k].ey) + m, mn, mx);
          clip_range(X0, X1, mn, mx, m);
          xr_j = X0 <= X1 ? ((uint32_t)(X0 >> 5) | ((uint32_t)(X1 >> 5) << 16)) : 1u; // (1: tiles 1 .. 0 = none)
        }
        ent[atomicAdd(&s_fill[lb0[k] + j], 1u)] = make_uint2(tpk[k], xr_j);
      }
    }
  }
  __syncthreads(); // (LDS is reused by this workgroup's next group)
}

// row range of the kept triangles of a 64-triangle chunk (= one wave's 64 consecutive triangles): k_raster_slow and the
// DESC_RAW walk of k_bin skip the chunks that cannot reach their rows without reading the 64 bounding boxes
__device__ __forceinline__ void chunk_rows_store(const RenderArgs &a, const uint32_t chunk_off, const uint32_t t, const uint32_t n_tris,
                                                 const bool keep, const BBox &bb) {
  int lo = keep ? (int)bb.sy : 0x7fff, hi = keep ? (int)bb.ey : -1;
  for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o)), hi = max(hi, __shfl_xor(hi, o));
  if ((threadIdx.x & 63) == 0 && (t & ~63u) < n_tris) a.chunk_rows[chunk_off + t / 64u] = ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
}

__device__ __forceinline__ void reset_render_counters(const RenderArgs &a) {
  // the work lists, k_shade's cursors into them, the record pool and the slow list start empty
  if (threadIdx.x < N_WORK_LISTS) a.work_count[threadIdx.x * CNT_STRIDE] = 0u, a.work_count[threadIdx.x * CNT_STRIDE + 1] = 0u;
  if (threadIdx.x <= a.pool_sub_mask) a.pool_heads[threadIdx.x * CNT_STRIDE] = 0u;
  if (threadIdx.x == 0) *a.slow_count = 0u, *a.redo_count = 0u;
}

// ================================================================================================================
// k_setup — per triangle: finite check, bbox, backface test (src/Triangle.cpp:147-151,243-257; Rasterizer.cpp:203);
// per group of GROUP_TRIS triangles (one workgroup pass, GROUP_K triangles per thread): the band sort above
// ================================================================================================================
template <bool STATS>
__global__ __launch_bounds__(256) void k_setup(RenderArgs a, BBox *bbox_out) {
  __shared__ uint32_t s_cnt[MAX_LOCAL_BANDS], s_off[MAX_LOCAL_BANDS], s_fill[MAX_LOCAL_BANDS], s_misc[2];
  if (blockIdx.x == 0 && blockIdx.y == 0) reset_render_counters(a);
  const SRZ_CAS FrameDesc *fd = as_const(a.frames) + blockIdx.y;
  const int W = fd->width, H = fd->height;
  const uint32_t n_tris = fd->n_tris, tri_off = fd->tri_off;
  const float ex = fd->eye[0], ey = fd->eye[1], ez = fd->eye[2];
  unsigned long long n_culled = 0, tests = 0;
  const uint32_t n_groups = (n_tris + GROUP_TRIS - 1u) / GROUP_TRIS;
  for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const uint32_t t0 = g * GROUP_TRIS;
    float P[GROUP_K][9];
#pragma unroll
    for (int k = 0; k < (int)GROUP_K; ++k) { // (all the loads of the thread's triangles in flight together)
      const uint32_t t = t0 + (uint32_t)k * 256u + threadIdx.x;
      load_pos9(as_const(a.tri_pos) + (size_t)(tri_off + (t < n_tris ? t : 0u)) * a.pos_stride, P[k]);
    }
    BBox bb[GROUP_K];
    bool keep[GROUP_K];
#pragma unroll
    for (int k = 0; k < (int)GROUP_K; ++k) {
      const uint32_t t = t0 + (uint32_t)k * 256u + threadIdx.x;
      const bool live = t < n_tris;
      keep[k] = setup_triangle(P[k], W, H, ex, ey, ez, live, bb[k]);
      if (STATS) {
        if (keep[k])
          tests += (unsigned long long)(bb[k].ex - bb[k].sx + 1) * (unsigned long long)(bb[k].ey - bb[k].sy + 1);
        else if (live)
          n_culled++;
      }
      if (live) bbox_out[tri_off + t] = bb[k];
      chunk_rows_store(a, fd->chunk_off, t, n_tris, keep[k], bb[k]);
    }
    bucket_group(a, fd->n_local_bands, fd->group_off + g, t0, (fd->flags & FD_PACKED) != 0u, tri_off, bb, keep, P, s_cnt, s_off, s_fill, s_misc);
  }
  if (STATS) {
    if (n_culled) atomicAdd(&a.stats[ST_CULLED], n_culled);
    if (tests) atomicAdd(&a.stats[ST_PIXEL_TESTS], tests);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&a.stats[ST_TRIS], (unsigned long long)n_tris);
  }
}

// k_chunks — scenesets: k_vertex has written the bounding boxes; what is left of k_setup is the reset of the per-render
// counters, the row range of every 64-triangle chunk and the band sort (8 bytes read per triangle instead of 96)
__global__ __launch_bounds__(256) void k_chunks(RenderArgs a) {
  __shared__ uint32_t s_cnt[MAX_LOCAL_BANDS], s_off[MAX_LOCAL_BANDS], s_fill[MAX_LOCAL_BANDS], s_misc[2];
  if (blockIdx.x == 0 && blockIdx.y == 0) reset_render_counters(a);
  const SRZ_CAS FrameDesc *fd = as_const(a.frames) + blockIdx.y;
  const uint32_t n_tris = fd->n_tris, tri_off = fd->tri_off;
  const SRZ_CAS u32x2 *bbox = as_const(reinterpret_cast<const u32x2 *>(a.bbox + tri_off));
  const uint32_t n_groups = (n_tris + GROUP_TRIS - 1u) / GROUP_TRIS;
  for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const uint32_t t0 = g * GROUP_TRIS;
    BBox bb[GROUP_K];
    bool keep[GROUP_K];
#pragma unroll
    for (int k = 0; k < (int)GROUP_K; ++k) {
      const uint32_t t = t0 + (uint32_t)k * 256u + threadIdx.x;
      bb[k].sx = 1, bb[k].sy = 1, bb[k].ex = 0, bb[k].ey = 0;
      if (t < n_tris) {
        const u32x2 r = bbox[t];
        bb[k].sx = (int16_t)(r.x & 0xffff), bb[k].sy = (int16_t)(r.x >> 16), bb[k].ex = (int16_t)(r.y & 0xffff), bb[k].ey = (int16_t)(r.y >> 16);
      }
      keep[k] = bb[k].sx <= bb[k].ex; // (the empty box of a culled triangle: sx > ex)
      chunk_rows_store(a, fd->chunk_off, t, n_tris, keep[k], bb[k]);
    }
    bucket_group(a, fd->n_local_bands, fd->group_off + g, t0, (fd->flags & FD_PACKED) != 0u, tri_off, bb, keep, nullptr, s_cnt, s_off, s_fill, s_misc);
  }
}

// ================================================================================================================
// k_bin — one WORKGROUP per (frame, local band): the triangles whose bbox touches the band are appended to the lists
// of the 32x32 tiles they overlap.  The rasteriser's result does not depend on the order of a tile's list (k_raster
// resolves depth ties with the triangle index, not with the list position), so this is a plain count / scan / fill with
// LDS atomics — no ordered compaction:
//   input   the band's entries, sorted out by k_setup / k_chunks (bucket_group): per group of GROUP_TRIS triangles one descriptor
//           word (first entry, entries) — 64 groups per wave load — whose entry runs are flattened into dense batches of
//           64 (the triangles that start inside a batch mark their position, a DPP max-scan gives every lane its group,
//           its descriptor comes over the LDS crossbar): the walk reads 8 bytes per (triangle, band) pair, nothing else.
//           Groups marked DESC_RAW (huge triangles) are walked the old way: chunk row ranges, then bounding boxes.
//   pass 1  every entry bumps the LDS counter of each tile it overlaps
//   scan    exclusive prefix over the tile counters (wave 0) = the band's layout; ONE global atomic takes the band's
//           records from the sub-pool of this workgroup (k_raster_slow serves the tiles of a band that does not fit)
//   pass 2  every (triangle, tile) pair becomes one 4-byte index at pool[band base + tile offset + slot]: assembled in LDS,
//           written as one coalesced run (k_raster gathers the triangles' 36 bytes of positions and their 8-byte boxes
//           through these indices)
// ================================================================================================================
constexpr int BIN_MAX_WAVES = 8; // launched with 2, 4 or 8 waves: the walk is latency-bound, so short streams take small
                                 // workgroups (more of them resident per CU), long ones more waves per band
constexpr uint32_t BIN_STAGE = 4096; // indices of one band staged in LDS (16 KB)
// The entries a wave met on its first walk (count) are kept in LDS for its second one (fill): BIN_KEEP batches of 64 per wave in the
// eight-wave build (16 KB: the wave slots, not the LDS, bound that build to four workgroups per CU), one batch in the smaller ones (whose
// eight workgroups per CU leave 2 KB each).  A wave that met more batches, or a DESC_RAW group, walks again as before (round 6)
__host__ __device__ constexpr uint32_t bin_keep(uint32_t waves) { return waves >= 8u ? 4u : 1u; }
// dynamic LDS = (3 * tiles_x + 64 * waves + 4 + BIN_STAGE + 128 * waves * bin_keep(waves)) dwords: [count | offset | fill cursor] per tile,
// per-wave marks, stage, kept entries
__global__ __launch_bounds__(64 * BIN_MAX_WAVES) void k_bin(RenderArgs a) {
  const int BIN_WAVES = (int)(blockDim.x >> 6);
  extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
  const uint32_t TX = a.tiles_x;
  uint32_t *s_cnt = s_dyn, *s_off = s_dyn + TX, *s_fill = s_dyn + 2 * TX, *s_marks = s_dyn + 3 * TX;
  uint32_t *s_misc = s_marks + 64 * BIN_WAVES; // [0] first index of the band in pool[] (or UNLISTED), [1] indices of the band
  uint32_t *s_stage = s_misc + 4;

  // same XCD-aware decomposition as k_raster: workgroup i bins frame (i % 8) of its group of 8 frames, so a frame's
  // records are written through the L2 of the XCD that will rasterise it
  const uint32_t wg = blockIdx.x, xcd = wg & 7u, jj = wg >> 3;
  const uint32_t frame = (jj / a.n_local_bands) * 8u + xcd, lb = jj % a.n_local_bands;
  if (frame >= a.n_frames) return; // workgroup-uniform
  const SRZ_CAS FrameDesc *fd = as_const(a.frames) + frame;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t KEEP = bin_keep((uint32_t)BIN_WAVES);
  // (8-byte entries: behind the stage, at an even dword whatever the frame's width in tiles)
  u32x2 *s_keep = reinterpret_cast<u32x2 *>(s_dyn + ((3u * TX + 64u * (uint32_t)BIN_WAVES + 4u + BIN_STAGE + 1u) & ~1u)) + (size_t)wave * KEEP * 64u;
  uint32_t n_seen = 0;    // batches this wave has met on the current walk (wave-uniform)
  bool keep_ok = true;    // ... and none of them came from a DESC_RAW group
  for (uint32_t w = threadIdx.x; w < 3 * TX; w += blockDim.x) s_dyn[w] = 0u;
  uint32_t *s_mark = s_marks + 64 * wave;
  s_mark[lane] = 0u;
  __syncthreads();
  const uint32_t n_tris = fd->n_tris;
  const bool packed = (fd->flags & FD_PACKED) != 0u; // (tile-list entries carry the batch above the index)
  const int band = band_of((int)lb, a.shard_rank, a.shard_world);
  const int y0 = band * BAND, y1 = y0 + BAND - 1;
  const SRZ_CAS u32x2 *bbox = as_const(reinterpret_cast<const u32x2 *>(a.bbox + fd->tri_off));
  const SRZ_CAS uint32_t *chunk_rows = as_const(a.chunk_rows) + fd->chunk_off;
  const uint32_t n_chunks = (n_tris + 63) / 64, n_groups = (n_tris + GROUP_TRIS - 1u) / GROUP_TRIS;
  const uint32_t nlb = a.n_local_bands;
  const SRZ_CAS uint32_t *desc = as_const(a.band_desc) + (size_t)fd->group_off * nlb + lb;
  const SRZ_CAS u32x2 *ents = reinterpret_cast<const SRZ_CAS u32x2 *>(as_const(a.band_ent) + (size_t)fd->group_off * ENT_PER_GROUP);

  // a DESC_RAW group: its 16 chunks' row ranges, then the bounding boxes of the chunks that can reach the band, the loads of
  // four candidate chunks in flight together
  auto walk_raw = [&](const uint32_t g, auto &&fn) {
    const uint32_t c0 = g * (GROUP_TRIS / 64u);
    bool cand = false;
    const uint32_t c = c0 + (uint32_t)lane;
    if (lane < (int)(GROUP_TRIS / 64u) && c < n_chunks) {
      const uint32_t r = chunk_rows[c];
      cand = (int)(int16_t)(r & 0xffffu) <= y1 && (int)(int16_t)(r >> 16) >= y0;
    }
    unsigned long long mc = __ballot(cand);
    while (mc) {
      uint32_t cj[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ok[u] = mc != 0ull;
        cj[u] = ok[u] ? (uint32_t)__builtin_ctzll(mc) : 0u;
        mc &= mc - 1ull; // (0 stays 0)
      }
      u32x2 r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = bbox[min((c0 + cj[u]) * 64u + (uint32_t)lane, n_tris - 1u)];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!ok[u]) break; // wave-uniform
        const uint32_t t = (c0 + cj[u]) * 64u + (uint32_t)lane;
        const int sx = (int16_t)(r[u].x & 0xffff), sy = (int16_t)(r[u].x >> 16), ex = (int16_t)(r[u].y & 0xffff), ey = (int16_t)(r[u].y >> 16);
        const bool hit = t < n_tris && sx <= ex && sy <= y1 && ey >= y0; // (bbox is clamped to the frame by k_setup)
        uint32_t tp = t;
        if (packed && hit) tp |= (uint32_t)as_const(a.tri_batch)[fd->tri_off + t] << PACK_IDX_BITS;
        fn(tp, hit, sx >> 5, ex >> 5);
      }
    }
  };
  // calls fn(triangle, hit, first tile x, last tile x) wave-wide for every triangle of the frame that reaches the band: every wave
  // reads the descriptors of all groups (64 per round) and takes every BIN_WAVES-th batch of 64 entries, continuing round-robin
  // across the rounds, so the entries of a frame with few groups are still spread over all the waves
  auto walk = [&](auto &&fn) {
    const uint32_t NW = (uint32_t)BIN_WAVES;
    uint32_t first = (uint32_t)wave; // the first batch of the next round that is this wave's
    for (uint32_t r0 = 0; r0 < n_groups; r0 += 64u) {
      const uint32_t g = r0 + (uint32_t)lane;
      const uint32_t d = g < n_groups ? desc[(size_t)g * nlb] : 0u;
      const bool raw = d == DESC_RAW;
      const uint32_t cnt = raw ? 0u : (d & 0xffffu), off = d >> 16;
      const uint32_t incl = wave_scan_add(cnt), excl = incl - cnt;
      const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63), nbat = (T + 63u) >> 6;
      uint32_t b = first;
      for (; b < nbat; b += NW) {
        const uint32_t P0 = b * 64u;
        // the group that reaches into this batch from before it: the last one that starts before P0
        const unsigned long long before = __ballot(cnt != 0u && excl < P0);
        const uint32_t carry = before ? 64u - (uint32_t)__builtin_clzll(before) : 0u;
        const uint32_t r = excl - P0;
        if (cnt != 0u && r < 64u) s_mark[r] = (uint32_t)lane + 1u;
        __builtin_amdgcn_wave_barrier();
        uint32_t m = s_mark[lane];
        __builtin_amdgcn_wave_barrier();
        s_mark[lane] = 0u;
        m = max(wave_scan_max(m), carry);
        const uint32_t sl = (m - 1u) & 63u; // the lane that holds this entry's group
        const uint32_t e_excl = (uint32_t)__builtin_amdgcn_ds_bpermute((int)sl * 4, (int)excl);
        const uint32_t e_off = (uint32_t)__builtin_amdgcn_ds_bpermute((int)sl * 4, (int)off);
        const uint32_t e = P0 + (uint32_t)lane;
        const bool valid = e < T;
        u32x2 en = {0u, 1u}; // (tiles 1 .. 0: none)
        if (valid) en = ents[(size_t)(r0 + sl) * ENT_PER_GROUP + e_off + (e - e_excl)];
        if (n_seen < KEEP) s_keep[n_seen * 64u + (uint32_t)lane] = en;
        ++n_seen;
        fn(en.x, valid, (int)(en.y & 0xffffu), (int)(en.y >> 16));
      }
      first = b - nbat; // (b is the first batch index >= nbat that is this wave's: b - nbat < NW)
      uint32_t ri = 0;  // DESC_RAW groups of the round: dealt to the waves one by one
      for (unsigned long long mr = __ballot(raw); mr != 0ull; mr &= mr - 1ull, ++ri)
        if (ri % NW == (uint32_t)wave) keep_ok = false, walk_raw(r0 + (uint32_t)__builtin_ctzll(mr), fn);
    }
  };
  // ---- pass 1: tile counts ---------------------------------------------------------------------------------------------
  walk([&](uint32_t, bool hit, int tlo, int thi) {
    if (hit)
      for (int tx = tlo; tx <= thi; ++tx) atomicAdd(&s_cnt[tx], 1u);
  });
  __syncthreads();
  // ---- scan (wave 0) + the band's allocation -----------------------------------------------------------------------------
  if (wave == 0) {
    uint32_t run = 0;
    for (uint32_t t0 = 0; t0 < TX; t0 += 64) {
      const uint32_t tx = t0 + lane;
      const uint32_t v = tx < TX ? s_cnt[tx] : 0u;
      const uint32_t incl = wave_scan_add(v);
      if (tx < TX) s_off[tx] = run + incl - v;
      run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (lane == 0) {
      uint32_t base = 0;
      if (run) {
        const uint32_t sub = wg & a.pool_sub_mask;
        const uint32_t start = atomicAdd(&a.pool_heads[sub * CNT_STRIDE], run); // (also the host's measure of what the render needed)
        base = (start <= a.pool_sub_cap && run <= a.pool_sub_cap - start) ? sub * a.pool_sub_cap + start : UNLISTED;
      }
      s_misc[0] = base, s_misc[1] = run;
    }
  }
  __syncthreads();
  const uint32_t base = s_misc[0];
  {
    uint2 *ti = a.tile_info + ((size_t)frame * a.n_local_bands + lb) * TX;
    for (uint32_t tx = threadIdx.x; tx < TX; tx += blockDim.x) ti[tx] = make_uint2(s_cnt[tx], base == UNLISTED ? UNLISTED : base + s_off[tx]);
  }
  if (base == UNLISTED || s_misc[1] == 0u) return; // workgroup-uniform
  // ---- pass 2: fill ------------------------------------------------------------------------------------------------------
  // The band's lists hold 4-byte triangle indices (the rasteriser gathers the positions of an index itself): they are
  // assembled in LDS — slots handed out by LDS atomics, tile after tile — and leave as ONE run of coalesced stores.  A band
  // with more pairs than the stage holds stores its indices straight into the pool.
  uint32_t *out = a.pool + base;
  const uint32_t run = s_misc[1];
  const bool staged = run <= BIN_STAGE; // workgroup-uniform
  auto fill = [&](uint32_t t, bool hit, int tlo, int thi) {
    if (hit)
      for (int tx = tlo; tx <= thi; ++tx) {
        const uint32_t slot = s_off[tx] + atomicAdd(&s_fill[tx], 1u);
        if (staged)
          s_stage[slot] = t;
        else
          out[slot] = t;
      }
  };
  if (keep_ok && n_seen <= KEEP) { // (wave-uniform) everything this wave met on the first walk is still in LDS: no second walk
    for (uint32_t k = 0; k < n_seen; ++k) {
      const u32x2 en = s_keep[k * 64u + (uint32_t)lane];
      fill(en.x, true, (int)(en.y & 0xffffu), (int)(en.y >> 16)); // (a lane without an entry kept tiles 1 .. 0)
    }
  } else {
    n_seen = KEEP; // (nothing more is kept)
    walk(fill);
  }
  if (staged) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < run; i += blockDim.x) out[i] = s_stage[i];
  }
}

// ================================================================================================================
// Fragment shaders
// ================================================================================================================
struct FrameK { // per-frame constants, wave-uniform (live in SGPRs)
  float eye[3], ka[3], ks[3], p, kh, kn;
  uint32_t n_lights;
  // FD_GREY (decided on the host): ka, ks and every light's intensity have three bit-equal channels.  The three channels of a
  // Blinn-Phong sum then differ only through the surface colour kd: with kd = (1, 1, 1) — the PHONG shader — they are the SAME
  // operations on the SAME operands, so the FAST builds compute one channel and copy it (identical bits by construction).  Only
  // BEHIND a pixel's light terms: a branch inside them (one division instead of three in the scalar path) cost the TEXTURE builds
  // 1.5 % — the terms are kept one straight line so that their independent normalisations interleave
  bool grey;
  const SRZ_CAS srz_light *lights;
};
struct ShadeDesc { // what a batch's Shader object holds: type + texture (Shader::texture, width_256/height_256)
  int shader, tw, th;
  const SRZ_CAS uint32_t *tex;
};

// BlinnPhong<__m256> for one light (include/shader/Shader.hpp:104-229)
template <class M, int NL>
__device__ __forceinline__ void v_blinn_phong(M &m, float nx, float ny, float nz, const FrameK &K, float kdr, float kdg, float kdb,
                                              const SRZ_CAS srz_light *L, float px, float py, float pz, float &o0, float &o1,
                                              float &o2) {
  const float Lx = L->pos[0], Ly = L->pos[1], Lz = L->pos[2], I0 = L->intensity[0], I1 = L->intensity[1], I2 = L->intensity[2];
  float lx = Lx - px, ly = Ly - py, lz = Lz - pz;
  float att = m.rsqrt2(fmaf_(lx, lx, ly * ly));
  float d0 = I0 * att, d1 = I1 * att, d2 = I2 * att;
  float hx = lx + (K.eye[0] - px), hy = ly + (K.eye[1] - py), hz = lz + (K.eye[2] - pz);
  v_normalized(m, hx, hy, hz);
  float nlx = lx, nly = ly, nlz = lz;
  v_normalized(m, nlx, nly, nlz);
  float cosA = sse_max(0.0f, fmaf_(nlx, nx, fmaf_(nly, ny, nlz * nz)));
  float cosT = pow_frame<NL>(m, sse_max(0.0f, fmaf_(hx, nx, fmaf_(hy, ny, hz * nz))), K.p);
  o0 = kdr * fmaf_(K.ka[0], I0, fmaf_(d0 * kdr, cosA, (d0 * K.ks[0]) * cosT));
  o1 = kdg * fmaf_(K.ka[1], I1, fmaf_(d1 * kdg, cosA, (d1 * K.ks[1]) * cosT));
  o2 = kdb * fmaf_(K.ka[2], I2, fmaf_(d2 * kdb, cosA, (d2 * K.ks[2]) * cosT));
}
// The same light in two steps: everything that does not involve the surface colour kd (attenuation, the two cosines, the
// power), then the combination.  The FAST build runs step 1 for BOTH lights between issuing the texel load and using it, so
// the load's latency passes under ~200 instructions instead of ~70 (same operations on the same operands: same bits).
struct LightTerms {
  float d0, d1, d2, cosA, cosT;
};
template <class M, int NL>
__device__ __forceinline__ void v_blinn_phong_terms(M &m, float nx, float ny, float nz, const FrameK &K, const SRZ_CAS srz_light *L,
                                                    float px, float py, float pz, LightTerms &t) {
  const float Lx = L->pos[0], Ly = L->pos[1], Lz = L->pos[2], I0 = L->intensity[0], I1 = L->intensity[1], I2 = L->intensity[2];
  float lx = Lx - px, ly = Ly - py, lz = Lz - pz;
  float att = m.rsqrt2(fmaf_(lx, lx, ly * ly));
  t.d0 = I0 * att, t.d1 = I1 * att, t.d2 = I2 * att;
  float hx = lx + (K.eye[0] - px), hy = ly + (K.eye[1] - py), hz = lz + (K.eye[2] - pz);
  v_normalized(m, hx, hy, hz);
  float nlx = lx, nly = ly, nlz = lz;
  v_normalized(m, nlx, nly, nlz);
  t.cosA = sse_max(0.0f, fmaf_(nlx, nx, fmaf_(nly, ny, nlz * nz)));
  t.cosT = pow_frame<NL>(m, sse_max(0.0f, fmaf_(hx, nx, fmaf_(hy, ny, hz * nz))), K.p);
}
__device__ __forceinline__ void v_blinn_phong_combine(const FrameK &K, const SRZ_CAS srz_light *L, const LightTerms &t, float kdr,
                                                      float kdg, float kdb, float &o0, float &o1, float &o2) {
  const float I0 = L->intensity[0], I1 = L->intensity[1], I2 = L->intensity[2];
  o0 = kdr * fmaf_(K.ka[0], I0, fmaf_(t.d0 * kdr, t.cosA, (t.d0 * K.ks[0]) * t.cosT));
  o1 = kdg * fmaf_(K.ka[1], I1, fmaf_(t.d1 * kdg, t.cosA, (t.d1 * K.ks[1]) * t.cosT));
  o2 = kdb * fmaf_(K.ka[2], I2, fmaf_(t.d2 * kdb, t.cosA, (t.d2 * K.ks[2]) * t.cosT));
}

// Shader::applyFragmentShader SIMD overload + simd_*_impl (src/Shader.cpp:128-386); colour out in [0,255]
template <class M, int SH, int NL>
__device__ __forceinline__ void v_shade(M &m, const FrameK &K, const ShadeDesc &sd, float px, float py, float pz, float nx, float ny,
                                        float nz, float u, float v, float &r0, float &r1, float &r2) {
  const int shader = SH >= 0 ? SH : sd.shader;
  constexpr int NLC = light_count<NL>();
  const uint32_t n_lights = NLC > 0 ? (uint32_t)NLC : K.n_lights;
  float c0 = 1.0f, c1 = 1.0f, c2 = 1.0f;
  if (shader == SRZ_SHADER_NORMAL) {
    c0 = (nx + 1.0f) * 0.5f, c1 = (ny + 1.0f) * 0.5f, c2 = (nz + 1.0f) * 0.5f;
  } else if (shader == SRZ_SHADER_TEXTURE || shader == SRZ_SHADER_PHONG) {
    float kd0 = 1.0f, kd1 = 1.0f, kd2 = 1.0f;
    uint32_t texel = 0u;
    if (shader == SRZ_SHADER_TEXTURE) {
      float tw = (float)sd.tw, th = (float)sd.th;
      u = u * tw, v = v * th;
      u = sse_max(0.0f, sse_min(u, tw - 1.0f));
      v = sse_max(0.0f, sse_min(v, th - 1.0f));
      int32_t xi = cvt_rne_i32(u), yi = cvt_rne_i32(v);
      texel = sd.tex[(size_t)yi * sd.tw + xi];
    }
    auto decode = [&]() {
      if (shader == SRZ_SHADER_TEXTURE) {
        const float inv255 = 1.0f / 255.0f;
        kd0 = (float)(texel & 0xffu) * inv255, kd1 = (float)((texel >> 8) & 0xffu) * inv255,
        kd2 = (float)((texel >> 16) & 0xffu) * inv255;
      }
    };
    c0 = c1 = c2 = 0.0f;
    if constexpr (NLC > 0) { // every light's colour-independent terms first, the texel only after them
      LightTerms t[NLC];
#pragma unroll
      for (int l = 0; l < NLC; ++l) v_blinn_phong_terms<M, NL>(m, nx, ny, nz, K, K.lights + l, px, py, pz, t[l]);
      asm volatile("" : "+v"(t[0].cosT), "+v"(t[NLC - 1].cosT), "+v"(texel)); // (keeps the decode below the terms)
      decode();
      if (SH == SRZ_SHADER_PHONG && K.grey) { // (wave-uniform) kd = 1 and grey constants: channel 0's operations ARE the other two's
#pragma unroll
        for (int l = 0; l < NLC; ++l) {
          const float I0 = (K.lights + l)->intensity[0];
          c0 = c0 + 1.0f * fmaf_(K.ka[0], I0, fmaf_(t[l].d0 * 1.0f, t[l].cosA, (t[l].d0 * K.ks[0]) * t[l].cosT));
        }
        r0 = r1 = r2 = sse_min(sse_max(c0, 0.0f), 1.0f) * 255.0f;
        return;
      }
#pragma unroll
      for (int l = 0; l < NLC; ++l) { // (summed in the lights' order, like the loop below)
        float o0, o1, o2;
        v_blinn_phong_combine(K, K.lights + l, t[l], kd0, kd1, kd2, o0, o1, o2);
        c0 = c0 + o0, c1 = c1 + o1, c2 = c2 + o2;
      }
    } else {
      decode();
      for (uint32_t l = 0; l < n_lights; ++l) {
        float o0, o1, o2;
        v_blinn_phong<M, NL>(m, nx, ny, nz, K, kd0, kd1, kd2, K.lights + l, px, py, pz, o0, o1, o2);
        c0 = c0 + o0, c1 = c1 + o1, c2 = c2 + o2;
      }
    }
  }
  // DISPLACEMENT / BUMP: the reference's SIMD versions are empty stubs (src/Shader.cpp:388-444) → (1,1,1) → 255
  r0 = sse_min(sse_max(c0, 0.0f), 1.0f) * 255.0f;
  r1 = sse_min(sse_max(c1, 0.0f), 1.0f) * 255.0f;
  r2 = sse_min(sse_max(c2, 0.0f), 1.0f) * 255.0f;
}

// TextureLoader::getTextureColor(vec2) (src/TextureLoader.cpp:14-31)
template <class M>
__device__ __forceinline__ void s_texel(M &m, const ShadeDesc &sd, float u, float v, float &o0, float &o1, float &o2) {
  float cu = std_clamp(u, 0.0f, 1.0f), cv = std_clamp(v, 0.0f, 1.0f);
  float fx = cu * (float)sd.tw, fy = cv * (float)sd.th;
  int x = cvt_trunc_i32(fx), y = cvt_trunc_i32(fy);
  if (x < 0 || x >= sd.tw || y < 0 || y >= sd.th) {
    o0 = o1 = o2 = 0.0f;
    return;
  }
  uint32_t texel = sd.tex[(size_t)y * sd.tw + x];
  o0 = m.div255((float)(texel & 0xffu)), o1 = m.div255((float)((texel >> 8) & 0xffu)),
  o2 = m.div255((float)((texel >> 16) & 0xffu));
}

// Shader::BlinnPhong scalar (src/Shader.cpp:510-543); the two std::pow(x,2) and the sqrt are binary64 there
template <class M, int NL>
__device__ __forceinline__ void s_blinn_phong(M &m, const FrameK &K, float px, float py, float pz, float nx, float ny, float nz,
                                              float kd0, float kd1, float kd2, const SRZ_CAS srz_light *L, float &o0, float &o1,
                                              float &o2) {
  const float Lx = L->pos[0], Ly = L->pos[1], Lz = L->pos[2], I0 = L->intensity[0], I1 = L->intensity[1], I2 = L->intensity[2];
  normalize3(m, nx, ny, nz);
  float ldx = Lx - px, ldy = Ly - py, ldz = Lz - pz;
  float dsq = m.len2d(ldx, ldy); // (binary64 in the reference: std::pow(x, 2), std::sqrt)
  float d0, d1, d2;
  m.div3(I0, I1, I2, dsq, d0, d1, d2);
  float nlx = ldx, nly = ldy, nlz = ldz;
  normalize3(m, nlx, nly, nlz);
  float cosTheta = std_max(0.0f, dot3(nx, ny, nz, nlx, nly, nlz));
  float vx = K.eye[0] - px, vy = K.eye[1] - py, vz = K.eye[2] - pz;
  float hx = ldx + vx, hy = ldy + vy, hz = ldz + vz;
  normalize3(m, hx, hy, hz);
  float cosAlpha = std_max(0.0f, dot3(nx, ny, nz, hx, hy, hz));
  float pw = pow_frame<NL>(m, cosAlpha, K.p);
  o0 = ((K.ka[0] * I0 + (cosTheta * kd0) * d0) + (pw * K.ks[0]) * d0) * kd0;
  o1 = ((K.ka[1] * I1 + (cosTheta * kd1) * d1) + (pw * K.ks[1]) * d1) * kd1;
  o2 = ((K.ka[2] * I2 + (cosTheta * kd2) * d2) + (pw * K.ks[2]) * d2) * kd2;
}
// the same light in two steps (see v_blinn_phong_terms): cosA = cosTheta, cosT = pow(cosAlpha, p)
template <class M, int NL>
__device__ __forceinline__ void s_blinn_phong_terms(M &m, const FrameK &K, float px, float py, float pz, float nx, float ny, float nz,
                                                    const SRZ_CAS srz_light *L, LightTerms &t) {
  const float Lx = L->pos[0], Ly = L->pos[1], Lz = L->pos[2], I0 = L->intensity[0], I1 = L->intensity[1], I2 = L->intensity[2];
  normalize3(m, nx, ny, nz);
  float ldx = Lx - px, ldy = Ly - py, ldz = Lz - pz;
  float dsq = m.len2d(ldx, ldy); // (binary64 in the reference: std::pow(x, 2), std::sqrt)
  m.div3(I0, I1, I2, dsq, t.d0, t.d1, t.d2); // (no branch on FrameK::grey here: the terms of a pixel stay one straight line of code)
  float nlx = ldx, nly = ldy, nlz = ldz;
  normalize3(m, nlx, nly, nlz);
  t.cosA = std_max(0.0f, dot3(nx, ny, nz, nlx, nly, nlz));
  float vx = K.eye[0] - px, vy = K.eye[1] - py, vz = K.eye[2] - pz;
  float hx = ldx + vx, hy = ldy + vy, hz = ldz + vz;
  normalize3(m, hx, hy, hz);
  float cosAlpha = std_max(0.0f, dot3(nx, ny, nz, hx, hy, hz));
  t.cosT = pow_frame<NL>(m, cosAlpha, K.p);
}
__device__ __forceinline__ void s_blinn_phong_combine(const FrameK &K, const SRZ_CAS srz_light *L, const LightTerms &t, float kd0,
                                                      float kd1, float kd2, float &o0, float &o1, float &o2) {
  const float I0 = L->intensity[0], I1 = L->intensity[1], I2 = L->intensity[2];
  o0 = ((K.ka[0] * I0 + (t.cosA * kd0) * t.d0) + (t.cosT * K.ks[0]) * t.d0) * kd0;
  o1 = ((K.ka[1] * I1 + (t.cosA * kd1) * t.d1) + (t.cosT * K.ks[1]) * t.d1) * kd1;
  o2 = ((K.ka[2] * I2 + (t.cosA * kd2) * t.d2) + (t.cosT * K.ks[2]) * t.d2) * kd2;
}
// s_texel in two steps for the FAST build: the load from an address that is always inside the image (the reference's
// out-of-range case — u or v == 1.0 → index == size → black — becomes a select afterwards), so it is not inside a branch
// and can stay in flight across the lights' terms
__device__ __forceinline__ uint32_t s_texel_issue(const ShadeDesc &sd, float u, float v, bool &inside) {
  float cu = std_clamp(u, 0.0f, 1.0f), cv = std_clamp(v, 0.0f, 1.0f);
  float fx = cu * (float)sd.tw, fy = cv * (float)sd.th;
  int x = cvt_trunc_i32(fx), y = cvt_trunc_i32(fy);
  inside = !(x < 0 || x >= sd.tw || y < 0 || y >= sd.th);
  const int xs = min(max(x, 0), sd.tw - 1), ys = min(max(y, 0), sd.th - 1);
  return sd.tex[(size_t)ys * sd.tw + xs];
}

// calcBumpMapping / calcDisplacementMapping common part (src/Shader.cpp:447-507)
template <class M>
__device__ __forceinline__ void s_bump_common(M &m, const ShadeDesc &sd, float nx, float ny, float nz, float u, float v, float kh,
                                              float kn, float &ox, float &oy, float &oz, float &origin_norm) {
  float sq = __builtin_sqrtf(nx * nx + nz * nz);
  float t0 = (nx * ny) / sq, t1 = sq, t2 = (nz * ny) / sq;
  float b0 = ny * t2 - t1 * nz, b1 = nz * t0 - t2 * nx, b2 = nx * t1 - t0 * ny;
  float a0, a1, a2, u0, u1, u2, w0, w1, w2;
  s_texel(m, sd, u, v, a0, a1, a2);
  float on = __builtin_sqrtf(dot3(a0, a1, a2, a0, a1, a2));
  s_texel(m, sd, (u + 1.0f) / (float)sd.tw, v, u0, u1, u2);
  s_texel(m, sd, u, (v + 1.0f) / (float)sd.th, w0, w1, w2);
  float dU = kh * kn * (__builtin_sqrtf(dot3(u0, u1, u2, u0, u1, u2)) - on);
  float dV = kh * kn * (__builtin_sqrtf(dot3(w0, w1, w2, w0, w1, w2)) - on);
  float l0 = -dU, l1 = -dV, l2 = 1.0f;
  ox = t0 * l0 + t1 * l1 + t2 * l2, oy = b0 * l0 + b1 * l1 + b2 * l2, oz = nx * l0 + ny * l1 + nz * l2;
  normalize3(m, ox, oy, oz);
  origin_norm = on;
}

// scalar applyFragmentShader + standard_*_impl + Tools::normalizedToRGB (src/Shader.cpp:547-640, src/Tools.cpp:94-104)
template <class M, int SH, int NL>
__device__ __forceinline__ void s_shade(M &m, const FrameK &K, const ShadeDesc &sd, float px, float py, float pz, float nx, float ny,
                                        float nz, float u, float v, float &r0, float &r1, float &r2) {
  const int shader = SH >= 0 ? SH : sd.shader;
  constexpr int NLC = light_count<NL>();
  const uint32_t n_lights = NLC > 0 ? (uint32_t)NLC : K.n_lights;
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  if (shader == SRZ_SHADER_NORMAL) {
    normalize3(m, nx, ny, nz);
    c0 = (nx + 1.0f) / 2.0f, c1 = (ny + 1.0f) / 2.0f, c2 = (nz + 1.0f) / 2.0f;
  } else if (shader >= SRZ_SHADER_TEXTURE && shader <= SRZ_SHADER_BUMP) {
    float kd0 = 1.0f, kd1 = 1.0f, kd2 = 1.0f;
    float sx = px, sy = py, sz = pz, snx = nx, sny = ny, snz = nz;
    if constexpr (NLC > 0 && (SH == SRZ_SHADER_TEXTURE || SH == SRZ_SHADER_PHONG)) {
      // FAST build: texel load issued first, every light's colour-independent terms, then the texel and the combination
      bool inside = true;
      uint32_t texel = 0u;
      if (SH == SRZ_SHADER_TEXTURE) texel = s_texel_issue(sd, u, v, inside);
      LightTerms t[NLC];
#pragma unroll
      for (int l = 0; l < NLC; ++l) s_blinn_phong_terms<M, NL>(m, K, sx, sy, sz, snx, sny, snz, K.lights + l, t[l]);
      asm volatile("" : "+v"(t[0].cosT), "+v"(t[NLC - 1].cosT), "+v"(texel));
      if (SH == SRZ_SHADER_TEXTURE) {
        kd0 = m.div255((float)(texel & 0xffu)), kd1 = m.div255((float)((texel >> 8) & 0xffu)), kd2 = m.div255((float)((texel >> 16) & 0xffu));
        if (!inside) kd0 = kd1 = kd2 = 0.0f;
      }
      if (SH == SRZ_SHADER_PHONG && K.grey) { // (wave-uniform) kd = 1 and grey constants: one channel, copied (see FrameK::grey)
#pragma unroll
        for (int l = 0; l < NLC; ++l) {
          const float I0 = (K.lights + l)->intensity[0];
          c0 = c0 + ((K.ka[0] * I0 + (t[l].cosA * 1.0f) * t[l].d0) + (t[l].cosT * K.ks[0]) * t[l].d0) * 1.0f;
        }
        const float q = std_clamp(c0, 0.0f, 1.0f) * 255.0f;
        r0 = r1 = r2 = (q == q) ? (float)(uint32_t)q : 0.0f;
        return;
      }
#pragma unroll
      for (int l = 0; l < NLC; ++l) {
        float o0, o1, o2;
        s_blinn_phong_combine(K, K.lights + l, t[l], kd0, kd1, kd2, o0, o1, o2);
        c0 = c0 + o0, c1 = c1 + o1, c2 = c2 + o2;
      }
    } else {
    if (shader != SRZ_SHADER_PHONG) s_texel(m, sd, u, v, kd0, kd1, kd2);
    if (shader == SRZ_SHADER_BUMP) {
      float on;
      s_bump_common(m, sd, nx, ny, nz, u, v, K.kh, K.kn, snx, sny, snz, on);
    } else if (shader == SRZ_SHADER_DISPLACEMENT) {
      float on;
      s_bump_common(m, sd, nx, ny, nz, u, v, K.kh, K.kn, snx, sny, snz, on);
      sx = px + (K.kn * nx) * on, sy = py + (K.kn * ny) * on, sz = pz + (K.kn * nz) * on;
    }
    for (uint32_t l = 0; l < n_lights; ++l) {
      float o0, o1, o2;
      s_blinn_phong<M, NL>(m, K, sx, sy, sz, snx, sny, snz, kd0, kd1, kd2, K.lights + l, o0, o1, o2);
      c0 = c0 + o0, c1 = c1 + o1, c2 = c2 + o2;
    }
    }
  }
  float q0 = std_clamp(c0, 0.0f, 1.0f) * 255.0f, q1 = std_clamp(c1, 0.0f, 1.0f) * 255.0f,
        q2 = std_clamp(c2, 0.0f, 1.0f) * 255.0f;
  r0 = (q0 == q0) ? (float)(uint32_t)q0 : 0.0f;
  r1 = (q1 == q1) ? (float)(uint32_t)q1 : 0.0f;
  r2 = (q2 == q2) ? (float)(uint32_t)q2 : 0.0f;
}

// ---- the hand-off: what the rasterisers (k_raster, k_raster_slow) leave for k_shade / k_visibility per OWNED tile -------------
// 1. A WORK ENTRY in one of 104 work lists: [build that shades the frame: FAST for 1 / 2 / 3 / 4 lights, the same for frames with
//    BUMP / DISPLACEMENT batches, the same for frames with a non-integer exponent, generic][frame % 8] (frame % 8 = the XCD that
//    rasterised it), in arrival order — k_raster's workgroups run in frame order, so every list comes out (roughly) frame by frame.
//    The lists exist only for the kinds the set's frames need: list [kind][sub] lives in storage slot work_slot(), the counters in
//    work_count[] are indexed by kind * 8 + sub (all of them exist).  An entry = {frame, local band | tile x << 10 | WORK_LP |
//    WORK_LP8, entries of the tile's triangle list, its first index in pool[]}: everything k_shade needs to start the tile's loads
//    travels with it, and nothing has to be divided out of a flat tile number (two scalar software divisions per tile otherwise).
// 2. The OWNER of every pixel, in the tile's slot of `vis` (PIX_SLOT entries, pixel p = ly * 32 + lx), in one of three widths:
//    - 32 bits (no flag): its index in the frame | S_CLASS_BIT, NO_TRI = nobody — the ordered rasteriser, long lists;
//    - 16 bits (WORK_LP): its POSITION in the tile's triangle list | 0x8000 for the S class, 0xffff = nobody — k_raster, tiles of at
//      most LP_MAX list entries in frames of fewer than 2^22 - 1 triangles: the position rides in the low bits of the depth key's
//      tie-break, below the triangle index, so the pixel's final key holds it for free.  k_shade then stages the list's triangles
//      in LDS once per tile and every pixel reads its owner's 96 bytes from there instead of gathering them from memory; and a
//      frame of 94 k triangles pays 2 bytes per pixel like one of 5 k;
//    - 8 bits (WORK_LP | WORK_LP8): the same for lists of at most LP8_MAX entries (most tiles of every BASELINE config), position |
//      0x80 for the S class, 0xff = nobody: 1 + 1 instead of 2 + 2 bytes per pixel of every owned tile written and read back, during
//      the part of a step in which the memory system is what everything waits for (NOTEBOOK r6 §2).
//    The S class: the pixel lies in the scalar-tail ("S") columns of its owner's bounding box.
// 3. The tile's RECTANGLE in the framebuffer: tile_rect().
// HELPER — k_shade's inline copy of it (any call in its tile loop moves its schedule; each copy names its helper; a fix goes into both):
//    work_decode, id_none / id_sbit, ids_load_raw, ids_unpack4 — shade_tile: head, step 1 and the classification
//    tile_rect — shade_tile, behind the FrameDesc loads
//    (k_gbuffer CALLS tile_rect, the owner-id constants, v_normalized, normalize3, s_texel and cvt_rne_i32; its copy of v_shade's prologue
//    and fetch and of shade_bary_v / _s's interpolation names them; k_motion CALLS tile_rect, the owner-id constants and load_pos9, its
//    copy of cover_v / cover_s's z interpolation names them; k_interp and k_interp_grad CALL tile_rect, quad_store, quad_at and the
//    owner-id constants, their copy of shade_bary_v / _s's uv interpolation names them; k_pos_grad CALLS the same and load_pos9, its
//    copy of k_interp_grad's scan, table and flush names them)
//    frame_k — class_pass, head
//    shade_bary_v / _s — the second half of shade_pixel_v / _s
// (copies without a helper: k_shade_vis's compaction and batch-by-batch loop, of k_shade's; k_visibility's o[3][4], of quad_load / quad_at)
constexpr uint32_t WORK_LP = 1u << 20, WORK_LP8 = 1u << 21;
constexpr uint32_t S_CLASS_BIT = 0x80000000u;
constexpr uint32_t PIX_SLOT = TILE * TILE, PIX_BITS = 10, PIX_MASK = PIX_SLOT - 1u;
constexpr uint32_t LP_BITS = 9, LP_MAX = 1u << LP_BITS; // (idx << 9 | position) <= 0x7ffffffe for idx < 2^22 - 1 (FD_PACKED)
static_assert(31 - LP_BITS == PACK_IDX_BITS, "the tie-break holds an index of PACK_IDX_BITS bits above the list position");
constexpr uint32_t LP8_MAX = 127;
__device__ __forceinline__ uint32_t id_pack8(uint32_t id) { return id == NO_TRI ? 0xffu : ((id & 127u) | ((id >> 24) & 0x80u)); }
__device__ __forceinline__ uint32_t id_pack16(uint32_t id) { return id == NO_TRI ? 0xffffu : ((id & (LP_MAX - 1u)) | ((id >> 16) & 0x8000u)); }

__device__ __forceinline__ uint4 work_entry(uint32_t frame, uint32_t lb, uint32_t tx, bool by_lp, bool lp8, uint32_t cnt, uint32_t off) {
  return make_uint4(frame, lb | (tx << 10) | (by_lp ? WORK_LP : 0u) | (lp8 ? WORK_LP8 : 0u), cnt, off);
}
struct Work {
  uint32_t f, lb, tx, cnt, off;
  bool by_lp, lp8; // the owner ids' width: 16 bits (by_lp), 8 (by_lp && lp8), else 32
};
__device__ __forceinline__ Work work_decode(u32x4 x) {
  return {x.x, x.y & 1023u, (x.y >> 10) & 1023u, x.z, x.w, (x.y & WORK_LP) != 0u, (x.y & WORK_LP8) != 0u};
}
template <class A> __device__ __forceinline__ uint32_t work_slot(A &a, uint32_t kind, uint32_t sub) {
  return ((uint32_t)(a.kind_slots >> (4u * kind)) & 15u) * 8u + sub;
}
__device__ __forceinline__ void work_append(const RenderArgs &a, uint32_t frame_flags, uint32_t entry /* frame * tiles + tile */, const uint4 &w) {
  // (fewer than 8 frames: the tiles are dealt over the 8 lists instead, so that every XCD has work)
  const uint32_t kind = a.force_generic ? SHADE_KIND_GENERIC : frame_kind(frame_flags);
  const uint32_t sub = (a.n_frames >= 8u ? w.x : w.x + entry) & 7u;
  a.worklist[(size_t)work_slot(a, kind, sub) * a.work_cap + atomicAdd(&a.work_count[(kind * 8u + sub) * CNT_STRIDE], 1u)] = w;
}

// the owners of pixels p0 .. p0 + 3 of a tile (p0 % 4 == 0) into / out of its slot.  Reading is two steps: the raw load, and
// ids_unpack4 into one id per pixel in the width's own code (compared with id_none / id_sbit, never widened)
__device__ __forceinline__ void ids_store4(uint32_t *slot, uint32_t p0, const uint4 &id, bool by_lp, bool lp8) {
  if (lp8) {
    *reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(slot) + p0) = id_pack8(id.x) | (id_pack8(id.y) << 8) | (id_pack8(id.z) << 16) | (id_pack8(id.w) << 24);
  } else if (by_lp) {
    const u32x2 w = {id_pack16(id.x) | (id_pack16(id.y) << 16), id_pack16(id.z) | (id_pack16(id.w) << 16)};
    *reinterpret_cast<u32x2 *>(reinterpret_cast<uint16_t *>(slot) + p0) = w;
  } else {
    *reinterpret_cast<uint4 *>(slot + p0) = id;
  }
}
__device__ __forceinline__ uint4 ids_load_raw(const uint32_t *slot, uint32_t p0, bool by_lp, bool lp8) {
  uint4 raw = make_uint4(0u, 0u, 0u, 0u);
  if (lp8) {
    raw.x = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(slot) + p0);
  } else if (by_lp) {
    const u32x2 w = *reinterpret_cast<const u32x2 *>(reinterpret_cast<const uint16_t *>(slot) + p0);
    raw.x = w.x, raw.y = w.y;
  } else {
    raw = *reinterpret_cast<const uint4 *>(slot + p0);
  }
  return raw;
}
__device__ __forceinline__ void ids_unpack4(const uint4 &raw, bool by_lp, bool lp8, uint32_t id[4]) {
  id[0] = raw.x, id[1] = raw.y, id[2] = raw.z, id[3] = raw.w;
  if (lp8)
    id[0] = raw.x & 0xffu, id[1] = (raw.x >> 8) & 0xffu, id[2] = (raw.x >> 16) & 0xffu, id[3] = raw.x >> 24;
  else if (by_lp)
    id[0] = raw.x & 0xffffu, id[1] = raw.x >> 16, id[2] = raw.y & 0xffffu, id[3] = raw.y >> 16;
}
__device__ __forceinline__ uint32_t id_none(bool by_lp, bool lp8) { return lp8 ? 0xffu : by_lp ? 0xffffu : NO_TRI; }
__device__ __forceinline__ uint32_t id_sbit(bool by_lp, bool lp8) { return lp8 ? 0x80u : by_lp ? 0x8000u : S_CLASS_BIT; }

// A tile's pixels [tx0, tx1] x [ty0, ty1] (frame coordinates, clipped to the frame), the floats between two planes of `out`, and
// plane 0 (z) at row ty0 (local band lb's first row).  `A` is RenderArgs or k_shade's kernarg view of it.
struct TileRect {
  int tx0, ty0, tx1, ty1;
  size_t plane;
  float *out0;
};
template <class A>
__device__ __forceinline__ TileRect tile_rect(A &a, const SRZ_CAS FrameDesc *fd, uint32_t frame, uint32_t lb, uint32_t tx) {
  const int W = fd->width, H = fd->height;
  TileRect r;
  r.tx0 = (int)tx * TILE, r.ty0 = band_of((int)lb, a.shard_rank, a.shard_world) * BAND;
  r.tx1 = min(r.tx0 + TILE, W) - 1, r.ty1 = min(r.ty0 + BAND, H) - 1;
  r.plane = (size_t)a.local_rows * (size_t)W;
  r.out0 = a.out + (size_t)frame * a.frame_stride + (size_t)lb * BAND * (size_t)W;
  return r;
}

// The frame's shading constants (scalar loads from one hot line; `lights`: the set's, before FrameDesc::light_off)
__device__ __forceinline__ FrameK frame_k(const SRZ_CAS FrameDesc *fd, const SRZ_CAS srz_light *lights) {
  return {{fd->eye[0], fd->eye[1], fd->eye[2]}, {fd->ka[0], fd->ka[1], fd->ka[2]}, {fd->ks[0], fd->ks[1], fd->ks[2]}, fd->p, fd->kh, fd->kn,
          fd->n_lights, (fd->flags & FD_GREY) != 0u, lights + fd->light_off};
}
// A triangle's nine position floats (ax ay z0 bx by z1 cx cy z2) → TriXY in its field order, tri_consts still to come (k_shade: unpack_pos)
template <class P> __device__ __forceinline__ TriXY tri_xy(const P *q) { return {q[0], q[1], q[3], q[4], q[6], q[7], q[2], q[5], q[8]}; }

// Everything the shader needs about the owner triangle of one pixel, fetched in ONE round trip (7 independent loads)
struct TriFetch {
  f32x4 q0, q1, q2, q3, q4, q5;
  uint32_t batch;
};
__device__ __forceinline__ void fetch_tri(const SRZ_CAS srz_tri *tris, const SRZ_CAS uint16_t *tri_batch, uint32_t idx,
                                          TriFetch &f) {
  const SRZ_CAS f32x4 *tp = reinterpret_cast<const SRZ_CAS f32x4 *>(tris + idx);
  f.q0 = tp[0], f.q1 = tp[1], f.q2 = tp[2], f.q3 = tp[3], f.q4 = tp[4], f.q5 = tp[5];
  f.batch = tri_batch[idx];
}

struct TriAttr {
  TriXY t;
  float n0x, n0y, n0z, n1x, n1y, n1z, n2x, n2y, n2z, u0, v0, u1, v1, u2, v2;
};
template <class M> __device__ __forceinline__ void unpack_pos(M &m, const TriFetch &f, TriAttr &a) {
  // pos: q0.xyz q0.w q1.xy q1.zw q2.x
  a.t.ax = f.q0.x, a.t.ay = f.q0.y, a.t.z0 = f.q0.z, a.t.bx = f.q0.w, a.t.by = f.q1.x, a.t.z1 = f.q1.y, a.t.cx = f.q1.z,
  a.t.cy = f.q1.w, a.t.z2 = f.q2.x;
  tri_consts(m, a.t);
}
__device__ __forceinline__ void unpack_attr(const TriFetch &f, TriAttr &a) {
  // nrm: q2.yzw q3.xyz q3.w q4.xy | uv: q4.zw q5.xy q5.zw
  a.n0x = f.q2.y, a.n0y = f.q2.z, a.n0z = f.q2.w, a.n1x = f.q3.x, a.n1y = f.q3.y, a.n1z = f.q3.z, a.n2x = f.q3.w, a.n2y = f.q4.x,
  a.n2z = f.q4.y;
  a.u0 = f.q4.z, a.v0 = f.q4.w, a.u1 = f.q5.x, a.v1 = f.q5.y, a.u2 = f.q5.z, a.v2 = f.q5.w;
}
// A triangle staged in LDS (k_shade, `late` != null) hands over its positions first and its normals / texture coordinates only
// when the barycentrics exist: LDS is close, and 24 values fetched at once are 16 registers held for nothing (the dependency
// on `dep` pins the second half of the reads behind the coverage arithmetic).  From memory (`late` == null) all 96 bytes come
// in ONE round trip, up front.
__device__ __forceinline__ void early_fetch(TriFetch &f, const f32x4 *late) {
  if (late != nullptr) f.q0 = late[0], f.q1 = late[1], f.q2 = late[2];
}
__device__ __forceinline__ void late_fetch(TriFetch &f, const f32x4 *late, float dep) {
  if (late != nullptr) {
    asm volatile("" : "+v"(late) : "v"(dep));
    f.q3 = late[3], f.q4 = late[4], f.q5 = late[5];
  }
}
// The shading from the barycentrics on, given the owner's normals and texture coordinates (a's attributes): k_shade_vis's per-pixel work
// (α, β and z from a visibility buffer).  The second half of shade_pixel_v / _s below is k_shade's inline copy, operation for operation.
template <class M, int SH, int NL>
__device__ __forceinline__ void shade_bary_v(M &m, const FrameK &K, const ShadeDesc &sd, const TriAttr &a, float alpha, float beta,
                                             float gamma, float fx, float fy, float zz, float &r0, float &r1, float &r2) {
  float nx = fmaf_(alpha, a.n0x, fmaf_(beta, a.n1x, gamma * a.n2x));
  float ny = fmaf_(alpha, a.n0y, fmaf_(beta, a.n1y, gamma * a.n2y));
  float nz = fmaf_(alpha, a.n0z, fmaf_(beta, a.n1z, gamma * a.n2z));
  v_normalized(m, nx, ny, nz);
  float u = fmaf_(alpha, a.u0, fmaf_(beta, a.u1, gamma * a.u2));
  float v = fmaf_(alpha, a.v0, fmaf_(beta, a.v1, gamma * a.v2));
  v_shade<M, SH, NL>(m, K, sd, fx, fy, zz, nx, ny, nz, u, v, r0, r1, r2);
}
template <class M, int SH, int NL>
__device__ __forceinline__ void shade_bary_s(M &m, const FrameK &K, const ShadeDesc &sd, const TriAttr &a, float alpha, float beta,
                                             float gamma, float fx, float fy, float zz, float &r0, float &r1, float &r2) {
  float nx = alpha * a.n0x + beta * a.n1x + gamma * a.n2x;
  float ny = alpha * a.n0y + beta * a.n1y + gamma * a.n2y;
  float nz = alpha * a.n0z + beta * a.n1z + gamma * a.n2z;
  normalize3(m, nx, ny, nz);
  float u = alpha * a.u0 + beta * a.u1 + gamma * a.u2;
  float v = alpha * a.v0 + beta * a.v1 + gamma * a.v2;
  s_shade<M, SH, NL>(m, K, sd, fx, fy, zz, nx, ny, nz, u, v, r0, r1, r2);
}
// Shade pixel (x,y) of depth z, owner `f`, 8-wide ("V") semantics (src/Rasterizer.cpp:380-389)
template <class M, int SH = -1, int NL = 0>
__device__ __forceinline__ void shade_pixel_v(M &m, const FrameK &K, const ShadeDesc &sd, const TriFetch &f_in, const f32x4 *late, int x,
                                              int y, float &r0, float &r1, float &r2) {
  TriAttr a;
  TriFetch f; // (a local copy: what the staged reads below define must not outlive this call — the caller's loops would carry it)
  if constexpr (std::is_same<M, ApproxMath>::value) { // (a staged triangle: nothing of f_in but the batch id is defined — copying the
    if (late == nullptr) f = f_in;                    // struct left a dead 4-byte scratch store per chunk in the tolerance builds)
  } else {
    f = f_in;
  }
  early_fetch(f, late);
  unpack_pos(m, f, a);
  const float fx = (float)x, fy = (float)y;
  float alpha, beta, gamma, zz;
  cover_v(a.t, fx, fy, alpha, beta, gamma, zz);
  late_fetch(f, late, gamma);
  unpack_attr(f, a);
  float nx = fmaf_(alpha, a.n0x, fmaf_(beta, a.n1x, gamma * a.n2x));
  float ny = fmaf_(alpha, a.n0y, fmaf_(beta, a.n1y, gamma * a.n2y));
  float nz = fmaf_(alpha, a.n0z, fmaf_(beta, a.n1z, gamma * a.n2z));
  v_normalized(m, nx, ny, nz);
  float u = fmaf_(alpha, a.u0, fmaf_(beta, a.u1, gamma * a.u2));
  float v = fmaf_(alpha, a.v0, fmaf_(beta, a.v1, gamma * a.v2));
  v_shade<M, SH, NL>(m, K, sd, fx, fy, zz, nx, ny, nz, u, v, r0, r1, r2); // zz: the depth k_raster stored (same operations)
}
// scalar-tail ("S") semantics (src/Rasterizer.cpp:470-492)
template <class M, int SH = -1, int NL = 0>
__device__ __forceinline__ void shade_pixel_s(M &m, const FrameK &K, const ShadeDesc &sd, const TriFetch &f_in, const f32x4 *late, int x,
                                              int y, float &r0, float &r1, float &r2) {
  TriAttr a;
  TriFetch f; // (a local copy: what the staged reads below define must not outlive this call — the caller's loops would carry it)
  if constexpr (std::is_same<M, ApproxMath>::value) { // (a staged triangle: nothing of f_in but the batch id is defined — copying the
    if (late == nullptr) f = f_in;                    // struct left a dead 4-byte scratch store per chunk in the tolerance builds)
  } else {
    f = f_in;
  }
  early_fetch(f, late);
  unpack_pos(m, f, a);
  const float fx = (float)x, fy = (float)y;
  float alpha, beta, gamma, zz;
  cover_s(a.t, fx, fy, alpha, beta, gamma, zz);
  late_fetch(f, late, gamma);
  unpack_attr(f, a);
  float nx = alpha * a.n0x + beta * a.n1x + gamma * a.n2x;
  float ny = alpha * a.n0y + beta * a.n1y + gamma * a.n2y;
  float nz = alpha * a.n0z + beta * a.n1z + gamma * a.n2z;
  normalize3(m, nx, ny, nz);
  float u = alpha * a.u0 + beta * a.u1 + gamma * a.u2;
  float v = alpha * a.v0 + beta * a.v1 + gamma * a.v2;
  s_shade<M, SH, NL>(m, K, sd, fx, fy, zz, nx, ny, nz, u, v, r0, r1, r2);
}

#ifdef SRZ_ISA_PROBE
// instruction-count probes (make asm-probe): the two per-pixel shading paths in isolation
__global__ void probe_v(RenderArgs a, float *o) {
  const SRZ_CAS FrameDesc *fd = as_const(a.frames);
  FrameK K = frame_k(fd, as_const(a.lights));
  K.p = 150.0f, K.n_lights = 2; // constants: the static count is the dynamic path
#ifdef SRZ_PROBE_GREY
  K.grey = true;
#else
  K.grey = false;
#endif
  TriFetch tf;
  fetch_tri(as_const(a.tris), as_const(a.tri_batch), threadIdx.x, tf);
  ShadeDesc sd;
  sd.shader = SRZ_SHADER_TEXTURE, sd.tw = 1024, sd.th = 1024, sd.tex = as_const((const uint32_t *)a.vis);
  float r0, r1, r2;
#ifndef SRZ_PROBE_SH
#define SRZ_PROBE_SH -1 /* -1: the generic build's per-pixel generality; 0 / 1 / 2: the FAST variant of that shader type */
#endif
#ifdef SRZ_PROBE_APPROX /* the tolerance mode's policy */
  ApproxMath fm;
#define SRZ_PROBE_M ApproxMath
#else
  FastMath fm;
#define SRZ_PROBE_M FastMath
#endif
#ifdef SRZ_PROBE_S
  shade_pixel_s<SRZ_PROBE_M, SRZ_PROBE_SH, (SRZ_PROBE_SH >= 0 ? 2 : 0)>(fm, K, sd, tf, nullptr, threadIdx.x, blockIdx.x, r0, r1, r2);
#else
  shade_pixel_v<SRZ_PROBE_M, SRZ_PROBE_SH, (SRZ_PROBE_SH >= 0 ? 2 : 0)>(fm, K, sd, tf, nullptr, threadIdx.x, blockIdx.x, r0, r1, r2);
#endif
#ifndef SRZ_PROBE_APPROX
  if (fm.is_bad()) r0 = -1.f;
#endif
  o[threadIdx.x] = r0 + r1 + r2;
}
#endif

// ================================================================================================================
// k_raster — VISIBILITY: one wave per 32x32 tile, ORDER-INDEPENDENT
//
// The reference walks the triangles in submission order; a fragment of the 8-wide ("V") columns replaces the pixel iff
// z < zbuf, one of the scalar-tail ("S") columns iff !(z > zbuf) (src/Rasterizer.cpp:334,475).  For ordinary depths
// (not NaN, not ±0) the pixel's final state is a function of the SET of its fragments:
//     final z = the smallest z;   final owner = the LAST S fragment at that z if there is one (every later S passes <=,
//     no later V passes <), otherwise the FIRST V fragment at that z (later ones fail <); an incoming depth equal to the
//     smallest z keeps the pixel against V fragments and loses it to S fragments.
// So every pixel holds ONE 64-bit key  (order-preserving image of z) << 32 | tie-break  and every fragment is an LDS
// ds_min_u64, in any order:   tie-break = 0x7ffffffe - idx (S)  <  0x7fffffff (incoming depth)  <  0x80000000 | idx (V),
// idx = the triangle's index in the frame = its submission order.
// What the min cannot express is detected and handed to k_raster_slow (the reference's ordered algorithm): a NaN depth
// that passes an S test (S fragments with NaN z and NaN incoming depths get the smallest key, 0) and a final depth of
// ±0 (-0 and +0 compare equal as floats but not as keys); both leave their mark in the pixel's final key.
//
// Because order is irrelevant the tile's (triangle, pixel) candidates can be spread DENSELY over the lanes instead of
// giving every triangle a wave pass of its own.  Per chunk of 64 list records (one per lane, geometry of bbox ∩ tile
// computed in parallel) the work is flattened into ITEMS — a V item is an 8-pixel piece of one bbox row, an S item is one
// pixel of the <= 7 scalar-tail columns — numbered by an exclusive scan of the per-triangle item counts.  A batch of 64
// consecutive items is then one item per lane: the triangles whose first item falls into the batch mark that position in
// LDS, an inclusive max-scan over the marks tells every lane its triangle, whose record comes over the LDS crossbar
// (ds_bpermute), and the lane tests its 8 pixels (V) or its pixel (S) with the reference's arithmetic.
// ================================================================================================================
__device__ __forceinline__ float rl_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ int rl_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ uint32_t f2u(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ __forceinline__ float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }
// streaming 16-byte store: written once, never re-read by this pipeline
// (measured on MI355X, 256 frames of 1024^2, ms per step with this store as nt / plain / sc1 / sc0 sc1 / sc1 nt in k_clear:
// 1.00 / 1.24 / 1.50 / 1.53 / 1.16; nt in k_clear and sc1 in the tile write-outs 1.15: nt everywhere)
__device__ __forceinline__ void store_nt(float *p, const float4 &v) {
  f32x4 w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, reinterpret_cast<f32x4 *>(p));
}
// The quads of N planes `plane` floats apart: pixels x4 .. x4 + 3 of a row at p, p + plane, ... — one 16-byte access per plane if
// the quad is whole, else the pixels up to tx1, pixel by pixel (a frame whose width is not a multiple of 4 has no aligned quads; a
// tile's last quad may end at the frame's edge)
__device__ __forceinline__ float &quad_at(float4 &v, int k) { return reinterpret_cast<float *>(&v)[k]; } // (k: a constant)
__device__ __forceinline__ float quad_at(const float4 &v, int k) { return reinterpret_cast<const float *>(&v)[k]; }
template <int N> __device__ __forceinline__ void quad_store(float *p, size_t plane, const float4 (&v)[N], bool whole, int x4, int tx1) {
  if (whole) {
#pragma unroll
    for (int i = 0; i < N; ++i) store_nt(p + i * plane, v[i]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x4 + k <= tx1)
#pragma unroll
        for (int i = 0; i < N; ++i) p[i * plane + k] = quad_at(v[i], k);
  }
}
// (pixels beyond tx1 keep what v holds)
template <int N> __device__ __forceinline__ void quad_load(const float *p, size_t plane, float4 (&v)[N], bool whole, int x4, int tx1) {
  if (whole) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = *reinterpret_cast<const float4 *>(p + i * plane);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x4 + k <= tx1)
#pragma unroll
        for (int i = 0; i < N; ++i) quad_at(v[i], k) = p[i * plane + k];
  }
}
// order-preserving image of binary32 in u32 (-0 just below +0, negative NaNs below -inf, positive NaNs above +inf)
__device__ __forceinline__ uint32_t zkey_of(float z) {
  const uint32_t b = f2u(z);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float z_of_key(uint32_t k) {
  return u2f(k ^ (~(uint32_t)((int32_t)k >> 31) | 0x80000000u));
}
constexpr uint32_t TB_NONE = 0x7fffffffu; // tie-break of the incoming depth
__device__ __forceinline__ float bperm_f(int addr, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ uint32_t bperm_u(int addr, uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)v); }

// WAVES = 1: the throughput build (batches: thousands of tiles in flight, one wave each).  WAVES = 4: the latency build for
// jobs of a few frames, where a frame is as slow as its heaviest tile — the four waves of a tile share its keys (the LDS
// minimum is atomic across waves), each loads the chunk's records and takes every fourth batch of 64 items and a quarter of
// the init / decode / write-out rows.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES, WAVES == 1 ? 5 : 1) void k_raster(RenderArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_key[TILE * KEY_STRIDE];
  __shared__ uint32_t s_mark_x[WAVES > 1 ? WAVES * 64 : 1]; // WAVES > 1: the item marks of each wave (one wave: the keys' pad column)
  __shared__ uint32_t s_wg[WAVES > 1 ? 3 : 1];              // WAVES > 1: redo / owner flags of the tile, the farthest depth
  constexpr int ITS = 4 / WAVES;                            // 8-row strips of the tile per wave in the row-wise phases

  const int lane = threadIdx.x & 63;
  const int wave = WAVES > 1 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
  auto wg_barrier = [] {
    if constexpr (WAVES > 1)
      __syncthreads();
    else
      __builtin_amdgcn_wave_barrier();
  };
  // XCD-aware tile assignment.  Workgroups are dealt round-robin to the 8 XCDs in launch order, and launch order is
  // strict: one XCD whose slots are full of long tiles stalls the dispatch of everything behind it.  So workgroup i
  // renders frame (i % 8) of its group of 8 frames: the 8 XCDs walk the SAME tile sequence in lockstep (balanced by
  // construction), and all tiles of one frame — hence its tile lists — live in ONE XCD's L2.
  const uint32_t wg = blockIdx.x;
  // what k_bin asked of the record pool (final: k_bin has finished) goes to the host through mapped pinned memory; the next
  // render of this set reads it before it launches and grows the pool if a band did not fit.  Only in the latency build
  // (batches copy it on the clear's side stream): with this store compiled into the throughput build — executed by one
  // workgroup, or by none — k_raster took 340 instead of 320 µs for 256 frames
  if constexpr (WAVES > 1)
    if (wg == 0 && wave == 0 && (uint32_t)lane <= a.pool_sub_mask) a.pool_demand[lane * CNT_STRIDE] = a.pool_heads[lane * CNT_STRIDE];
  const uint32_t xcd = wg & 7u, j = wg >> 3;
  const uint32_t tiles_per_frame = a.n_local_bands * a.tiles_x;
  const uint32_t frame = (j / tiles_per_frame) * 8u + xcd, tile = j % tiles_per_frame;
  if (frame >= a.n_frames) return;
  // nothing listed for this tile: nothing to rasterise; its clear (if any) is k_clear's job — or, in a small job that has
  // no k_clear beside it (one kernel boundary less on the latency path), this wave's
  const u32x2 tinfo = as_const(reinterpret_cast<const u32x2 *>(a.tile_info))[(size_t)frame * tiles_per_frame + tile];
  const uint32_t cnt = tinfo.x;
  if (cnt == 0u && !a.clear_in_raster) return; // (three tiles in four of a batch: out after ONE load)
  const SRZ_CAS FrameDesc *fd = as_const(a.frames) + frame;
  const uint32_t flags = fd->flags | a.flags_or;
  if (cnt == 0u) {
    if (flags & SRZ_FUSED_CLEAR) {
      const int W = fd->width;
      const TileRect rc = tile_rect(a, fd, frame, tile / a.tiles_x, tile % a.tiles_x);
      const float inf = __builtin_inff();
      const float4 inf4 = make_float4(inf, inf, inf, inf), zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < ITS; ++k) {
        const int it = wave * ITS + k;
        const int ly = it * 8 + (lane >> 3), x4 = rc.tx0 + (lane & 7) * 4;
        if (rc.ty0 + ly > rc.ty1 || x4 > rc.tx1) continue;
        float *gz = rc.out0 + (size_t)ly * W + x4;
        if (((W & 3) == 0) && x4 + 3 <= rc.tx1) {
          store_nt(gz, inf4), store_nt(gz + rc.plane, zero4), store_nt(gz + 2 * rc.plane, zero4), store_nt(gz + 3 * rc.plane, zero4);
        } else {
          for (int k = 0; k < 4 && x4 + k <= rc.tx1; ++k) gz[k] = inf, gz[rc.plane + k] = 0.f, gz[2 * rc.plane + k] = 0.f, gz[3 * rc.plane + k] = 0.f;
        }
      }
    }
    return;
  }
  const uint32_t off = tinfo.y;
  // the tie-break's payload: the triangle's index, or index << LP_BITS | its position in this tile's list (same order)
  const bool lp_mode = cnt <= LP_MAX && (fd->flags & FD_PACKED) != 0u; // wave-uniform
  const bool lp8 = lp_mode && cnt <= LP8_MAX;                          // (the ids then take 8 bits per pixel)
  const uint32_t idx_mask = (fd->flags & FD_PACKED) ? PACK_IDX_MASK : 0xffffffffu; // (a packed list entry = index | batch << 22)
  if (off == UNLISTED || a.force_ordered || (flags & SRZ_ORDERED_RASTER)) { // the reference's ordered algorithm, from the stream
    if (lane == 0 && wave == 0) a.slow_list[atomicAdd(a.slow_count, 1u)] = frame * tiles_per_frame + tile;
    return;
  }
  const uint32_t lb = tile / a.tiles_x, tx = tile % a.tiles_x;
  const int W = fd->width;
  const TileRect rc = tile_rect(a, fd, frame, lb, tx);
  const bool fused = (flags & SRZ_FUSED_CLEAR) != 0;

  // (the first 64 indices of the tile's list are loaded under the tile init)
  const uint32_t i_first = as_const(a.pool)[off + min((uint32_t)lane, cnt - 1u)] & idx_mask;
  // ---- phase A: tile init (fused clear → +inf, else the in/out z plane) with the incoming-depth tie-break ----------
  if (fused) { // (wave-uniform) straight stores of one constant: nothing here waits for the index load above
    const unsigned long long k_inf = ((unsigned long long)zkey_of(__builtin_inff()) << 32) | TB_NONE;
    unsigned long long *kp = &s_key[((int)threadIdx.x >> 5) * KEY_STRIDE + ((int)threadIdx.x & 31)];
#pragma unroll
    for (int it = 0; it < TILE * TILE / (64 * WAVES); ++it) kp[it * (2 * WAVES * KEY_STRIDE)] = k_inf; // (one address, 16 offsets)
  } else {
    for (int i = (int)threadIdx.x; i < TILE * TILE; i += 64 * WAVES) {
      const int ly = i >> 5, lx = i & 31;
      float z = __builtin_inff();
      if (rc.tx0 + lx <= rc.tx1 && rc.ty0 + ly <= rc.ty1) z = rc.out0[(size_t)ly * W + rc.tx0 + lx];
      const uint32_t zk = (z == z) ? zkey_of(z) : 0u; // a NaN already in the buffer: only the ordered algorithm knows
      s_key[ly * KEY_STRIDE + lx] = ((unsigned long long)zk << 32) | TB_NONE;
    }
  }
  // the pad key of every row is scratch: 64 dword marks, mark r in row r / 2
  // (plain LDS accesses: the mark a triangle writes may be the one this lane reads, so the compiler keeps their order;
  // `volatile` would turn them into flat, system-scope accesses)
  uint32_t *const s_mark = WAVES > 1 ? s_mark_x + wave * 64 : reinterpret_cast<uint32_t *>(s_key);
  auto mark_at = [](uint32_t r) { return WAVES > 1 ? r : ((r >> 1) * (uint32_t)KEY_STRIDE + TILE) * 2u + (r & 1u); };
  const uint32_t my_mark = mark_at((uint32_t)lane);
  s_mark[my_mark] = 0u;
  if (WAVES > 1 && threadIdx.x < 3) s_wg[threadIdx.x] = 0u;
  wg_barrier();

  // ---- phase B: the tile's list, 64 records at a time --------------------------------------------------------------
  // geometry of one record's bbox ∩ tile in TILE-LOCAL coordinates: V columns [x0, v-1] in nseg pieces of 8, S columns [v, x1]
  // An S item is a COLUMN piece: S_ROWS vertically adjacent pixels of one scalar-tail column.  (Rounds 2-5: one pixel per item —
  // 45 instructions of item expansion per pixel test; a triangle's S columns are at most 7 wide but as tall as its box, so pieces
  // run down the column: the x-dependent halves of the three edge functions are shared by the piece's pixels.)
  constexpr uint32_t S_ROWS = 4;
  struct Geo {
    bool ok;
    uint32_t nV, nS, word; // items of the two kinds; packed x0 | y0 << 5 | v << 10 | nseg << 16 | ws << 19 | (rows - 1) << 22
    float zmin;            // nearest vertex depth
  };
  auto geometry = [&](const f32x4 &r0, const f32x4 &r1, const f32x4 &r2, float s_area, bool valid) {
    // r0 = ax ay z0 bx | r1 = by z1 cx cy | r2 = z2 bbx bby -
    const uint32_t bbx = f2u(r2.y), bby = f2u(r2.z);
    const int bsx = (int16_t)(bbx & 0xffff), bsy = (int16_t)(bbx >> 16), bex = (int16_t)(bby & 0xffff), bey = (int16_t)(bby >> 16);
    int x0 = max(bsx, rc.tx0) - rc.tx0, x1 = min(bex, rc.tx1) - rc.tx0, y0 = max(bsy, rc.ty0) - rc.ty0, y1 = min(bey, rc.ty1) - rc.ty0;
    // the rectangle that is walked: bounding box ∩ tile, tightened to the triangle (see tight_margin): the triangle's x-extent
    // inside the rectangle's rows, then its y-extent inside the remaining columns.  About half of the pixel tests of a large
    // triangle and 30 % of a small one's go away (the integer box starts at trunc(min), a column / row before the first pixel
    // centre that can be inside; a large triangle's rectangle in a tile is mostly outside it).
    {
      const float ax = r0.x, ay = r0.y, bx = r0.w, by = r1.x, cx = r1.z, cy = r1.w;
      float m, mn, mx;
      if (tight_margin(ax, ay, bx, by, cx, cy, s_area, bsx, bsy, bex, bey, m)) {
        int X0 = rc.tx0 + x0, X1 = rc.tx0 + x1, Y0 = rc.ty0 + y0, Y1 = rc.ty0 + y1;
        slab_extent(ax, ay, bx, by, cx, cy, (float)Y0 - m, (float)Y1 + m, mn, mx);
        clip_range(X0, X1, mn, mx, m);
        slab_extent(ay, ax, by, bx, cy, cx, (float)X0 - m, (float)X1 + m, mn, mx);
        clip_range(Y0, Y1, mn, mx, m);
        x0 = X0 - rc.tx0, x1 = X1 - rc.tx0, y0 = Y0 - rc.ty0, y1 = Y1 - rc.ty0;
      }
    }
    const int vend = (flags & SRZ_UNIFIED) ? bex + 1 : bsx + ((bex - bsx + 1) & ~7);
    const int v = min(max(vend - rc.tx0, x0), x1 + 1);
    Geo g;
    g.ok = valid && x0 <= x1 && y0 <= y1;
    const uint32_t h = g.ok ? (uint32_t)(y1 - y0 + 1) : 0u, nseg = (uint32_t)(v - x0 + 7) >> 3, ws = (uint32_t)(x1 + 1 - v);
    g.nV = __umul24(h, nseg), g.nS = __umul24((h + S_ROWS - 1u) / S_ROWS, ws); // <= 128 / <= 56 per triangle
    g.word = (uint32_t)x0 | ((uint32_t)y0 << 5) | ((uint32_t)v << 10) | (nseg << 16) | (ws << 19) | (((h - 1u) & 31u) << 22);
    g.zmin = __builtin_fminf(__builtin_fminf(r0.z, r1.y), r2.x);
    return g;
  };
  const SRZ_CAS uint32_t *list = as_const(a.pool) + off; // the tile's triangle indices
  // a list entry's record: the triangle's 9 position floats from the dense stream + its 8-byte bounding box (four independent loads)
  const SRZ_CAS float *tpos = as_const(a.tri_pos) + (size_t)fd->tri_off * a.pos_stride;
  const SRZ_CAS u32x2 *tbox = as_const(reinterpret_cast<const u32x2 *>(a.bbox + fd->tri_off));
  const uint32_t pos_stride = a.pos_stride;
  auto rec_load = [&](uint32_t i, f32x4 &q0, f32x4 &q1, f32x4 &q2) { // q0 = ax ay z0 bx | q1 = by z1 cx cy | q2 = z2 bbx bby -
    const SRZ_CAS float *q = tpos + (size_t)i * pos_stride;
    const F3 v0 = ld3(q), v1 = ld3(q + 3), v2 = ld3(q + 6);
    const u32x2 bb = tbox[i];
    q0 = f32x4{v0.x, v0.y, v0.z, v1.x}, q1 = f32x4{v1.y, v1.z, v2.x, v2.y}, q2 = f32x4{v2.z, u2f_(bb.x), u2f_(bb.y), 0.0f};
  };
  // ---- depth-ordered groups for chunks with heavy overdraw -----------------------------------------------------------
  // The keys make the order of the triangles irrelevant, so a chunk of records that asks for several times the tile's area in
  // pixel tests is rasterised NEAREST FIRST, in 4 groups of equal depth range of the triangles' nearest vertex (the records
  // stay in registers); after each group the tile's farthest depth is read back, and the items of a triangle whose nearest
  // possible depth lies behind it are dropped: they could not win a pixel.  Conservative bounds (positive depths only):
  //   V items: 0 < alpha, beta, gamma < 1 holds for every fragment, so its depth is >= zmin = min(z0,z1,z2) less a few ulps:
  //            bound zmin * (1 - 2^-20)
  //   S items: the inside test is on the edge functions, not on the barycentrics, which may leave [0,1] by their rounding
  //            error <= ~6 * 2^-24 * d^2 / |area2| (d = extent of the vertices, area2 = twice the area).  Only for triangles
  //            with d^2 <= 2^10 |area2| (error < 4e-4): bound zmin - (zmax - zmin) / 256, then * (1 - 2^-20); slivers are
  //            never dropped
  uint32_t zfar = 0xffffffffu; // image of the tile's farthest depth when last read back (all ones: nothing can be dropped yet;
                               // depths only come down, so an old value stays a valid bound)
  // two-deep pipeline: the indices of chunk c + 2 and the records of chunk c + 1 are in flight while chunk c is rasterised
  f32x4 n0, n1, n2;
  bool nv = (uint32_t)lane < cnt;
  uint32_t i_cur = i_first, i_nxt = 64u < cnt ? (list[min(64u + (uint32_t)lane, cnt - 1u)] & idx_mask) : 0u;
  rec_load(i_cur, n0, n1, n2);
  for (uint32_t base = 0; base < cnt; base += 64) {
    const f32x4 r0 = n0, r1 = n1, r2 = n2;
    const uint32_t my_idx = lp_mode ? ((i_cur << LP_BITS) | (base + (uint32_t)lane)) : i_cur; // (the tie-break's payload)
    // the per-triangle constants of the two coverage tests, once per record (not stored anywhere: 8 bytes more per triangle to write and to gather)
    float rec_v_inv, rec_s_area;
    {
      TriXY k;
      k.ax = r0.x, k.ay = r0.y, k.bx = r0.w, k.by = r1.x, k.cx = r1.z, k.cy = r1.w;
      BranchMath bm;
      tri_consts(bm, k);
      rec_v_inv = k.v_inv, rec_s_area = k.s_area;
    }
    const bool valid = nv;
    nv = base + 64 + lane < cnt;
    if (base + 64 < cnt) {
      i_cur = i_nxt;
      rec_load(i_cur, n0, n1, n2);
      if (base + 128 < cnt) i_nxt = list[min(base + 128u + (uint32_t)lane, cnt - 1u)] & idx_mask;
    }
    const Geo G = geometry(r0, r1, r2, rec_s_area, valid);
    const uint32_t geom = G.word;
    uint32_t group = 0, n_groups = 1, znear = 0, znear_s = 0; // nearest possible depth of a V / S fragment, as keys (0: unknown → kept)
    if ((uint32_t)rl_i((int)wave_scan_add(8u * G.nV + S_ROWS * G.nS), 63) > 4u * TILE * TILE) { // > 4 pixel tests per pixel of the tile
      float lo = G.ok ? G.zmin : __builtin_inff(), hi = G.ok ? G.zmin : -__builtin_inff();
      for (int o = 32; o > 0; o >>= 1) lo = __builtin_fminf(lo, __shfl_xor(lo, o)), hi = __builtin_fmaxf(hi, __shfl_xor(hi, o));
      if (hi > lo && hi < __builtin_inff() && lo > -__builtin_inff()) {
        n_groups = 4;
        const float g = (G.zmin - lo) * (4.0f / (hi - lo)); // (a NaN depth → group 0)
        group = (g > 0.0f && g < 4.0f) ? (uint32_t)g : (g >= 4.0f ? 3u : 0u);
      }
    }
    if (n_groups > 1 || zfar != 0xffffffffu) {
      if (G.zmin > 0.0f) znear = zkey_of(G.zmin * 0.99999905f);
      const float zmax = __builtin_fmaxf(__builtin_fmaxf(r0.z, r1.y), r2.x);
      const float dx = __builtin_fmaxf(__builtin_fmaxf(r0.x, r0.w), r1.z) - __builtin_fminf(__builtin_fminf(r0.x, r0.w), r1.z);
      const float dy = __builtin_fmaxf(__builtin_fmaxf(r0.y, r1.x), r1.w) - __builtin_fminf(__builtin_fminf(r0.y, r1.x), r1.w);
      const float zs = (G.zmin - (zmax - G.zmin) * 0.00390625f) * 0.99999905f;
      if (dx * dx + dy * dy <= 1024.0f * __builtin_fabsf(rec_s_area) && zmax < 1e30f && zs > 0.0f) znear_s = zkey_of(zs);
    }
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
    const bool mine = G.ok && group == gi;
    const uint32_t nV = (mine && znear <= zfar) ? G.nV : 0u, nS = (mine && znear_s <= zfar) ? G.nS : 0u;
    const uint32_t packed = nV | (nS << 16), incl = wave_scan_add(packed);
    const uint32_t offs = incl - packed; // exclusive: first V item | first S item << 16
    const uint32_t tot = (uint32_t)rl_i((int)incl, 63), TV = tot & 0xffffu, TS = tot >> 16;

    // ---- V items: 8 pixels of one row each (barycentric(__m256) + inside mask + z, src/Rasterizer.cpp:89-127,310-334)
    uint32_t carry = 0;
    for (uint32_t P0 = 64u * (uint32_t)wave; P0 < TV; P0 += 64u * WAVES) {
      if constexpr (WAVES > 1) { // (this wave did not run the batch before: the triangle that reaches into this one is the last to start before it)
        const unsigned long long before = __ballot(nV != 0u && (offs & 0xffffu) < P0);
        carry = before ? 64u - (uint32_t)__builtin_clzll(before) : 0u;
      }
      const uint32_t r = (offs & 0xffffu) - P0;
      if (nV != 0u && r < 64u) s_mark[mark_at(r)] = (uint32_t)lane + 1u;
      __builtin_amdgcn_wave_barrier();
      uint32_t m = s_mark[my_mark];
      __builtin_amdgcn_wave_barrier();
      s_mark[my_mark] = 0u;
      m = max(wave_scan_max(m), carry);
      carry = (uint32_t)rl_i((int)m, 63);
      const int src = (int)((m - 1u) & 63u) * 4;
      const float ax = bperm_f(src, r0.x), ay = bperm_f(src, r0.y), z0 = bperm_f(src, r0.z), bx = bperm_f(src, r0.w);
      const float by = bperm_f(src, r1.x), z1 = bperm_f(src, r1.y), cx = bperm_f(src, r1.z), cy = bperm_f(src, r1.w);
      const float z2 = bperm_f(src, r2.x), v_inv = bperm_f(src, rec_v_inv);
      const uint32_t g = bperm_u(src, geom), idx = bperm_u(src, my_idx), o = bperm_u(src, offs);
      const uint32_t item = P0 + (uint32_t)lane, i = item - (o & 0xffffu), ns = (g >> 16) & 7u;
      // row = i / ns: (i + 0.5) / ns is at least 1 / 8 away from every integer, far more than the error of v_rcp
      const uint32_t row = (uint32_t)(((float)i + 0.5f) * __builtin_amdgcn_rcpf((float)ns)), seg = i - __umul24(row, ns);
      const uint32_t yl = ((g >> 5) & 31u) + row, xs = (g & 31u) + 8u * seg;
      const int lim = item < TV ? (int)((g >> 10) & 63u) - (int)xs : 0; // pixels of this piece inside the V columns
      const float fy = (float)(rc.ty0 + (int)yl), fx0 = (float)(rc.tx0 + (int)xs);
      const float PBy = by - fy, PCy = cy - fy, PAy = ay - fy;
      unsigned long long *kp = s_key + ((yl << 5) + yl) + xs; // yl * KEY_STRIDE
      const uint32_t tb = 0x80000000u | idx;
      // all the arithmetic of the 8 independent pixels first, then the predicated LDS atomics
      uint32_t zk[8];
      bool inside[8];
#pragma unroll
      for (int px = 0; px < 8; ++px) {
        const float fx = fx0 + (float)px; // (exact)
        const float PBx = bx - fx, PCx = cx - fx, PAx = ax - fx;
        const float aPBC = fmsubf(PBx, PCy, PCx * PBy), aPCA = fmsubf(PCx, PAy, PAx * PCy);
        const float al = aPBC * v_inv, be = aPCA * v_inv, ga = 1.0f - (al + be);
        const float z = fmaf_(al, z0, fmaf_(be, z1, ga * z2));
        // 0<al<1 & 0<be<1 & 0<ga<1  <=>  al>0 & be>0 & ga>0 & ga<1 (al+be is rounded monotonically, so ga>0 forces
        // al,be <= al+be < 1); every compare is ordered, so NaNs reject exactly like _CMP_*_OQ
        // (a NaN alpha or beta makes gamma NaN, which fails gamma < 1: the three-way minimum may drop NaNs)
        inside[px] = (px < lim) & (__builtin_fminf(__builtin_fminf(al, be), ga) > 0.0f) & (ga < 1.0f);
        // (an inside fragment's depth is a sum of finite terms of bounded weights: ±inf on overflow at worst, never NaN)
        zk[px] = zkey_of(z);
        asm volatile("" : "+v"(zk[px])); // (keeps the depth arithmetic out of the predicated blocks: 8 pixels of straight-line code)
      }
#pragma unroll
      for (int px = 0; px < 8; ++px)
        if (inside[px])
          __hip_atomic_fetch_min(kp + px, ((unsigned long long)zk[px] << 32) | tb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // ---- S items: S_ROWS pixels of one column each (insideTriangle + barycentric(scalar) + z, src/Rasterizer.cpp:11-70,465-477)
    carry = 0;
    for (uint32_t P0 = 64u * (uint32_t)wave; P0 < TS; P0 += 64u * WAVES) {
      if constexpr (WAVES > 1) {
        const unsigned long long before = __ballot(nS != 0u && (offs >> 16) < P0);
        carry = before ? 64u - (uint32_t)__builtin_clzll(before) : 0u;
      }
      const uint32_t r = (offs >> 16) - P0;
      if (nS != 0u && r < 64u) s_mark[mark_at(r)] = (uint32_t)lane + 1u;
      __builtin_amdgcn_wave_barrier();
      uint32_t m = s_mark[my_mark];
      __builtin_amdgcn_wave_barrier();
      s_mark[my_mark] = 0u;
      m = max(wave_scan_max(m), carry);
      carry = (uint32_t)rl_i((int)m, 63);
      const int src = (int)((m - 1u) & 63u) * 4;
      const float ax = bperm_f(src, r0.x), ay = bperm_f(src, r0.y), z0 = bperm_f(src, r0.z), bx = bperm_f(src, r0.w);
      const float by = bperm_f(src, r1.x), z1 = bperm_f(src, r1.y), cx = bperm_f(src, r1.z), cy = bperm_f(src, r1.w);
      const float z2 = bperm_f(src, r2.x), s_area = bperm_f(src, rec_s_area);
      const uint32_t g = bperm_u(src, geom), idx = bperm_u(src, my_idx), o = bperm_u(src, offs);
      const uint32_t item = P0 + (uint32_t)lane, i = item - (o >> 16), w = (g >> 19) & 7u;
      const uint32_t piece = (uint32_t)(((float)i + 0.5f) * __builtin_amdgcn_rcpf((float)w)), col = i - __umul24(piece, w);
      const uint32_t yl0 = ((g >> 5) & 31u) + S_ROWS * piece, xl = ((g >> 10) & 63u) + col;
      const int lim = item < TS ? (int)((g >> 22) & 31u) + 1 - (int)(S_ROWS * piece) : 0; // rows of this piece inside the rectangle
      const float fy0 = (float)(rc.ty0 + (int)yl0), fx = (float)(rc.tx0 + (int)xl);
      // the reference's expressions per pixel; what depends on x alone is the same for the piece's pixels.  P?x = ?x - fx is the exact
      // negative of ?Px = fx - ?x, and a product of two negated factors is the product: aPBC = PBx * PCy - PBy * PCx = BPx * CPy - BPy * CPx
      const float ABx = bx - ax, ABy = by - ay, BCx = cx - bx, BCy = cy - by, CAx = ax - cx, CAy = ay - cy;
      const float APx = fx - ax, BPx = fx - bx, CPx = fx - cx;
      const float t0 = ABy * APx, t1 = BCy * BPx, t2 = CAy * CPx;
      unsigned long long *kp = s_key + ((yl0 << 5) + yl0) + xl; // yl0 * KEY_STRIDE; the next row is KEY_STRIDE keys further
      const uint32_t tb = 0x7ffffffeu - idx;
      uint32_t zk[S_ROWS];
      bool hit[S_ROWS];
#pragma unroll
      for (int k = 0; k < (int)S_ROWS; ++k) {
        const float fy = fy0 + (float)k; // (exact)
        const float APy = fy - ay, BPy = fy - by, CPy = fy - cy;
        const float e0 = ABx * APy - t0, e1 = BCx * BPy - t1, e2 = CAx * CPy - t2;
        const bool in_tri = ((e0 > 0) & (e1 > 0) & (e2 > 0)) | ((e0 < 0) & (e1 < 0) & (e2 < 0));
        const float aPBC = BPx * CPy - BPy * CPx, aPCA = CPx * APy - CPy * APx;
        const float al = aPBC / s_area, be = aPCA / s_area, ga = 1.0f - al - be;
        const float z = al * z0 + be * z1 + ga * z2;
        hit[k] = (k < lim) & in_tri; // '<=' passes and so does a NaN depth (src/Rasterizer.cpp:475): key 0 = "ask the ordered rasteriser"
        zk[k] = (z == z) ? zkey_of(z) : 0u;
        asm volatile("" : "+v"(zk[k])); // (as in the V loop: the arithmetic of the piece's pixels is one straight line)
      }
#pragma unroll
      for (int k = 0; k < (int)S_ROWS; ++k)
        if (hit[k])
          __hip_atomic_fetch_min(kp + k * KEY_STRIDE, ((unsigned long long)zk[k] << 32) | tb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // the tile's farthest depth after this group (pixels outside the frame keep +inf: no dropping there); also between the
    // chunks of a long list once dropping has started paying
    if (gi + 1 < n_groups || (n_groups > 1 && base + 64 < cnt)) {
      wg_barrier(); // (every wave's minima of this group are in the keys)
      uint32_t zm = 0;
#pragma unroll
      for (int it = 0; it < 16; ++it) zm = max(zm, (uint32_t)(s_key[(it * 2 + (lane >> 5)) * KEY_STRIDE + (lane & 31)] >> 32));
      for (int o = 32; o > 0; o >>= 1) zm = max(zm, (uint32_t)__shfl_xor((int)zm, o));
      zfar = zm;
      // (the waves must agree on the bound: it decides the item counts, hence which items a batch holds — no wave may lower a
      // key before all have read them)
      wg_barrier();
    }
    } // groups
  } // chunks
  wg_barrier();

  // ---- phase C: decode the keys, write out ------------------------------------------------------------------------
  //  some final key needs the ordered algorithm  : the tile goes to k_raster_slow, nothing is written here
  //  nobody owns the tile: fused → the clear itself (z=+inf, colour 0), else the framebuffer is left untouched
  //  owned tile          : z plane + owner ids, and the tile is queued for k_shade (which writes the 3 colour planes)
  float4 z4[ITS];
  uint4 id4[ITS];
  bool any_owner = false, redo = false;
#pragma unroll
  for (int it = 0; it < ITS; ++it) {
    const int ly = (wave * ITS + it) * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
    const unsigned long long *kr = &s_key[ly * KEY_STRIDE + lx4]; // (rows are 264 bytes apart: 8-byte aligned reads)
    const unsigned long long k0 = kr[0], k1 = kr[1], k2 = kr[2], k3 = kr[3];
    const uint32_t tb[4] = {(uint32_t)k0, (uint32_t)k1, (uint32_t)k2, (uint32_t)k3};
    const uint32_t zk[4] = {(uint32_t)(k0 >> 32), (uint32_t)(k1 >> 32), (uint32_t)(k2 >> 32), (uint32_t)(k3 >> 32)};
    float zz[4];
    uint32_t id[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      redo |= (zk[k] == 0u) | ((zk[k] + 0x80000001u) <= 1u); // NaN that passed / final depth ±0
      zz[k] = z_of_key(zk[k]);
      // (the payload of the tie-break: the triangle's index, or — lp_mode — index << LP_BITS | list position: the ids keep
      // either all of it or its position bits, id_pack16)
      id[k] = (tb[k] & 0x80000000u) ? (tb[k] & 0x7fffffffu) : (tb[k] == TB_NONE ? NO_TRI : ((0x7ffffffeu - tb[k]) | S_CLASS_BIT));
      any_owner |= tb[k] != TB_NONE;
    }
    z4[it] = make_float4(zz[0], zz[1], zz[2], zz[3]);
    id4[it] = make_uint4(id[0], id[1], id[2], id[3]);
  }
  bool tile_redo = __ballot(redo) != 0ull, tile_has_owner = __ballot(any_owner) != 0ull; // wave-uniform
  if constexpr (WAVES > 1) { // tile-wide: through LDS
    if (lane == 0 && tile_redo) s_wg[0] = 1u;
    if (lane == 0 && tile_has_owner) s_wg[1] = 1u;
    __syncthreads();
    tile_redo = s_wg[0] != 0u, tile_has_owner = s_wg[1] != 0u;
  }
  if (tile_redo) {
    if (lane == 0 && wave == 0) a.slow_list[atomicAdd(a.slow_count, 1u)] = frame * tiles_per_frame + tile;
    return;
  }
  const bool vec_ok = (W & 3) == 0;
  if (tile_has_owner || fused) {
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t *slot = a.vis + ((size_t)frame * tiles_per_frame + tile) * PIX_SLOT;
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
      const int ly = (wave * ITS + it) * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
      const int y = rc.ty0 + ly, x4 = rc.tx0 + lx4;
      // the owners of ALL of the tile's pixels (those beyond the frame's edge have none: their keys never got a fragment);
      // re-read by k_shade: cacheable
      if (tile_has_owner) ids_store4(slot, (uint32_t)(ly * TILE + lx4), id4[it], lp_mode, lp8);
      if (y > rc.ty1 || x4 > rc.tx1) continue;
      float *gz = rc.out0 + (size_t)ly * W + x4;
      const bool full = vec_ok && x4 + 3 <= rc.tx1;
      if (tile_has_owner)
        quad_store(gz, rc.plane, {z4[it]}, full, x4, rc.tx1); // final: k_shade recomputes the depth it needs from the owner triangle
      else // touched by a bbox but owned by nobody: the clear itself
        quad_store(gz, rc.plane, {z4[it], zero4, zero4, zero4}, full, x4, rc.tx1);
    }
  }
  // owned tile → the frame's own work list (a counter per frame: one shared counter serialises ~10 ns per tile)
  if (tile_has_owner && lane == 0 && wave == 0)
    work_append(a, fd->flags, frame * tiles_per_frame + tile, work_entry(frame, lb, tx, lp_mode, lp8, cnt, off));
}

// ================================================================================================================
// k_raster_slow — the reference's ORDERED algorithm for the tiles k_raster could not finish: tiles whose band did not
// fit the record pool, tiles where a NaN or ±0 depth decides a pixel, and every touched tile of a counting run or under
// SRZ_ORDERED_RASTER.  One wave per tile (persistent grid over the list); the wave walks the FRAME's triangles in
// submission order (64 bboxes at a time, chunks whose rows miss the tile are skipped), broadcasts one hit triangle at a
// time into SGPRs and sweeps bbox ∩ tile in 64-pixel blocks against z + owner planes in LDS: a wave's LDS operations are
// ordered, so "last writer in submission order wins" needs no lock.
// ================================================================================================================
template <bool STATS>
__global__ __launch_bounds__(64) void k_raster_slow(RenderArgs a) {
  __shared__ __attribute__((aligned(16))) float zl[TILE * LDS_STRIDE];
  __shared__ __attribute__((aligned(16))) uint32_t il[TILE * LDS_STRIDE];
  const int lane = threadIdx.x & 63;
  const uint32_t tiles_per_frame = a.n_local_bands * a.tiles_x;
  const uint32_t n_slow = *as_const(a.slow_count);
  unsigned long long n_frag = 0, n_shaded = 0;
  for (uint32_t e = blockIdx.x; e < n_slow; e += gridDim.x) {
    const uint32_t entry = as_const(a.slow_list)[e];
    const uint32_t frame = entry / tiles_per_frame, tile = entry % tiles_per_frame;
    const SRZ_CAS FrameDesc *fd = as_const(a.frames) + frame;
    const uint32_t lb = tile / a.tiles_x, tx = tile % a.tiles_x;
    const int W = fd->width;
    const uint32_t n_tris = fd->n_tris;
    const uint32_t flags = fd->flags | a.flags_or;
    const TileRect rc = tile_rect(a, fd, frame, lb, tx);
    const bool fused = (flags & SRZ_FUSED_CLEAR) != 0;
    // ---- phase A: tile init (fused clear → +inf, else load the in/out z plane) -------------------------------
    for (int i = lane; i < TILE * TILE; i += 64) {
      const int ly = i >> 5, lx = i & 31;
      float z = __builtin_inff();
      if (!fused && rc.tx0 + lx <= rc.tx1 && rc.ty0 + ly <= rc.ty1) z = rc.out0[(size_t)ly * W + rc.tx0 + lx];
      zl[ly * LDS_STRIDE + lx] = z;
      il[ly * LDS_STRIDE + lx] = NO_TRI;
    }
    __builtin_amdgcn_wave_barrier();
    // ---- phase B: the frame's triangles in submission order ------------------------------------------------------
    const SRZ_CAS u32x2 *bbox = as_const(reinterpret_cast<const u32x2 *>(a.bbox + fd->tri_off));
    const SRZ_CAS float *tpos = as_const(a.tri_pos) + (size_t)fd->tri_off * a.pos_stride;
    const SRZ_CAS uint32_t *chunk_rows = as_const(a.chunk_rows) + fd->chunk_off;
    const uint32_t n_chunks = (n_tris + 63) / 64;
    for (uint32_t c = 0; c < n_chunks; ++c) {
      const uint32_t cr = chunk_rows[c]; // wave-uniform
      if ((int)(int16_t)(cr & 0xffffu) > rc.ty1 || (int)(int16_t)(cr >> 16) < rc.ty0) continue;
      const uint32_t my = c * 64u + (uint32_t)lane;
      const u32x2 bb = bbox[min(my, n_tris - 1u)];
      const int bsx = (int16_t)(bb.x & 0xffff), bsy = (int16_t)(bb.x >> 16), bex = (int16_t)(bb.y & 0xffff), bey = (int16_t)(bb.y >> 16);
      const bool hit = my < n_tris && bsx <= bex && bex >= rc.tx0 && bsx <= rc.tx1 && bey >= rc.ty0 && bsy <= rc.ty1;
      unsigned long long m = __ballot(hit);
      if (m == 0ull) continue;
      TriXY t;
      t.ax = t.ay = t.bx = t.by = t.cx = t.cy = t.z0 = t.z1 = t.z2 = t.v_inv = t.s_area = 0.0f;
      // Per-lane (= per-triangle) geometry of bbox ∩ tile in TILE-LOCAL coordinates, packed into one word:
      //   [4:0] x0  [9:5] x1  [14:10] y0  [19:15] y1  [25:20] v = first scalar-tail column (V part = [x0,v-1], S = [v,x1])
      //   [27:26] log2(block width) of the V sweep  [29:28] of the S sweep   (block = BW x 64/BW pixels: 8x8, 16x4, 4x16,
      //   whichever needs the fewest blocks)
      uint32_t geom = 0;
      if (hit) {
        float p[9];
        load_pos9(tpos + (size_t)my * a.pos_stride, p);
        t.ax = p[0], t.ay = p[1], t.z0 = p[2], t.bx = p[3], t.by = p[4], t.z1 = p[5], t.cx = p[6], t.cy = p[7], t.z2 = p[8];
        BranchMath bm;
        tri_consts(bm, t);
        const int x0 = max(bsx, rc.tx0) - rc.tx0, x1 = min(bex, rc.tx1) - rc.tx0, y0 = max(bsy, rc.ty0) - rc.ty0, y1 = min(bey, rc.ty1) - rc.ty0;
        const int vend = (flags & SRZ_UNIFIED) ? bex + 1 : bsx + ((bex - bsx + 1) & ~7);
        const int v = min(max(vend - rc.tx0, x0), x1 + 1);
        const int h = y1 - y0 + 1, wv = v - x0, ws = x1 + 1 - v;
        auto pick = [h](int w) {
          const int n88 = ((w + 7) >> 3) * ((h + 7) >> 3), n164 = ((w + 15) >> 4) * ((h + 3) >> 2), n416 = ((w + 3) >> 2) * ((h + 15) >> 4);
          int l = 3;
          if (n164 < n88 && n164 <= n416) l = 4;
          if (n416 < n88 && n416 < n164) l = 2;
          return l;
        };
        geom = (uint32_t)x0 | ((uint32_t)x1 << 5) | ((uint32_t)y0 << 10) | ((uint32_t)y1 << 15) | ((uint32_t)v << 20) |
               ((uint32_t)(pick(wv) - 2) << 26) | ((uint32_t)(pick(ws) - 2) << 28);
      }
      while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        // broadcast triangle j to the wave (uniform values → SGPRs)
        TriXY u;
        u.ax = rl_f(t.ax, j), u.ay = rl_f(t.ay, j), u.bx = rl_f(t.bx, j), u.by = rl_f(t.by, j), u.cx = rl_f(t.cx, j);
        u.cy = rl_f(t.cy, j), u.z0 = rl_f(t.z0, j), u.z1 = rl_f(t.z1, j), u.z2 = rl_f(t.z2, j);
        u.v_inv = rl_f(t.v_inv, j), u.s_area = rl_f(t.s_area, j);
        const uint32_t idx = c * 64u + (uint32_t)j;
        const uint32_t g = (uint32_t)rl_i((int)geom, j);
        const int x0 = g & 31, x1 = (g >> 5) & 31, y0 = (g >> 10) & 31, y1 = (g >> 15) & 31, vx = (g >> 20) & 63;
        if (y1 < y0) continue; // (cannot happen for a hit; keeps the loops well-formed)
        if (vx > x0) { // ---- "V" sweep over columns [x0, vx-1] -------------------------------------------------
          const int lbw = (int)((g >> 26) & 3) + 2, bw = 1 << lbw, bh = 64 >> lbw;
          const int lx = lane & (bw - 1), ly = lane >> lbw;
          for (int yb = y0; yb <= y1; yb += bh) {
            const int yl = yb + ly;
            const float fy = (float)(rc.ty0 + yl);
            const float PBy = u.by - fy, PCy = u.cy - fy, PAy = u.ay - fy;
            const bool rowok = yl <= y1;
            for (int xb = x0; xb < vx; xb += bw) {
              const int xl = xb + lx;
              const float fx = (float)(rc.tx0 + xl);
              const float PBx = u.bx - fx, PCx = u.cx - fx, PAx = u.ax - fx;
              const float aPBC = fmsubf(PBx, PCy, PCx * PBy), aPCA = fmsubf(PCx, PAy, PAx * PCy);
              const float al = aPBC * u.v_inv, be = aPCA * u.v_inv, ga = 1.0f - (al + be);
              const float z = fmaf_(al, u.z0, fmaf_(be, u.z1, ga * u.z2));
              const int li = min(yl * LDS_STRIDE + xl, TILE * LDS_STRIDE - 1); // clamped: idle lanes read a valid word
              const float zold = zl[li];
              const bool inside = rowok & (xl < vx) & (al > 0.0f) & (be > 0.0f) & (ga > 0.0f) & (ga < 1.0f);
              const bool pass = inside & (z < zold); // strict (src/Rasterizer.cpp:334)
              if (pass) {
                zl[li] = z;
                il[li] = idx;
              }
              if (STATS) n_frag += inside ? 1 : 0, n_shaded += pass ? 1 : 0;
            }
          }
        }
        if (vx <= x1) { // ---- scalar-tail "S" sweep over columns [vx, x1] (<= 7 wide) -----------------------------
          const int lbw = (int)((g >> 28) & 3) + 2, bw = 1 << lbw, bh = 64 >> lbw;
          const int lx = lane & (bw - 1), ly = lane >> lbw;
          const float ABx = u.bx - u.ax, ABy = u.by - u.ay, BCx = u.cx - u.bx, BCy = u.cy - u.by, CAx = u.ax - u.cx,
                      CAy = u.ay - u.cy;
          for (int yb = y0; yb <= y1; yb += bh) {
            const int yl = yb + ly;
            const float fy = (float)(rc.ty0 + yl);
            const bool rowok = yl <= y1;
            for (int xb = vx; xb <= x1; xb += bw) {
              const int xl = xb + lx;
              const float fx = (float)(rc.tx0 + xl);
              // insideTriangle (src/Rasterizer.cpp:11-41)
              const float APx = fx - u.ax, APy = fy - u.ay, BPx = fx - u.bx, BPy = fy - u.by, CPx = fx - u.cx, CPy = fy - u.cy;
              const float e0 = ABx * APy - ABy * APx, e1 = BCx * BPy - BCy * BPx, e2 = CAx * CPy - CAy * CPx;
              const bool in_tri = ((e0 > 0) & (e1 > 0) & (e2 > 0)) | ((e0 < 0) & (e1 < 0) & (e2 < 0));
              // barycentric (scalar) + z (src/Rasterizer.cpp:43-70,473)
              const float PAx = u.ax - fx, PAy = u.ay - fy, PBx = u.bx - fx, PBy = u.by - fy, PCx = u.cx - fx, PCy = u.cy - fy;
              const float aPBC = PBx * PCy - PBy * PCx, aPCA = PCx * PAy - PCy * PAx;
              const float al = aPBC / u.s_area, be = aPCA / u.s_area, ga = 1.0f - al - be;
              const float z = al * u.z0 + be * u.z1 + ga * u.z2;
              const int li = min(yl * LDS_STRIDE + xl, TILE * LDS_STRIDE - 1);
              const float zold = zl[li];
              const bool inside = rowok & (xl <= x1) & in_tri;
              const bool pass = inside & !(z > zold); // <= passes, NaN passes (src/Rasterizer.cpp:475)
              if (pass) {
                zl[li] = z;
                il[li] = idx | S_CLASS_BIT;
              }
              if (STATS) n_frag += inside ? 1 : 0, n_shaded += pass ? 1 : 0;
            }
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    bool any_owner = false;
    for (int it = 0; it < 4; ++it) {
      const uint4 q = *reinterpret_cast<const uint4 *>(&il[(it * 8 + (lane >> 3)) * LDS_STRIDE + (lane & 7) * 4]);
      any_owner |= (q.x & q.y & q.z & q.w) != NO_TRI;
    }
    const bool tile_has_owner = __ballot(any_owner) != 0ull; // wave-uniform
    // ---- phase C: write-out (as k_raster) ---------------------------------------------------------------------------
    const bool vec_ok = (W & 3) == 0;
    if (tile_has_owner || fused) {
      const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int it = 0; it < 4; ++it) {
        const int ly = it * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
        const int y = rc.ty0 + ly, x4 = rc.tx0 + lx4;
        if (y > rc.ty1 || x4 > rc.tx1) continue;
        const float4 z4 = *reinterpret_cast<const float4 *>(&zl[ly * LDS_STRIDE + lx4]);
        float *gz = rc.out0 + (size_t)ly * W + x4;
        const bool full = vec_ok && x4 + 3 <= rc.tx1;
        if (tile_has_owner)
          quad_store(gz, rc.plane, {z4}, full, x4, rc.tx1);
        else
          quad_store(gz, rc.plane, {z4, zero4, zero4, zero4}, full, x4, rc.tx1);
      }
    }
    if (tile_has_owner) { // the owners of all of the tile's pixels, by index (32 bits each), and the tile's work entry
      uint32_t *slot = a.vis + (size_t)entry * PIX_SLOT;
      for (int it = 0; it < 4; ++it) {
        const int ly = it * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
        ids_store4(slot, (uint32_t)(ly * TILE + lx4), *reinterpret_cast<const uint4 *>(&il[ly * LDS_STRIDE + lx4]), false, false);
      }
      if (lane == 0) work_append(a, fd->flags, entry, work_entry(frame, lb, tx, false, false, 0u, 0u));
    }
    __builtin_amdgcn_wave_barrier(); // the planes are reused by this wave's next tile
  }
  if (STATS) {
    for (int o = 32; o > 0; o >>= 1) n_frag += __shfl_down(n_frag, o), n_shaded += __shfl_down(n_shaded, o);
    if (lane == 0) {
      if (n_frag) atomicAdd(&a.stats[ST_FRAGMENTS], n_frag);
      if (n_shaded) atomicAdd(&a.stats[ST_SHADED], n_shaded);
    }
  }
}

// ================================================================================================================
// k_peel — DEPTH PEELING (srz_frameset_peel_visibility, the rule: include/srz.h): layer k + 1 of a visibility buffer
// from layer k (`prev`, this render's frames as `a.out` has them).  It takes k_raster's place in a render: one wave per tile with
// k_raster<1>'s XCD-aware tile assignment and early-outs; k_visibility behind it writes id / alpha / beta as for any layer 1.
// Per pixel the fragments are totally ordered by (z as a float, tie-break) with k_raster's tie-breaks — 0x7ffffffe - idx (S, the
// later the smaller) < 0x80000000 | idx (V, the earlier the smaller): "last S at that depth, else first V" — and the output is the
// smallest fragment strictly above prev's.  The tile holds prev's (z, tie-break) and the best candidate's in four LDS planes (16 KB:
// ten waves per CU); an ENDED pixel (id 0 or out of range, NaN depth, beyond the frame's edge) holds (+inf, PEEL_NOBODY), above
// which nothing lies.  The order does not depend on the sequence of the fragments, so a listed tile feeds the sweep from its list
// in the pool (64 entries per load, as k_raster) and a tile of an UNLISTED band from the frame's stream (chunk_rows and the
// bounding boxes, as k_raster_slow: counted in slow_count[0]).  A wave's LDS operations are ordered: no atomics.  prev is compared,
// never used as an index.  The render is always a fused-clear one (the host ors the flag in).
// (inline copies, each names its definition: the cleared tile of k_raster; the per-lane geometry, the broadcast, the V and S
// sweeps and the write-out of k_raster_slow — as helpers they would have to leave k_raster_slow's registers as they are)
// ================================================================================================================
constexpr uint32_t PEEL_NOBODY = 0xffffffffu; // the tie-break of no fragment: above every fragment's
__global__ __launch_bounds__(64) void k_peel(RenderArgs a, const float *prev) {
  __shared__ __attribute__((aligned(16))) float s_zp[TILE * LDS_STRIDE], s_bz[TILE * LDS_STRIDE];
  __shared__ __attribute__((aligned(16))) uint32_t s_tp[TILE * LDS_STRIDE], s_bt[TILE * LDS_STRIDE];
  const int lane = threadIdx.x & 63;
  // (k_raster's XCD-aware tile assignment)
  const uint32_t wg = blockIdx.x;
  const uint32_t xcd = wg & 7u, j0 = wg >> 3;
  const uint32_t tiles_per_frame = a.n_local_bands * a.tiles_x;
  const uint32_t frame = (j0 / tiles_per_frame) * 8u + xcd, tile = j0 % tiles_per_frame;
  if (frame >= a.n_frames) return;
  const u32x2 tinfo = as_const(reinterpret_cast<const u32x2 *>(a.tile_info))[(size_t)frame * tiles_per_frame + tile];
  const uint32_t cnt = tinfo.x;
  if (cnt == 0u && !a.clear_in_raster) return; // (k_clear's tile)
  const SRZ_CAS FrameDesc *fd = as_const(a.frames) + frame;
  const uint32_t flags = fd->flags | a.flags_or;
  const uint32_t lb = tile / a.tiles_x, tx = tile % a.tiles_x;
  const int W = fd->width;
  const uint32_t n_tris = fd->n_tris;
  const TileRect rc = tile_rect(a, fd, frame, lb, tx);
  const bool vec_ok = (W & 3) == 0;
  const float inf = __builtin_inff();
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (cnt == 0u) { // nothing listed: the clear itself (k_raster's cnt == 0 branch)
    const float4 inf4 = make_float4(inf, inf, inf, inf);
    for (int it = 0; it < 4; ++it) {
      const int ly = it * 8 + (lane >> 3), x4 = rc.tx0 + (lane & 7) * 4;
      if (rc.ty0 + ly > rc.ty1 || x4 > rc.tx1) continue;
      quad_store(rc.out0 + (size_t)ly * W + x4, rc.plane, {inf4, zero4, zero4, zero4}, vec_ok && x4 + 3 <= rc.tx1, x4, rc.tx1);
    }
    return;
  }
  const uint32_t off = tinfo.y;
  const bool listed = off != UNLISTED; // wave-uniform
  const uint32_t idx_mask = (fd->flags & FD_PACKED) ? PACK_IDX_MASK : 0xffffffffu; // (a packed list entry = index | batch << 22)
  if (!listed && lane == 0) atomicAdd(a.slow_count, 1u);
  // ---- init: prev's (z, tie-break) per pixel, best = nobody ----------------------------------------------------------------
  const float *pz = prev + (rc.out0 - a.out); // (plane 0 of prev at row ty0: the two buffers share one layout)
  for (int i = lane; i < TILE * TILE; i += 64) {
    const int ly = i >> 5, lx = i & 31;
    float zp = inf;
    uint32_t tp = PEEL_NOBODY;
    if (rc.tx0 + lx <= rc.tx1 && rc.ty0 + ly <= rc.ty1) {
      const size_t o = (size_t)ly * W + rc.tx0 + lx;
      const float z = pz[o];
      const uint32_t id = f2u(pz[rc.plane + o]);
      const uint32_t wp = (id & 0x7fffffffu) - 1u; // (id 0, or only the class bit: 0xffffffff, out of range)
      if (id != 0u && wp < n_tris && z == z) zp = z, tp = (id & S_CLASS_BIT) ? 0x7ffffffeu - wp : (0x80000000u | wp);
    }
    s_zp[ly * LDS_STRIDE + lx] = zp, s_tp[ly * LDS_STRIDE + lx] = tp;
    s_bz[ly * LDS_STRIDE + lx] = inf, s_bt[ly * LDS_STRIDE + lx] = PEEL_NOBODY;
  }
  __builtin_amdgcn_wave_barrier();
  // ---- feed: 64 triangles per round, from the tile's list or from the frame's stream -----------------------------------------
  const SRZ_CAS u32x2 *bbox = as_const(reinterpret_cast<const u32x2 *>(a.bbox + fd->tri_off));
  const SRZ_CAS float *tpos = as_const(a.tri_pos) + (size_t)fd->tri_off * a.pos_stride;
  const SRZ_CAS uint32_t *chunk_rows = as_const(a.chunk_rows) + fd->chunk_off;
  const uint32_t n_rounds = ((listed ? cnt : n_tris) + 63u) / 64u;
  for (uint32_t c = 0; c < n_rounds; ++c) {
    uint32_t my;
    bool valid;
    if (listed) {
      const uint32_t e = c * 64u + (uint32_t)lane;
      my = as_const(a.pool)[off + min(e, cnt - 1u)] & idx_mask;
      valid = e < cnt;
    } else {
      const uint32_t cr = chunk_rows[c]; // wave-uniform
      if ((int)(int16_t)(cr & 0xffffu) > rc.ty1 || (int)(int16_t)(cr >> 16) < rc.ty0) continue;
      my = c * 64u + (uint32_t)lane;
      valid = my < n_tris;
    }
    // (from here to the update rule: k_raster_slow's phase B)
    const u32x2 bb = bbox[min(my, n_tris - 1u)];
    const int bsx = (int16_t)(bb.x & 0xffff), bsy = (int16_t)(bb.x >> 16), bex = (int16_t)(bb.y & 0xffff), bey = (int16_t)(bb.y >> 16);
    const bool hit = valid && bsx <= bex && bex >= rc.tx0 && bsx <= rc.tx1 && bey >= rc.ty0 && bsy <= rc.ty1;
    unsigned long long m = __ballot(hit);
    if (m == 0ull) continue;
    TriXY t;
    t.ax = t.ay = t.bx = t.by = t.cx = t.cy = t.z0 = t.z1 = t.z2 = t.v_inv = t.s_area = 0.0f;
    // [4:0] x0  [9:5] x1  [14:10] y0  [19:15] y1  [25:20] v = first scalar-tail column  [27:26] / [29:28] log2(block width) - 2 of the V / S sweep
    uint32_t geom = 0;
    if (hit) {
      float p[9];
      load_pos9(tpos + (size_t)my * a.pos_stride, p);
      t.ax = p[0], t.ay = p[1], t.z0 = p[2], t.bx = p[3], t.by = p[4], t.z1 = p[5], t.cx = p[6], t.cy = p[7], t.z2 = p[8];
      BranchMath bm;
      tri_consts(bm, t);
      const int x0 = max(bsx, rc.tx0) - rc.tx0, x1 = min(bex, rc.tx1) - rc.tx0, y0 = max(bsy, rc.ty0) - rc.ty0, y1 = min(bey, rc.ty1) - rc.ty0;
      const int vend = (flags & SRZ_UNIFIED) ? bex + 1 : bsx + ((bex - bsx + 1) & ~7);
      const int v = min(max(vend - rc.tx0, x0), x1 + 1);
      const int h = y1 - y0 + 1, wv = v - x0, ws = x1 + 1 - v;
      auto pick = [h](int w) {
        const int n88 = ((w + 7) >> 3) * ((h + 7) >> 3), n164 = ((w + 15) >> 4) * ((h + 3) >> 2), n416 = ((w + 3) >> 2) * ((h + 15) >> 4);
        int l = 3;
        if (n164 < n88 && n164 <= n416) l = 4;
        if (n416 < n88 && n416 < n164) l = 2;
        return l;
      };
      geom = (uint32_t)x0 | ((uint32_t)x1 << 5) | ((uint32_t)y0 << 10) | ((uint32_t)y1 << 15) | ((uint32_t)v << 20) |
             ((uint32_t)(pick(wv) - 2) << 26) | ((uint32_t)(pick(ws) - 2) << 28);
    }
    while (m) {
      const int j = __builtin_ctzll(m);
      m &= m - 1;
      // broadcast triangle j to the wave (uniform values → SGPRs)
      TriXY u;
      u.ax = rl_f(t.ax, j), u.ay = rl_f(t.ay, j), u.bx = rl_f(t.bx, j), u.by = rl_f(t.by, j), u.cx = rl_f(t.cx, j);
      u.cy = rl_f(t.cy, j), u.z0 = rl_f(t.z0, j), u.z1 = rl_f(t.z1, j), u.z2 = rl_f(t.z2, j);
      u.v_inv = rl_f(t.v_inv, j), u.s_area = rl_f(t.s_area, j);
      const uint32_t idx = (uint32_t)rl_i((int)my, j);
      const uint32_t g = (uint32_t)rl_i((int)geom, j);
      const int x0 = g & 31, x1 = (g >> 5) & 31, y0 = (g >> 10) & 31, y1 = (g >> 15) & 31, vx = (g >> 20) & 63;
      if (y1 < y0) continue; // (cannot happen for a hit; keeps the loops well-formed)
      if (vx > x0) { // ---- "V" sweep over columns [x0, vx-1] (k_raster_slow's) ----------------------------------------
        const uint32_t tb = 0x80000000u | idx; // (uniform per triangle)
        const int lbw = (int)((g >> 26) & 3) + 2, bw = 1 << lbw, bh = 64 >> lbw;
        const int lx = lane & (bw - 1), ly = lane >> lbw;
        for (int yb = y0; yb <= y1; yb += bh) {
          const int yl = yb + ly;
          const float fy = (float)(rc.ty0 + yl);
          const float PBy = u.by - fy, PCy = u.cy - fy, PAy = u.ay - fy;
          const bool rowok = yl <= y1;
          for (int xb = x0; xb < vx; xb += bw) {
            const int xl = xb + lx;
            const float fx = (float)(rc.tx0 + xl);
            const float PBx = u.bx - fx, PCx = u.cx - fx, PAx = u.ax - fx;
            const float aPBC = fmsubf(PBx, PCy, PCx * PBy), aPCA = fmsubf(PCx, PAy, PAx * PCy);
            const float al = aPBC * u.v_inv, be = aPCA * u.v_inv, ga = 1.0f - (al + be);
            const float z = fmaf_(al, u.z0, fmaf_(be, u.z1, ga * u.z2));
            const int li = min(yl * LDS_STRIDE + xl, TILE * LDS_STRIDE - 1); // clamped: idle lanes read a valid word
            const bool inside = rowok & (xl < vx) & (al > 0.0f) & (be > 0.0f) & (ga > 0.0f) & (ga < 1.0f);
            // the update rule: strictly after prev's fragment, strictly before the best so far (a NaN z compares false throughout)
            const float zp = s_zp[li], bz = s_bz[li];
            const bool after = (z > zp) | ((z == zp) & (tb > s_tp[li]));
            const bool before = (z < bz) | ((z == bz) & (tb < s_bt[li]));
            if (inside & after & before) s_bz[li] = z, s_bt[li] = tb;
          }
        }
      }
      if (vx <= x1) { // ---- scalar-tail "S" sweep over columns [vx, x1] (k_raster_slow's) ------------------------------
        const uint32_t tb = 0x7ffffffeu - idx;
        const int lbw = (int)((g >> 28) & 3) + 2, bw = 1 << lbw, bh = 64 >> lbw;
        const int lx = lane & (bw - 1), ly = lane >> lbw;
        const float ABx = u.bx - u.ax, ABy = u.by - u.ay, BCx = u.cx - u.bx, BCy = u.cy - u.by, CAx = u.ax - u.cx,
                    CAy = u.ay - u.cy;
        for (int yb = y0; yb <= y1; yb += bh) {
          const int yl = yb + ly;
          const float fy = (float)(rc.ty0 + yl);
          const bool rowok = yl <= y1;
          for (int xb = vx; xb <= x1; xb += bw) {
            const int xl = xb + lx;
            const float fx = (float)(rc.tx0 + xl);
            // insideTriangle (src/Rasterizer.cpp:11-41)
            const float APx = fx - u.ax, APy = fy - u.ay, BPx = fx - u.bx, BPy = fy - u.by, CPx = fx - u.cx, CPy = fy - u.cy;
            const float e0 = ABx * APy - ABy * APx, e1 = BCx * BPy - BCy * BPx, e2 = CAx * CPy - CAy * CPx;
            const bool in_tri = ((e0 > 0) & (e1 > 0) & (e2 > 0)) | ((e0 < 0) & (e1 < 0) & (e2 < 0));
            // barycentric (scalar) + z (src/Rasterizer.cpp:43-70,473)
            const float PAx = u.ax - fx, PAy = u.ay - fy, PBx = u.bx - fx, PBy = u.by - fy, PCx = u.cx - fx, PCy = u.cy - fy;
            const float aPBC = PBx * PCy - PBy * PCx, aPCA = PCx * PAy - PCy * PAx;
            const float al = aPBC / u.s_area, be = aPCA / u.s_area, ga = 1.0f - al - be;
            const float z = al * u.z0 + be * u.z1 + ga * u.z2;
            const int li = min(yl * LDS_STRIDE + xl, TILE * LDS_STRIDE - 1);
            const bool inside = rowok & (xl <= x1) & in_tri;
            const float zp = s_zp[li], bz = s_bz[li];
            const bool after = (z > zp) | ((z == zp) & (tb > s_tp[li]));
            const bool before = (z < bz) | ((z == bz) & (tb < s_bt[li]));
            if (inside & after & before) s_bz[li] = z, s_bt[li] = tb;
          }
        }
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  // ---- write-out (k_raster_slow's phase C; the tie-breaks decode as in k_raster's) ------------------------------------------
  uint4 id4[4];
  bool any_owner = false;
  for (int it = 0; it < 4; ++it) {
    const uint4 q = *reinterpret_cast<const uint4 *>(&s_bt[(it * 8 + (lane >> 3)) * LDS_STRIDE + (lane & 7) * 4]);
    any_owner |= (q.x & q.y & q.z & q.w) != PEEL_NOBODY;
    auto id_of = [](uint32_t tb) { return tb == PEEL_NOBODY ? NO_TRI : (tb & 0x80000000u) ? (tb & 0x7fffffffu) : ((0x7ffffffeu - tb) | S_CLASS_BIT); };
    id4[it] = make_uint4(id_of(q.x), id_of(q.y), id_of(q.z), id_of(q.w));
  }
  const bool tile_has_owner = __ballot(any_owner) != 0ull; // wave-uniform
  for (int it = 0; it < 4; ++it) {
    const int ly = it * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
    const int y = rc.ty0 + ly, x4 = rc.tx0 + lx4;
    if (y > rc.ty1 || x4 > rc.tx1) continue;
    const float4 z4 = *reinterpret_cast<const float4 *>(&s_bz[ly * LDS_STRIDE + lx4]);
    float *gz = rc.out0 + (size_t)ly * W + x4;
    const bool full = vec_ok && x4 + 3 <= rc.tx1;
    if (tile_has_owner)
      quad_store(gz, rc.plane, {z4}, full, x4, rc.tx1);
    else // touched by a bbox but owned by nobody in this layer: the clear itself
      quad_store(gz, rc.plane, {z4, zero4, zero4, zero4}, full, x4, rc.tx1);
  }
  if (tile_has_owner) { // the owners of all of the tile's pixels, by index (32 bits each), and the tile's work entry
    uint32_t *slot = a.vis + ((size_t)frame * tiles_per_frame + tile) * PIX_SLOT;
    for (int it = 0; it < 4; ++it) ids_store4(slot, (uint32_t)((it * 8 + (lane >> 3)) * TILE + (lane & 7) * 4), id4[it], false, false);
    if (lane == 0) work_append(a, fd->flags, frame * tiles_per_frame + tile, work_entry(frame, lb, tx, false, false, 0u, 0u));
  }
}

// ================================================================================================================
// k_shade — VISIBILITY-FIRST SHADING: one workgroup per owned tile (persistent grid over the worklist).
// The tile's owned pixels arrive COMPACTED by semantics class (the rasteriser's write-out made the two lists: V pixels, then S
// pixels), so every wave runs one of the two shader variants with full lanes instead of both under divergence;
// colours go to LDS planes and leave as coalesced 16-byte stores.
// ================================================================================================================
// k_clear — the fused clear of every tile NO bbox reaches (k_bin's tile counts), i.e. most of the framebuffer.  It runs
// on a second stream NEXT TO k_raster, which skips those tiles: no LDS and < 32 VGPRs, so its waves fit beside the
// rasteriser's on every CU and the bulk of the frame's HBM writes drains under the visibility arithmetic.
// One work item = one band of one frame, written ROW-MAJOR: a wave-instruction covers 1 KiB of one framebuffer row
// (256 consecutive pixels), so runs of untouched tiles become long contiguous DRAM bursts instead of 128-byte tile rows
// 4 KiB apart — the same bytes occupy the memory system for less time, which is what the kernels beside it pay for.
// One work item = ONE PLANE of one band of one frame (round 6; rounds 2-5: one band, its four planes interleaved row by row).  A thread writes
// its 16 bytes of 32 consecutive rows of the plane: a workgroup streams one plane's rows instead of keeping four streams 4 MB apart going, and
// the memory system — which is what the compute kernels beside the clear wait for — takes the same bytes in less time: measured beside
// k_raster / k_shade, two lanes, at each form's best grid: config 2 0.645 -> 0.738 of the roofline, config 3 0.600 -> 0.675, config 4
// 0.411 -> 0.438, config 5 0.43 -> 0.444 (NOTEBOOK r6 §6; the rows of a plane written one after the other by the whole workgroup — fewer
// stores in flight per thread — is slower again: 0.67 on config 2).
__global__ __launch_bounds__(256) void k_clear(RenderArgs a) {
  const uint32_t n_items = a.n_frames * a.n_local_bands * 4u;
  const float inf = __builtin_inff();
  // the workgroups that take part: the whole grid, or — while the set measures its grid (srz_device.h, ClearCtl) — the first `wgs` of it
  uint32_t n_wgs = gridDim.x;
  if (a.clear_wgs_dev) {
    const uint32_t w = *as_const(a.clear_wgs_dev);
    n_wgs = min(w ? w : CLEAR_CAND[0], gridDim.x);
    if (blockIdx.x >= n_wgs) return;
  }
  for (uint32_t it = blockIdx.x; it < n_items; it += n_wgs) { // it = (frame * n_local_bands + lb) * 4 + plane
    const uint32_t br = it >> 2, pl = it & 3u;
    const uint32_t f = br / a.n_local_bands, lb = br % a.n_local_bands;
    const SRZ_CAS FrameDesc *fd = as_const(a.frames) + f;
    if (!((fd->flags | a.flags_or) & SRZ_FUSED_CLEAR)) continue;
    const int W = fd->width, H = fd->height;
    const int band = band_of((int)lb, a.shard_rank, a.shard_world);
    const int rows = min(BAND, H - band * BAND);
    const size_t plane = (size_t)a.local_rows * (size_t)W;
    float *base = a.out + (size_t)f * a.frame_stride + (size_t)lb * BAND * (size_t)W + pl * plane;
    const float v = pl == 0u ? inf : 0.f; // (plane 0 = z)
    const float4 v4 = make_float4(v, v, v, v);
    const SRZ_CAS u32x2 *cnt = as_const(reinterpret_cast<const u32x2 *>(a.tile_info)) + (size_t)br * a.tiles_x;
    for (int x4 = (int)threadIdx.x * 4; x4 < W; x4 += (int)blockDim.x * 4) {
      if (cnt[(uint32_t)x4 / TILE].x != 0u) continue; // some bbox reaches this tile: the rasteriser's
      if (((W & 3) == 0)) {
        for (int ly = 0; ly < rows; ++ly) store_nt(base + (size_t)ly * W + x4, v4);
      } else { // odd widths: scalar stores, the quad may end at the frame's edge or straddle nothing else (TILE % 4 == 0)
        for (int ly = 0; ly < rows; ++ly)
          for (int k = 0; k < 4 && x4 + k < W; ++k) base[(size_t)ly * W + x4 + k] = v;
      }
    }
  }
}


// k_shade is latency-sensitive: measurably slower at 3 waves per SIMD than at 4 — hold the allocator to 128 VGPRs
#ifndef SRZ_FAST_MINW
#define SRZ_FAST_MINW 6 // (80 VGPRs: the FAST builds for 1 / 2 lights fit with a few prologue spills; 3 lights keep 5 — see k_shade)
#endif
#ifndef SRZ_STAGE_TRIS
#define SRZ_STAGE_TRIS 96 // triangles of a tile's list k_shade stages in LDS (12 KB colours + 4 KB lists + 9 KB triangles: 6 workgroups per CU)
#endif
constexpr uint32_t STAGE_TRIS = SRZ_STAGE_TRIS, STAGE_SD = 16;
// (s_tri doubles as the {pixel, index} pair list of tiles whose ids are triangle indices: 2 dwords per pixel of the tile)
static_assert(SRZ_STAGE_TRIS * 6 * 16 >= 2 * 32 * 32 * 4, "SRZ_STAGE_TRIS: s_tri must hold a tile's 1024 {pixel, index} pairs (>= 86 triangles)");
#ifndef SRZ_GENPOW_MINW
#define SRZ_GENPOW_MINW 5 // (the builds with pow_fast: 81 VGPRs for two lights; held to 80 they spill 20 bytes into the chunk loops: -3 %)
#endif
#ifndef SRZ_SHADE_MINW
#define SRZ_SHADE_MINW 4
#endif
// Two builds of the same kernel share the persistent walk over the frames' work lists:
//   FAST     (one build per light count 1..4) frames whose shading is fully described at compile time up to the shader type and
//            the exponent: FASTNL lights, an integer exponent 0..256 (FD_FAST_SHADE + the count, decided on the host).  Per 64-pixel chunk ONE wave-uniform
//            switch picks the variant compiled for the chunk's shader type (mixed chunks take one pass per type);
//            optimistic FastMath only — a tile where an operand left the fast range is handed back through redo_list.
//   generic  every other frame with per-pixel generality (any shader, any light count, any exponent), FastMath first and
//            the IEEE expansions for a tile that needs them; then the tiles the FAST build handed back, IEEE at once.
//   FASTNL < 0: the FAST build for -FASTNL lights and a non-integer exponent in (0, 4096] (pow_fast; its ambiguous roundings go to the generic build) — frames that
//            differ from the common case only in Shader::p keep the per-chunk variants, the unrolled lights and the hoisted texel
//   APPROX   (SRZ_OPT_APPROX_SHADE, one build per light count 1..4): the FAST walk with the ApproxMath policy — the tolerance mode.
//            Any exponent (x^p is exp2(p log2 x) there), never a re-shade; frames it does not cover (0 or > 4 lights, BUMP /
//            DISPLACEMENT batches) keep the exact builds.
template <bool STATS, int FASTNL, bool BUMPY = false, bool APPROX = false>
__global__ __launch_bounds__(256, (FASTNL > 0 && FASTNL <= 2 && !BUMPY) ? SRZ_FAST_MINW : (FASTNL < 0 && FASTNL >= -2) ? SRZ_GENPOW_MINW
                                  : ((FASTNL == 3 || FASTNL == -3) && !BUMPY) ? 5 : SRZ_SHADE_MINW)
void k_shade(RenderArgs a) {
  constexpr bool FAST = FASTNL != 0, GENPOW = FASTNL < 0;
  static_assert(FAST || !BUMPY, "BUMPY is a property of the FAST builds");
  static_assert(!APPROX || (FASTNL > 0 && !BUMPY && !STATS), "the tolerance mode has FAST builds for 1..4 lights only");
  static_assert(!(GENPOW && BUMPY), "frames with BUMP / DISPLACEMENT batches and a non-integer exponent take the generic build");
  __shared__ __attribute__((aligned(16))) float s_c[3][TILE * TILE];
  // the tile's owned pixels compacted by class: V entries [0, nV), S entries [nV, nV + nS), row-major each; an entry = pixel |
  // owner's list position << 10 — or, for tiles whose ids are triangle indices, {pixel, index} pairs in s_tri's memory (no
  // triangles are staged for those)
  __shared__ __attribute__((aligned(16))) uint32_t s_ent[PIX_SLOT];
  __shared__ uint32_t s_wcnt[4];                                        // per wave: V-class | S-class << 16 pixels among its 256
  // the triangles of the tile's list, staged once per tile (96 bytes each, by list position) + their batch ids, and the frame's
  // shader descriptors: a pixel takes its owner's data from here instead of gathering it from memory — 26 KB of LDS in all,
  // six workgroups per CU as before
  __shared__ __attribute__((aligned(16))) f32x4 s_tri[STAGE_TRIS * 6];
  __shared__ uint16_t s_bat[STAGE_TRIS];
  __shared__ __attribute__((aligned(16))) ShadeDescG s_sd[STAGE_SD];
  __shared__ uint32_t s_flag;                                           // "some operand left FastMath's range"

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned long long n_vis = 0, n_vis_tex = 0;
#ifdef SRZ_PHASE_PROBE /* dev build (tools/mkvariant.sh probe -DSRZ_PHASE_PROBE, tools/phase_probe.py): where a wave's time per tile goes */
  unsigned long long ph[6] = {0, 0, 0, 0, 0, 0}, ph_t = 0;
  // (and the clock the wave ran at: shader clocks against the constant 100 MHz counter over the wave's whole life)
  const unsigned long long ph_c0 = __builtin_amdgcn_s_memtime(), ph_r0 = __builtin_amdgcn_s_memrealtime();
#define SRZ_STAMP(K) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); ph[K] += t_ - ph_t, ph_t = t_; }
#else
#define SRZ_STAMP(K)
#endif

  // ---- one owned tile: x = its work-list entry (work_append).  mode: 0 = FAST variants, 1 = generic (FastMath, then IEEE if
  //      needed), 2 = IEEE at once -------------------------------------------------------------------------------------------------
  auto shade_tile = [&](const u32x4 x, auto mode_c) {
    constexpr int MODE = decltype(mode_c)::value;
    // (everything a thread derives from its index is derived HERE, per tile, from an opaque copy: hoisted out of the tile loop
    // those values live across the chunk loops, get spilled, and every tile starts with scratch round trips in front of its loads)
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
#ifdef SRZ_PHASE_PROBE
    ph_t = __builtin_amdgcn_s_memtime(), ph[5] += 1;
#endif
    // (likewise the kernel's arguments: read from the kernarg segment per tile — scalar loads that hit the constant cache —
    // through an opaque pointer.  Loaded once at kernel entry they are ~50 scalar registers alive across everything: the compiler
    // parks them in VGPR lanes (v_writelane) and fetches them back with a VALU instruction each (v_readlane), 8 % of the
    // kernel's vector instructions)
    const SRZ_CAS RenderArgs *ap = (const SRZ_CAS RenderArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ap));
    const uint32_t tpf = ap->n_local_bands * ap->tiles_x;
    // how the tile's ids name a pixel's owner: by position in the tile's triangle list (16-bit ids) — the list's triangles are
    // staged in LDS if they fit (by_lp && staged), else looked up per pixel (by_lp) — or by index in the frame (32-bit ids)
    const bool by_lp = (x.y & WORK_LP) != 0u, staged = by_lp && x.z <= STAGE_TRIS; // workgroup-uniform
    const bool lp8 = (x.y & WORK_LP8) != 0u;                                        // (8-bit ids: id_pack8)
    const SRZ_CAS uint32_t *tlist = as_const(ap->pool) + x.w;
    // ---- 1. this thread's 4 pixels: their owner ids (nothing but the entry is needed for the address: the load is in flight
    //         under the frame descriptor's scalar loads), and the indices of the list entries whose pieces it will stage
    const int ly = wave * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
    const int p0 = ly * TILE + lx4;
    // (the 16-bit codes are classified as they are — position | 0x8000 for the S class, 0xffff = nobody —, never widened; and they
    // are taken apart only at the classification below: unpacked here, the wait for this load would sit in front of the index
    // loads that follow, one more round trip in a row per tile)
    const uint32_t f = x.x, lb = x.y & 1023u, tx = (x.y >> 10) & 1023u;
    const uint32_t tile_slot = f * tpf + lb * ap->tiles_x + tx;
    uint4 id_raw = make_uint4(0u, 0u, 0u, 0u);
    { // (inline copy of ids_load_raw; `none` / `sbit` below: of id_none / id_sbit; by_lp, lp8, f, lb, tx above: of work_decode)
      const uint32_t *slot = ap->vis + (size_t)tile_slot * PIX_SLOT;
      if (lp8) {
        id_raw.x = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(slot) + p0);
      } else if (by_lp) {
        const u32x2 w = *reinterpret_cast<const u32x2 *>(reinterpret_cast<const uint16_t *>(slot) + p0);
        id_raw.x = w.x, id_raw.y = w.y;
      } else {
        id_raw = *reinterpret_cast<const uint4 *>(slot + p0);
      }
    }
    const uint32_t none = lp8 ? 0xffu : by_lp ? 0xffffu : NO_TRI, sbit = lp8 ? 0x80u : by_lp ? 0x8000u : S_CLASS_BIT; // (scalar)
    constexpr int PASSES = (STAGE_TRIS * 6 + 255) / 256;
    const uint32_t n_pc = staged ? x.z * 6u : 0u;
    uint32_t ti[PASSES];
#pragma unroll
    for (int k = 0; k < PASSES; ++k) { // (passes the list does not reach are skipped by a SCALAR branch: most lists fit the first)
      ti[k] = 0u;
      if (n_pc > 256u * k) {
        const uint32_t pc = (uint32_t)tid + 256u * k;
        if (pc < n_pc) ti[k] = tlist[pc / 6u];
      }
    }
    const SRZ_CAS FrameDesc *fd = as_const(ap->frames) + f;
    const int W = fd->width, H = fd->height;
    const uint32_t tri_off = fd->tri_off, batch_off = fd->batch_off;
    const uint32_t flags = fd->flags | ap->flags_or;
    const bool fused = (flags & SRZ_FUSED_CLEAR) != 0;
    const SRZ_CAS srz_tri *tris = as_const(ap->tris) + tri_off;
    const SRZ_CAS uint16_t *tri_batch = as_const(ap->tri_batch) + tri_off;
    const SRZ_CAS ShadeDescG *sdesc = as_const(ap->sdesc) + batch_off;
    const bool sd_staged = fd->n_batches <= STAGE_SD; // workgroup-uniform

    const int band = band_of((int)lb, ap->shard_rank, ap->shard_world); // (inline copy of tile_rect, to out0)
    const int tx0 = (int)tx * TILE, ty0 = band * BAND;
    const int tx1 = min(tx0 + TILE, W) - 1, ty1 = min(ty0 + BAND, H) - 1;
    const size_t plane = (size_t)ap->local_rows * (size_t)W;
    const size_t row0 = (size_t)lb * BAND;
    float *out0 = ap->out + (size_t)f * ap->frame_stride + row0 * (size_t)W;

    // (the frame's shader descriptors: loaded here, parked in LDS behind the first barrier — the store's wait for the load would
    // otherwise hold wave 0, and with it the barrier, until this load, the last one issued, is back)
    const bool sd_mine = sd_staged && (uint32_t)tid < fd->n_batches;
    ShadeDescG sd_reg;
    sd_reg.shader = 0, sd_reg.tw = sd_reg.th = 1, sd_reg._pad = 0, sd_reg.tex = nullptr;
    if (sd_mine) {
      const SRZ_CAS ShadeDescG *g = sdesc + tid;
      sd_reg.shader = g->shader, sd_reg.tw = g->tw, sd_reg.th = g->th, sd_reg.tex = g->tex;
    }

    // ---- 2. the colour staging planes start as what the pixels this call does not own must hold: 0 after the fused clear, else
    //         the colour already in the framebuffer (the z plane is not read: the shader's depth is recomputed from the owner
    //         triangle with k_raster's own operations, which is cheaper than 4 bytes per pixel of HBM read)
    const int y = ty0 + ly, x4 = tx0 + lx4;
    const bool in_tile = y <= ty1 && x4 <= tx1;
    const bool full = in_tile && ((W & 3) == 0) && x4 + 3 <= tx1;
    float *gz = out0 + (size_t)ly * W + x4;
    float4 C0 = make_float4(0.f, 0.f, 0.f, 0.f), C1 = C0, C2 = C0;
    if (!fused) { // keep the colour of pixels this call does not own
      if (full) {
        C0 = *reinterpret_cast<const float4 *>(gz + plane);
        C1 = *reinterpret_cast<const float4 *>(gz + 2 * plane);
        C2 = *reinterpret_cast<const float4 *>(gz + 3 * plane);
      } else if (in_tile) {
        if (x4 + 0 <= tx1) C0.x = gz[plane + 0], C1.x = gz[2 * plane + 0], C2.x = gz[3 * plane + 0];
        if (x4 + 1 <= tx1) C0.y = gz[plane + 1], C1.y = gz[2 * plane + 1], C2.y = gz[3 * plane + 1];
        if (x4 + 2 <= tx1) C0.z = gz[plane + 2], C1.z = gz[2 * plane + 2], C2.z = gz[3 * plane + 2];
        if (x4 + 3 <= tx1) C0.w = gz[plane + 3], C1.w = gz[2 * plane + 3], C2.w = gz[3 * plane + 3];
      }
    }
    *reinterpret_cast<float4 *>(&s_c[0][p0]) = C0;
    *reinterpret_cast<float4 *>(&s_c[1][p0]) = C1;
    *reinterpret_cast<float4 *>(&s_c[2][p0]) = C2;
    // classify this thread's 4 pixels: per-thread counts, one packed wave scan (DPP), the waves' totals through LDS
#ifdef SRZ_PHASE_PROBE
    asm volatile("" : "+v"(id_raw.x), "+v"(id_raw.y), "+v"(ti[0])); // (the wait for the owner ids and the first indices lands here)
    SRZ_STAMP(0) // tile start → owner ids + list indices here
#endif
    uint32_t idk[4] = {id_raw.x, id_raw.y, id_raw.z, id_raw.w}; // (inline copy of ids_unpack4)
    if (lp8)
      idk[0] = id_raw.x & 0xffu, idk[1] = (id_raw.x >> 8) & 0xffu, idk[2] = (id_raw.x >> 16) & 0xffu, idk[3] = id_raw.x >> 24;
    else if (by_lp)
      idk[0] = id_raw.x & 0xffffu, idk[1] = id_raw.x >> 16, idk[2] = id_raw.y & 0xffffu, idk[3] = id_raw.y >> 16;
    uint32_t cnt2 = 0; // V count | S count << 16 of this thread
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt2 += idk[k] == none ? 0u : ((idk[k] & sbit) ? 0x10000u : 1u);
    const uint32_t incl2 = wave_scan_add(cnt2);
    if (lane == 63) s_wcnt[wave] = incl2;
    if (tid == 0) s_flag = 0;
    // ---- 1b. the tile's triangles → LDS by DMA: 16-byte piece q of list entry l per thread (six threads per triangle: coalesced
    //          96 bytes).  The pieces go from memory straight to LDS — the wave's 64 land one after the other at a wave-uniform
    //          base, which is s_tri's own order — and hold no registers while in flight, under the compaction below
    if (staged) {
#pragma unroll
      for (int k = 0; k < PASSES; ++k) {
        if (n_pc <= 256u * k) break; // scalar
        const uint32_t pc = (uint32_t)tid + 256u * k;
        if (pc < n_pc) {
          const uint32_t q = pc % 6u;
          __builtin_amdgcn_global_load_lds(reinterpret_cast<const f32x4 *>(ap->tris + tri_off + (ti[k] & PACK_IDX_MASK)) + q,
                                           (__attribute__((address_space(3))) void *)(s_tri + (wave * 64 + 256 * k)), 16, 0, 0);
          if (q == 0u) s_bat[pc / 6u] = (uint16_t)(ti[k] >> PACK_IDX_BITS); // (by_lp = FD_PACKED: the list entry carries the batch)
        }
      }
    }
    // raw barrier: only the LDS stores above must be visible (lgkmcnt); the DMA pieces stay in flight across it.  s_barrier is
    // IntrNoMem for the compiler: the two empty asm statements are compiler-level fences that keep the LDS stores above in front
    // of it and the reads of the other waves' s_wcnt[] behind it (no instruction, vmcnt untouched)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xc07f); // lgkmcnt(0), vmcnt / expcnt untouched
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    SRZ_STAMP(1) // → classification done, first barrier passed
    uint32_t bV = 0, bS = 0, nV = 0, nS = 0; // this wave's first slot in each list, list lengths (all wave-uniform)
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) {
      const uint32_t t2 = s_wcnt[w2];
      bV += w2 < wave ? (t2 & 0xffffu) : 0u, bS += w2 < wave ? (t2 >> 16) : 0u, nV += t2 & 0xffffu, nS += t2 >> 16;
    }
    nV = (uint32_t)__builtin_amdgcn_readfirstlane((int)nV), nS = (uint32_t)__builtin_amdgcn_readfirstlane((int)nS);
    if (sd_mine) s_sd[tid] = sd_reg;
    uint32_t *const s_ent2 = reinterpret_cast<uint32_t *>(s_tri); // ({pixel, index} pairs: tiles without staged triangles)
    {
      uint32_t oV = bV + ((incl2 - cnt2) & 0xffffu), oS = nV + bS + ((incl2 - cnt2) >> 16);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool own = idk[k] != none, isS = own && (idk[k] & sbit) != 0;
        const uint32_t o = isS ? oS : oV, owner = idk[k] & ~sbit;
        if (own) {
          if (by_lp)
            s_ent[o] = (uint32_t)(p0 + k) | (owner << PIX_BITS);
          else
            s_ent2[2 * o] = (uint32_t)(p0 + k), s_ent2[2 * o + 1] = owner;
        }
        oV += (own && !isS) ? 1u : 0u, oS += isS ? 1u : 0u;
      }
    }
    // (the DMA pieces must have landed: an LDS-DMA is a pending LDS write on the vector-memory counter — the barrier's fence waits
    // for it by itself with this compiler; the explicit wait states the requirement)
    __builtin_amdgcn_s_waitcnt(0x0f70); // vmcnt(0), expcnt / lgkmcnt untouched
    __syncthreads();
    SRZ_STAMP(2) // → compaction done, staged triangles landed, second barrier passed

    // ---- 3. dense passes: the two lists are cut into 64-entry chunks dealt round-robin to the 4 waves, so a wave runs
    //         ONE shader variant per chunk with (nearly) all lanes busy; only the last chunk of each list is partial.
    const uint32_t cV = (nV + 63) >> 6, cS = (nS + 63) >> 6;
    // (one loop per class: a single loop over both keeps the registers of the V and of the S shader alive together)
    auto class_pass = [&](auto policy, auto is_v, auto staged_c, bool count) -> bool {
      using M = decltype(policy);
      constexpr bool isV = decltype(is_v)::value, STAGED = decltype(staged_c)::value;
      bool bad = false;
      // the frame's shading constants are (re)read here, after the IO phase: scalar loads from a hot line, and ~20 SGPRs
      // fewer alive across the phase that has none to spare (inline copy of frame_k)
      FrameK K;
      K.eye[0] = fd->eye[0], K.eye[1] = fd->eye[1], K.eye[2] = fd->eye[2];
      K.ka[0] = fd->ka[0], K.ka[1] = fd->ka[1], K.ka[2] = fd->ka[2];
      K.ks[0] = fd->ks[0], K.ks[1] = fd->ks[1], K.ks[2] = fd->ks[2];
      K.p = fd->p, K.kh = fd->kh, K.kn = fd->kn, K.n_lights = fd->n_lights;
      K.grey = (fd->flags & FD_GREY) != 0u;
      K.lights = as_const(ap->lights) + fd->light_off;
      // chunk c of the tile, dealt round-robin to the waves: the S chunks first (the dearer ones: ~450 instructions against ~310), so that
      // the waves' loads differ by at most one V chunk at the barrier behind the passes
      for (uint32_t c = (uint32_t)wave; c < cV + cS; c += 4) {
        if ((c >= cS) != isV) continue;
        const uint32_t i = (isV ? c - cS : c) * 64 + lane;
        if (i >= (isV ? nV : nS)) continue;
        const uint32_t slot = isV ? i : nV + i;
        uint32_t p, id;
        if (by_lp) {
          const uint32_t en = s_ent[slot];
          p = en & PIX_MASK, id = en >> PIX_BITS;
        } else {
          p = s_ent2[2 * slot], id = s_ent2[2 * slot + 1];
        }
        float r0 = 1.f, r1 = 2.f, r2 = 3.f;
        ShadeDesc sd;
        TriFetch tf;
        const f32x4 *late = nullptr;
        if constexpr (STAGED) { // the owner's positions and its batch from the tile's staged list now, its attributes later (late_fetch)
          late = s_tri + id * 6u; // (read inside the shading variant: early_fetch / late_fetch)
          tf.batch = s_bat[id];
        } else {
          if (by_lp) id = tlist[id] & PACK_IDX_MASK; // (a list too long for the stage: position → index, then the gather)
          fetch_tri(tris, tri_batch, id, tf);
        }
        const int px = tx0 + (int)(p & 31), py = ty0 + (int)(p >> 5);
        M m;
        if constexpr (MODE == 0) {
          // The pixels of a chunk are shaded batch by batch (nearly always there is one): the batch's shader descriptor — type,
          // texture size and address — is WAVE-UNIFORM (scalar registers: LDS read + readfirstlane, or scalar loads), one
          // scalar switch picks the variant compiled for its shader type, and the lanes of other batches wait for their pass
          bool todo = true;
          for (unsigned long long tm = __ballot(true); tm != 0ull; tm = __ballot(todo)) {
            const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)tf.batch, __builtin_ctzll(tm)); // batch of the first pixel still to do
            if (sd_staged) {
              const ShadeDescG &g = s_sd[b0];
              const unsigned long long tp = reinterpret_cast<unsigned long long>(g.tex);
              sd.shader = __builtin_amdgcn_readfirstlane(g.shader), sd.tw = __builtin_amdgcn_readfirstlane(g.tw);
              sd.th = __builtin_amdgcn_readfirstlane(g.th);
              sd.tex = reinterpret_cast<const SRZ_CAS uint32_t *>((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tp) |
                                                                  ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(tp >> 32)) << 32));
            } else {
              const SRZ_CAS ShadeDescG *g = sdesc + b0; // (uniform address: scalar loads)
              sd.shader = g->shader, sd.tw = g->tw, sd.th = g->th, sd.tex = as_const(g->tex);
            }
            if (todo && tf.batch == b0) {
              auto run = [&](auto sh) {
                if constexpr (isV)
                  shade_pixel_v<M, decltype(sh)::value, FASTNL>(m, K, sd, tf, late, px, py, r0, r1, r2);
                else
                  shade_pixel_s<M, decltype(sh)::value, FASTNL>(m, K, sd, tf, late, px, py, r0, r1, r2);
              };
              const int sh0 = sd.shader; // wave-uniform
              if (sh0 == SRZ_SHADER_TEXTURE)
                run(std::integral_constant<int, SRZ_SHADER_TEXTURE>{});
              else if (sh0 == SRZ_SHADER_PHONG)
                run(std::integral_constant<int, SRZ_SHADER_PHONG>{});
              else if (!BUMPY || sh0 == SRZ_SHADER_NORMAL)
                run(std::integral_constant<int, SRZ_SHADER_NORMAL>{});
              else if constexpr (BUMPY) { // (the builds for frames with BUMP / DISPLACEMENT batches: their scalar-tail variants
                                          // cost ~20 VGPRs more than the other three types need)
                if (sh0 == SRZ_SHADER_BUMP)
                  run(std::integral_constant<int, SRZ_SHADER_BUMP>{});
                else
                  run(std::integral_constant<int, SRZ_SHADER_DISPLACEMENT>{});
              }
              todo = false;
            }
          }
        } else {
          if (sd_staged) {
            const ShadeDescG &g = s_sd[tf.batch];
            sd.shader = g.shader, sd.tw = g.tw, sd.th = g.th, sd.tex = as_const(g.tex);
          } else {
            const SRZ_CAS ShadeDescG *g = sdesc + tf.batch;
            sd.shader = g->shader, sd.tw = g->tw, sd.th = g->th, sd.tex = as_const(g->tex);
          }
          if constexpr (isV)
            shade_pixel_v<M>(m, K, sd, tf, late, px, py, r0, r1, r2);
          else
            shade_pixel_s<M>(m, K, sd, tf, late, px, py, r0, r1, r2);
        }
        if constexpr (std::is_same<M, FastMath>::value) bad |= m.is_bad();
        s_c[0][p] = r0, s_c[1][p] = r1, s_c[2][p] = r2;
        if (STATS && count)
          n_vis++, n_vis_tex += (sd.shader == SRZ_SHADER_TEXTURE || sd.shader == SRZ_SHADER_DISPLACEMENT || sd.shader == SRZ_SHADER_BUMP);
      }
      return bad;
    };
    auto dense_passes = [&](auto policy, bool count) -> bool {
      bool bv, bs;
      if (staged) { // workgroup-uniform
        bv = class_pass(policy, std::true_type{}, std::true_type{}, count);
        bs = class_pass(policy, std::false_type{}, std::true_type{}, count);
      } else {
        bv = class_pass(policy, std::true_type{}, std::false_type{}, count);
        bs = class_pass(policy, std::false_type{}, std::false_type{}, count);
      }
      return bv | bs;
    };
    bool skip_write = false;
    if constexpr (APPROX) {
      dense_passes(ApproxMath{}, true);
      __syncthreads();
    } else if constexpr (MODE == 2) {
      if (STATS && tid == 0) atomicAdd(&ap->stats[ST_DBG_IEEE_TILES], 1ull);
      dense_passes(IeeeMath{}, true);
      __syncthreads();
    } else {
      // First with the optimistic FastMath; a tile where any operand left the fast range (degenerate normals, a light
      // straight above a pixel, ...) is shaded again with the IEEE expansions.
      const bool bad = dense_passes(FastMath{}, true);
      if (__ballot(bad) != 0ull && lane == 0) s_flag = 1u;
      __syncthreads();
      if (s_flag) { // workgroup-uniform
        if constexpr (MODE == 0) { // hand the tile to the generic build
          if (tid == 0) ap->redo_list[atomicAdd(ap->redo_count, 1u)] = make_uint4(x.x, x.y, x.z, x.w);
          skip_write = true;
        } else {
          if (STATS && tid == 0) atomicAdd(&ap->stats[ST_DBG_IEEE_TILES], 1ull);
          dense_passes(IeeeMath{}, false);
          __syncthreads();
        }
      }
    }

    SRZ_STAMP(3) // → dense passes done (and the barrier behind them)
    // ---- 4. coalesced write-out of the three colour planes ----------------------------------------------------------
    if (!skip_write) {
      C0 = *reinterpret_cast<const float4 *>(&s_c[0][p0]);
      C1 = *reinterpret_cast<const float4 *>(&s_c[1][p0]);
      C2 = *reinterpret_cast<const float4 *>(&s_c[2][p0]);
      if (full) {
        store_nt(gz + plane, C0);
        store_nt(gz + 2 * plane, C1);
        store_nt(gz + 3 * plane, C2);
      } else if (in_tile) {
        if (x4 + 0 <= tx1) gz[plane + 0] = C0.x, gz[2 * plane + 0] = C1.x, gz[3 * plane + 0] = C2.x;
        if (x4 + 1 <= tx1) gz[plane + 1] = C0.y, gz[2 * plane + 1] = C1.y, gz[3 * plane + 1] = C2.y;
        if (x4 + 2 <= tx1) gz[plane + 2] = C0.z, gz[2 * plane + 2] = C1.z, gz[3 * plane + 2] = C2.z;
        if (x4 + 3 <= tx1) gz[plane + 3] = C0.w, gz[2 * plane + 3] = C1.w, gz[3 * plane + 3] = C2.w;
      }
    }
    SRZ_STAMP(4) // → write-out issued
  };

  // Workgroup b (on XCD b % 8) shades entries b/8, b/8 + G/8, ... of work list [this build][b % 8]: the tiles of the frames
  // that XCD rasterised (its L2 holds their pixel lists), in frame order.  The grid is LARGE (a tile or two per workgroup),
  // so the hardware dispatcher hands the work out in order and at tile granularity: all resident workgroups are on the same
  // few frames at any time (triangles + lists stay cache-resident), a CU slowed by the clear's waves simply receives fewer
  // workgroups, the kernel's tail is a tile long — and, unlike a persistent grid, CU slots keep turning over, which lets the
  // kernels of another stream (LaneRenderer: the next batch's k_bin / k_raster) in beside this one.  Measured on MI355X, 256
  // frames of 1024^2: a persistent grid of 4096 workgroups dealing every 128th tile of a frame 0.78 ms (one stream), a
  // persistent grid drawing tiles from atomic cursors the same on one stream but 7 % slower on two (it holds every CU slot to
  // its end), this walk 0.73 ms.
  constexpr uint32_t KIND = build_kind<FASTNL, BUMPY>();
  const uint32_t L = KIND * 8u + (blockIdx.x & 7u), Ls = ((uint32_t)(a.kind_slots >> (4u * KIND)) & 15u) * 8u + (blockIdx.x & 7u);
  const SRZ_CAS u32x4 *list = reinterpret_cast<const SRZ_CAS u32x4 *>(as_const(a.worklist)) + (size_t)Ls * a.work_cap;
  // the list's length and this workgroup's first entry are loaded TOGETHER (the entry's index is clamped into the list's
  // storage; it is used only if it lies below the length): one round trip instead of two before the tile's own loads start
  uint32_t w = blockIdx.x >> 3;
  u32x4 x = list[min(w, a.work_cap - 1u)];
  const uint32_t n_work = (FAST || a.force_generic || a.any_generic) ? as_const(a.work_count)[L * CNT_STRIDE] : 0u;
  while (w < n_work) {
    const u32x4 xc = x;
    w += gridDim.x >> 3;
    if (w < n_work) x = list[w];
    if constexpr (FAST)
      shade_tile(xc, std::integral_constant<int, 0>{});
    else
      shade_tile(xc, std::integral_constant<int, 1>{});
    __syncthreads(); // LDS is reused by the next tile
  }

  if constexpr (!FAST) { // the tiles the FAST build handed back (it ran before this kernel on the same stream)
    const uint32_t n_redo = *as_const(a.redo_count);
    for (uint32_t i = blockIdx.x; i < n_redo; i += gridDim.x) {
      const u32x4 xr = reinterpret_cast<const SRZ_CAS u32x4 *>(as_const(a.redo_list))[i];
      shade_tile(xr, std::integral_constant<int, 2>{});
      __syncthreads(); // LDS is reused by the next tile
    }

  }
#ifdef SRZ_PHASE_PROBE
  if (lane == 0 && FAST) {
    for (int k = 0; k < 6; ++k)
      if (ph[k]) atomicAdd(&a.stats[ST_DBG_CYC_A + k], ph[k]);
    atomicAdd(&a.stats[0], __builtin_amdgcn_s_memtime() - ph_c0), atomicAdd(&a.stats[1], __builtin_amdgcn_s_memrealtime() - ph_r0);
  }
#endif
  if (STATS) {
    for (int o = 32; o > 0; o >>= 1) {
      n_vis += __shfl_down(n_vis, o);
      n_vis_tex += __shfl_down(n_vis_tex, o);
    }
    if (lane == 0) {
      if (n_vis) atomicAdd(&a.stats[ST_VISIBLE], n_vis);
      if (n_vis_tex) atomicAdd(&a.stats[ST_VISIBLE_TEX], n_vis_tex);
    }
  }
}

// ================================================================================================================
// k_visibility — the VISIBILITY BUFFER in place of the shaded colour (srz_frameset_render_visibility, layout: include/srz.h):
// plane 1 = owner's index in the frame + 1 | S class << 31 (0 = nobody), planes 2 / 3 = the owner's α / β exactly as k_shade
// computes them (cover_v with the correctly rounded reciprocal, cover_s with the IEEE division).  Plane 0 is k_raster's.
// One workgroup per owned tile, walking every work list a render filled (all build kinds, this workgroup's XCD list of each);
// a thread owns 4 consecutive pixels of one row, so nothing is compacted or staged for the write-out: the three quads leave as
// 16-byte non-temporal stores straight from registers.  Only the owner's 36 bytes of positions are read (the dense copy), staged
// in LDS once per tile for lists of up to VIS_STAGE entries whose ids are list positions, gathered per pixel otherwise.  The
// bound is the memory system: 12 bytes written per pixel of an owned tile + 1 / 2 / 4 bytes of owner ids read.
// ================================================================================================================
constexpr uint32_t VIS_STAGE = 256; // one list entry per thread
__global__ __launch_bounds__(256) void k_visibility(RenderArgs a) {
  __shared__ float s_pos[VIS_STAGE * TRI_POS_F];
  __shared__ uint32_t s_idx[VIS_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ly = wave * 8 + (lane >> 3), lx4 = (lane & 7) * 4, p0 = ly * TILE + lx4;
  const uint32_t sub = blockIdx.x & 7u, step = gridDim.x >> 3;
  const uint32_t tpf = a.n_local_bands * a.tiles_x;
  for (uint32_t kind = 0; kind <= SHADE_KIND_GENERIC; ++kind) {
    const uint32_t n_work = as_const(a.work_count)[(kind * 8u + sub) * CNT_STRIDE];
    if (n_work == 0u) continue; // (wave-uniform: kinds no frame of the set needs have no storage slot and count 0)
    const SRZ_CAS u32x4 *list = reinterpret_cast<const SRZ_CAS u32x4 *>(as_const(a.worklist)) + (size_t)work_slot(a, kind, sub) * a.work_cap;
    for (uint32_t w = blockIdx.x >> 3; w < n_work; w += step) {
      const Work e = work_decode(list[w]);
      const bool staged = e.by_lp && e.cnt <= VIS_STAGE;
      const SRZ_CAS uint32_t *tlist = as_const(a.pool) + e.off;
      // 1. this thread's 4 owner ids
      uint32_t idk[4];
      ids_unpack4(ids_load_raw(a.vis + (size_t)(e.f * tpf + e.lb * a.tiles_x + e.tx) * PIX_SLOT, p0, e.by_lp, e.lp8), e.by_lp, e.lp8, idk);
      const uint32_t none = id_none(e.by_lp, e.lp8), sbit = id_sbit(e.by_lp, e.lp8);
      const SRZ_CAS FrameDesc *fd = as_const(a.frames) + e.f;
      const int W = fd->width;
      const uint32_t tri_off = fd->tri_off;
      const bool fused = ((fd->flags | a.flags_or) & SRZ_FUSED_CLEAR) != 0;
      const SRZ_CAS float *tpos = as_const(a.tri_pos) + (size_t)tri_off * a.pos_stride;
      // 2. a short list's positions → LDS, by list position (one entry per thread)
      if (staged && (uint32_t)tid < e.cnt) {
        const uint32_t idx = tlist[tid] & PACK_IDX_MASK; // (by_lp = FD_PACKED: the entry carries the batch above the index)
        const SRZ_CAS float *q = tpos + (size_t)idx * a.pos_stride;
        s_idx[tid] = idx;
#pragma unroll
        for (int k = 0; k < (int)TRI_POS_F; ++k) s_pos[tid * TRI_POS_F + k] = q[k];
      }
      __syncthreads();
      const TileRect rc = tile_rect(a, fd, e.f, e.lb, e.tx);
      const int y = rc.ty0 + ly, x4 = rc.tx0 + lx4;
      const bool in_tile = y <= rc.ty1 && x4 <= rc.tx1;
      const bool full = in_tile && ((W & 3) == 0) && x4 + 3 <= rc.tx1;
      float *gz = rc.out0 + (size_t)ly * W + x4;
      float o[3][4]; // (inline copy of quad_load into float4[3] / quad_at: as float4s the staging costs 13 VGPRs and a wave per SIMD)
#pragma unroll
      for (int k = 0; k < 4; ++k) o[0][k] = o[1][k] = o[2][k] = 0.f;
      if (!fused && in_tile) { // accumulate mode: pixels nobody owns keep what the buffer holds
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (x4 + k <= rc.tx1) o[pl][k] = gz[(pl + 1) * rc.plane + k];
      }
      // 3. α and β of each owned pixel from its owner's positions
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (idk[k] == none || !in_tile) continue;
        const bool isS = (idk[k] & sbit) != 0u;
        const uint32_t pos = idk[k] & ~sbit;
        TriXY t;
        uint32_t idx;
        if (staged) {
          idx = s_idx[pos];
          t = tri_xy(s_pos + pos * TRI_POS_F);
        } else {
          idx = e.by_lp ? (tlist[pos] & PACK_IDX_MASK) : pos; // (a long list: position → index, then the gather)
          t = tri_xy(tpos + (size_t)idx * a.pos_stride);
        }
        BranchMath m; // (the correctly rounded reciprocal, no flag-and-redo: there is no redo list here)
        tri_consts(m, t);
        const float fx = (float)(x4 + k), fy = (float)y;
        float alpha, beta, gamma, zz;
        if (isS)
          cover_s(t, fx, fy, alpha, beta, gamma, zz);
        else
          cover_v(t, fx, fy, alpha, beta, gamma, zz);
        o[0][k] = u2f_((idx + 1u) | (isS ? S_CLASS_BIT : 0u)), o[1][k] = alpha, o[2][k] = beta;
      }
      // 4. planes 1..3 of the tile's rows
      if (in_tile) {
        const float4 q[3] = {make_float4(o[0][0], o[0][1], o[0][2], o[0][3]), make_float4(o[1][0], o[1][1], o[1][2], o[1][3]), make_float4(o[2][0], o[2][1], o[2][2], o[2][3])};
        quad_store(gz + rc.plane, rc.plane, q, full, x4, rc.tx1);
      }
      __syncthreads(); // s_pos / s_idx are reused by the next tile
    }
  }
}

// ================================================================================================================
// THE WALK OF THE PASSES OVER A VISIBILITY BUFFER (k_shade_vis and the kernels behind it, down to k_tex_mip_grad).  No work lists: the
// buffer is all there is, so the grid (tile_grid: one workgroup per tile up to a cap) walks every (frame, 32x32 tile) of the set in
// k_shade's XCD order: workgroup b takes the frames f ≡ b mod 8, whose triangles stay in its XCD's L2, tile after tile, gridDim / 8
// tiles apart; a set of fewer than 8 frames has its tiles dealt round-robin instead, so that every XCD has work.  Within a tile a
// thread owns 4 consecutive pixels of one row (k_visibility's deal: 8 threads a row, a wave 8 rows), so every plane is read and
// written in 16-byte accesses.
//   pass_tiles  the striding loop and the (frame, tile) decode: body(f, t) per tile of this workgroup;
//   pass_tile   a thread's place in tile t of frame f: the tile's rectangle (tile_rect), the thread's row and first column, whether
//               it lies inside, whether its quad is whole, and where its pixels are in a frame's plane 0 and in `out`;
//   pass_walk   the two together.  A kernel with barriers (KEEP_OUTSIDE) gets every thread, one outside the frame owning nothing;
//               in the others such a thread just moves on.
// Then what the bodies do next: quad_ids (the four owner ids, strangers clamped to nobody), quad_bary (α, β and γ of the owned
// pixels) and quad_store_owned (whole quads, or the owned pixels only).
// CALLERS: k_shade_vis (pass_tiles with its kind filter, pass_tile, quad_ids), k_interp, k_interp_grad, k_interp_deriv (all of it),
// k_cube and k_cube_grad (the walk, quad_ids, quad_store_owned), k_cube_mip, k_cube_mip_grad and k_cube_level (the same, and
// quad_load), k_persp (the walk, quad_ids), k_persp_grad and
// k_interp_deriv_persp (all of it), k_light (the walk, quad_ids, quad_load, quad_store_owned) and k_light_grad (the same through
// pass_tiles and pass_tile: the tile's index names its row of partial sums), k_normal_map and k_normal_map_grad (as k_light), k_microfacet and k_microfacet_grad (as k_light and k_light_grad),
// k_reflect, k_reflect_grad, k_ibl and k_ibl_grad (as k_light), k_sh and k_sh_grad (as k_light and k_light_grad).
// Beyond tile_grid's cap (a workgroup's second trip round pass_tiles' loop, with what it carries) the callers are tested in
// tests/test_gpu_pass_walk.py (k_shade_vis, k_interp, k_interp_grad, k_interp_deriv, and the COPIES), in
// tests/test_gpu_pass_walk_lit.py (every other caller but the two below, and k_shadow and k_shadow_grad) and in
// tests/test_gpu_pass_walk_sh.py (k_sh, k_sh_grad).
// COPIES, each naming this definition — a fix to the walk goes into them too: k_gbuffer, k_motion, k_pos_grad, aa_body, k_tex,
// k_tex_grad, k_tex_mip, k_tex_mip_grad (with tex_quad and mip_quad).  Moved onto these helpers they computed the same words
// (the whole suite passed) but ran slower than their inline text on an MI355X at 256 frames of 1024²: k_gbuffer +4 %, k_motion +6 %,
// k_pos_grad +2..6 %, k_antialias +1.5..3 % (k_antialias_grad −15 %: one body serves both), k_tex_grad and k_tex_mip_grad +12 % on
// their guv legs — same arithmetic, another schedule; NOTEBOOK has the series.  They stay as they were until someone finds why.
// Left inline in the callers, because a helper would be no shorter than the statements: the per-kernel plane pointers (a.vis + f *
// a.vis_stride + poff: the strides' names and meanings differ between the Args structs); k_shade_vis's load of z, α, β into LDS
// (three planes by pixel, not two by owner) and its in-place write-out; the gout quads of k_interp_grad's chunk loop.
// ================================================================================================================
struct PassTile {
  const SRZ_CAS FrameDesc *fd;
  uint32_t f;    // the frame
  TileRect rc;
  int y, x4;     // the thread's row and first column (frame coordinates)
  bool inside;   // its first pixel lies in the tile's rectangle
  bool whole;    // inside, all four pixels, and the rows 16-byte aligned: one 16-byte access per plane
  size_t poff;   // floats from a frame's plane 0 to the thread's first pixel (any buffer of the set's geometry)
  float *out;    // the thread's first pixel in plane 0 of the frame in a.out
  // (something the body asks for: AntialiasArgs has no flags_or)
  __device__ __forceinline__ bool fused(uint32_t flags_or) const { return ((fd->flags | flags_or) & SRZ_FUSED_CLEAR) != 0; }
};
template <class A, class Body> __device__ __forceinline__ void pass_tiles(const A &a, Body body) {
  const uint32_t tpf = a.n_local_bands * a.tiles_x, n_items = a.n_frames * tpf;
  const uint32_t sub = blockIdx.x & 7u, step = gridDim.x >> 3;
  for (uint32_t j = blockIdx.x >> 3;; j += step) {
    uint32_t f, t;
    if (a.n_frames >= 8u) {
      f = sub + 8u * (j / tpf), t = j % tpf;
      if (f >= a.n_frames) break;
    } else {
      const uint32_t i = j * 8u + sub;
      if (i >= n_items) break;
      f = i / tpf, t = i % tpf;
    }
    body(f, t);
  }
}
template <class A> __device__ __forceinline__ PassTile pass_tile(const A &a, uint32_t f, uint32_t t) {
  const int ly = (int)threadIdx.x >> 3, lx4 = ((int)threadIdx.x & 7) * 4; // (wave * 8 + lane / 8, lane % 8 * 4)
  PassTile p;
  p.fd = as_const(a.frames) + f, p.f = f;
  const uint32_t lb = t / a.tiles_x, tx = t % a.tiles_x;
  p.rc = tile_rect(a, p.fd, f, lb, tx);
  const int W = p.fd->width;
  p.y = p.rc.ty0 + ly, p.x4 = p.rc.tx0 + lx4;
  p.inside = p.y <= p.rc.ty1 && p.x4 <= p.rc.tx1;
  p.whole = p.inside && (W & 3) == 0 && p.x4 + 3 <= p.rc.tx1;
  p.poff = (size_t)lb * BAND * (size_t)W + (size_t)ly * (size_t)W + (size_t)p.x4;
  p.out = p.rc.out0 + (size_t)ly * (size_t)W + (size_t)p.x4;
  return p;
}
template <bool KEEP_OUTSIDE, class A, class Body> __device__ __forceinline__ void pass_walk(const A &a, Body body) {
  pass_tiles(a, [&](uint32_t f, uint32_t t) {
    const PassTile p = pass_tile(a, f, t);
    if (KEEP_OUTSIDE || p.inside) body(p);
  });
}
// The four owner ids of the thread's quad (plane 1 of the frame's visibility buffer, gv its plane 0 at the thread's first pixel):
// index + 1 | S class.  0, the bare class bit (both wrap to 0xffffffff) and an index outside the frame's triangles are nobody: id 0.
// -> one bit per owned pixel.  KEEP: the bits of an owner's id the kernel wants (k_interp_deriv: not the class); stray: the pixels
// whose word is not 0 and names nobody (k_shade_vis gives them the clear values).  A thread outside the tile owns nothing.
template <uint32_t KEEP = 0xffffffffu>
__device__ __forceinline__ uint32_t quad_ids(const PassTile &t, const float *gv, uint32_t (&id)[4], uint32_t *stray = nullptr) {
  id[0] = id[1] = id[2] = id[3] = 0u;
  if (t.whole) {
    const uint4 q = *reinterpret_cast<const uint4 *>(gv + t.rc.plane);
    id[0] = q.x, id[1] = q.y, id[2] = q.z, id[3] = q.w;
  } else if (t.inside) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (t.x4 + k <= t.rc.tx1) id[k] = f2u(gv[t.rc.plane + k]);
  }
  const uint32_t n_tris = t.fd->n_tris;
  uint32_t own = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if ((id[k] & ~S_CLASS_BIT) - 1u < n_tris) {
      own |= 1u << k, id[k] &= KEEP;
    } else {
      if (stray && id[k] != 0u) *stray |= 1u << k;
      id[k] = 0u;
    }
  }
  return own;
}
// α and β (planes 2 and 3) of the quad's owned pixels, the others 0, and each owner's γ by its class (cover_s / cover_v)
__device__ __forceinline__ void quad_bary(const PassTile &t, const float *gv, uint32_t own, const uint32_t (&id)[4], float4 &al, float4 &be,
                                          float4 &ga) {
  al = be = ga = make_float4(0.f, 0.f, 0.f, 0.f);
  if (own == 0u) return;
  if (t.whole) {
    al = *reinterpret_cast<const float4 *>(gv + 2 * t.rc.plane), be = *reinterpret_cast<const float4 *>(gv + 3 * t.rc.plane);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (own & (1u << k)) quad_at(al, k) = gv[2 * t.rc.plane + k], quad_at(be, k) = gv[3 * t.rc.plane + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    quad_at(ga, k) = (id[k] & S_CLASS_BIT) ? 1.0f - quad_at(al, k) - quad_at(be, k) : 1.0f - (quad_at(al, k) + quad_at(be, k));
}
// N planes of the quad at p: whole quads with the fused clear or four owners (quad_store), else the owned pixels only
template <int N>
__device__ __forceinline__ void quad_store_owned(float *p, const PassTile &t, const float4 (&q)[N], bool fused, uint32_t own) {
  if (fused || own == 15u) {
    quad_store(p, t.rc.plane, q, t.whole, t.x4, t.rc.tx1);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (own & (1u << k))
#pragma unroll
        for (int i = 0; i < N; ++i) p[i * t.rc.plane + k] = quad_at(q[i], k);
  }
}

// ================================================================================================================
// k_shade_vis — the COLOUR OF A VISIBILITY BUFFER (srz_frameset_shade_visibility, include/srz.h): what k_shade would have written,
// from the owner id, z, α and β a visibility render left, without rasterising again.  The passes' walk (pass_tiles).  Per tile:
//   1. a thread's 4 owner ids in one 16-byte load (plane 1); an id above the frame's triangle count is nobody (with SRZ_FUSED_CLEAR it
//      gets the clear values, in place too); z, α, β only for quads with an owner, into LDS by pixel;
//   2. the owned pixels compacted by class (V entries, then S entries), as k_shade does, so a wave runs one class per 64-entry chunk;
//   3. per pixel: the owner's 60 bytes of normals and texture coordinates (no positions) + batch id, γ from α and β as the class
//      computes it, then shade_bary_v / _s — the same instantiations k_shade runs for the frame's build: the FAST variants picked by
//      one wave-uniform switch on the batch's shader type per pass, FastMath; a tile where an operand left FastMath's range is handed
//      to the generic build through redo_list (as k_shade's FAST builds do), which re-shades it with IEEE math — the generic build
//      re-shades its own such tiles at once; ApproxMath in the tolerance mode;
//   4. the four planes with 16-byte non-temporal stores (in place: the owned pixels' three colour planes only, and the clear values
//      where an out-of-range id meets SRZ_FUSED_CLEAR).
// One launch per build kind, as launch_shade: each instantiation keeps its own register count; tiles of other kinds' frames are
// skipped after one scalar load.  The floor is the memory system: 4 bytes of ids read per pixel, 12 more + 60 of triangle (+ a 2-byte
// batch id) per owned pixel, and 16 bytes written per pixel with SRZ_FUSED_CLEAR (per owned pixel without it, 12 in place).
// ================================================================================================================
// (4 waves per SIMD: 128 VGPRs; the four-light pow_fast build needs more — held to 128 it spills 136 bytes — and gets 3)
template <int FASTNL, bool BUMPY = false, bool APPROX = false>
__global__ __launch_bounds__(256, FASTNL == -4 ? 3 : SRZ_SHADE_MINW) void k_shade_vis(ShadeVisArgs a) {
  constexpr bool FAST = FASTNL != 0;
  static_assert(FAST || !BUMPY, "BUMPY is a property of the FAST builds");
  static_assert(!APPROX || (FASTNL > 0 && !BUMPY), "the tolerance mode has FAST builds for 1..4 lights only");
  constexpr uint32_t KIND = build_kind<FASTNL, BUMPY>();
  __shared__ __attribute__((aligned(16))) float s_in[3][TILE * TILE]; // z, α, β by pixel
  __shared__ __attribute__((aligned(16))) float s_c[3][TILE * TILE];  // colour by pixel
  __shared__ uint32_t s_idx[PIX_SLOT];                                // compacted owned pixels: owner's index in the frame
  __shared__ uint16_t s_pix[PIX_SLOT];                                // and pixel (ly * 32 + lx)
  __shared__ uint32_t s_wcnt[4];
  __shared__ uint32_t s_flag;
  __shared__ uint8_t s_bog[256]; // per thread: its pixels whose id word is out of range
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p0 = tid * 4; // (ly * TILE + lx4 of pass_tile's deal)
  const uint32_t tpf = a.n_local_bands * a.tiles_x;
  // ---- tile t of frame f.  mode: 0 = the FAST variants (a tile where an operand left FastMath's range goes to redo_list), 1 = the
  //      generic instantiation (FastMath, then IEEE if needed), 2 = IEEE at once (the tiles handed back) --------------------------------
  auto shade_tile = [&](const uint32_t f, const uint32_t t, auto mode_c) {
    constexpr int MODE = decltype(mode_c)::value;
    const PassTile pt = pass_tile(a, f, t);
    const SRZ_CAS FrameDesc *fd = pt.fd;
    const int tx0 = pt.rc.tx0, ty0 = pt.rc.ty0, tx1 = pt.rc.tx1, x4 = pt.x4;
    const bool in_tile = pt.inside, whole = pt.whole, fused = pt.fused(a.flags_or);
    const size_t plane = pt.rc.plane;
    const float *gv = a.vis + (size_t)f * a.frame_stride + pt.poff;
    float *go = pt.out;
    // ---- 1. owner ids, and z, α, β of owned quads
    uint32_t id[4], bogus = 0u; // bogus bit k: pixel k's id word is neither 0 nor a triangle of the frame
    // (what the write-out needs of the ids: one bit per pixel — the ids and the quads below are not kept alive across the passes)
    const uint32_t own = quad_ids(pt, gv, id, &bogus);
    s_bog[tid] = (uint8_t)bogus; // (read back by the in-place write-out only: no register holds it across the passes)
    const bool any_own = own != 0u;
    float4 in[3] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    if (any_own) {
      if (whole) {
        in[0] = *reinterpret_cast<const float4 *>(gv);
        in[1] = *reinterpret_cast<const float4 *>(gv + 2 * plane);
        in[2] = *reinterpret_cast<const float4 *>(gv + 3 * plane);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x4 + k <= tx1) quad_at(in[0], k) = gv[k], quad_at(in[1], k) = gv[2 * plane + k], quad_at(in[2], k) = gv[3 * plane + k];
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) *reinterpret_cast<float4 *>(&s_in[i][p0]) = in[i];
    // ---- 2. compaction by class (k_shade's: per-thread counts, one packed wave scan, the waves' totals through LDS)
    uint32_t cnt2 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt2 += id[k] == 0u ? 0u : ((id[k] & S_CLASS_BIT) ? 0x10000u : 1u);
    const uint32_t incl2 = wave_scan_add(cnt2);
    if (lane == 63) s_wcnt[wave] = incl2;
    if (tid == 0) s_flag = 0u;
    __syncthreads();
    uint32_t bV = 0, bS = 0, nV = 0, nS = 0;
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) {
      const uint32_t t2 = s_wcnt[w2];
      bV += w2 < wave ? (t2 & 0xffffu) : 0u, bS += w2 < wave ? (t2 >> 16) : 0u, nV += t2 & 0xffffu, nS += t2 >> 16;
    }
    nV = (uint32_t)__builtin_amdgcn_readfirstlane((int)nV), nS = (uint32_t)__builtin_amdgcn_readfirstlane((int)nS);
    {
      uint32_t oV = bV + ((incl2 - cnt2) & 0xffffu), oS = nV + bS + ((incl2 - cnt2) >> 16);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (id[k] == 0u) continue;
        const bool isS = (id[k] & S_CLASS_BIT) != 0u;
        const uint32_t o = isS ? oS++ : oV++;
        s_idx[o] = (id[k] & ~S_CLASS_BIT) - 1u, s_pix[o] = (uint16_t)(p0 + k);
      }
    }
    __syncthreads();
    // ---- 3. the shading passes over 64-entry chunks, dealt round-robin to the waves (S chunks first, as k_shade)
    if (nV + nS != 0u) { // workgroup-uniform
      const SRZ_CAS srz_tri *tris = as_const(a.tris) + fd->tri_off;
      const SRZ_CAS uint16_t *tri_batch = as_const(a.tri_batch) + fd->tri_off;
      const SRZ_CAS ShadeDescG *sdesc = as_const(a.sdesc) + fd->batch_off;
      const uint32_t cV = (nV + 63) >> 6, cS = (nS + 63) >> 6;
      // GEN: per-pixel generality (the generic build's instantiation: any shader, run-time light count, pow_cr)
      auto class_pass = [&](auto policy, auto is_v, auto gen_c) -> bool {
        using M = decltype(policy);
        constexpr bool isV = decltype(is_v)::value, GEN = decltype(gen_c)::value;
        bool bad = false;
        const FrameK K = frame_k(fd, as_const(a.lights));
        for (uint32_t c = (uint32_t)wave; c < cV + cS; c += 4) {
          if ((c >= cS) != isV) continue;
          const uint32_t i = (isV ? c - cS : c) * 64 + lane;
          if (i >= (isV ? nV : nS)) continue;
          const uint32_t slot = isV ? i : nV + i;
          const uint32_t idx = s_idx[slot], p = s_pix[slot];
          // the owner's normals and texture coordinates (floats 9..23 of its record) and its batch
          TriFetch tf;
          const SRZ_CAS f32x4 *tq = reinterpret_cast<const SRZ_CAS f32x4 *>(tris + idx);
          const F3 n0 = ld3(reinterpret_cast<const SRZ_CAS float *>(tq) + 9);
          tf.q2 = f32x4{0.f, n0.x, n0.y, n0.z}, tf.q3 = tq[3], tf.q4 = tq[4], tf.q5 = tq[5];
          tf.batch = tri_batch[idx];
          TriAttr at;
          unpack_attr(tf, at);
          const float zz = s_in[0][p], alpha = s_in[1][p], beta = s_in[2][p];
          const float gamma = isV ? 1.0f - (alpha + beta) : 1.0f - alpha - beta; // (cover_v / cover_s)
          const float fx = (float)(tx0 + (int)(p & 31u)), fy = (float)(ty0 + (int)(p >> 5));
          float r0 = 1.f, r1 = 2.f, r2 = 3.f;
          M m;
          ShadeDesc sd;
          if constexpr (!GEN) {
            // batch by batch, the batch's descriptor wave-uniform and one scalar switch on its shader type (inline copy of k_shade's, MODE 0)
            bool todo = true;
            for (unsigned long long tm = __ballot(true); tm != 0ull; tm = __ballot(todo)) {
              const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)tf.batch, __builtin_ctzll(tm));
              const SRZ_CAS ShadeDescG *g = sdesc + b0; // (uniform address: scalar loads)
              sd.shader = g->shader, sd.tw = g->tw, sd.th = g->th, sd.tex = as_const(g->tex);
              if (todo && tf.batch == b0) {
                auto run = [&](auto sh) {
                  if constexpr (isV)
                    shade_bary_v<M, decltype(sh)::value, FASTNL>(m, K, sd, at, alpha, beta, gamma, fx, fy, zz, r0, r1, r2);
                  else
                    shade_bary_s<M, decltype(sh)::value, FASTNL>(m, K, sd, at, alpha, beta, gamma, fx, fy, zz, r0, r1, r2);
                };
                const int sh0 = sd.shader; // wave-uniform
                if (sh0 == SRZ_SHADER_TEXTURE)
                  run(std::integral_constant<int, SRZ_SHADER_TEXTURE>{});
                else if (sh0 == SRZ_SHADER_PHONG)
                  run(std::integral_constant<int, SRZ_SHADER_PHONG>{});
                else if (!BUMPY || sh0 == SRZ_SHADER_NORMAL)
                  run(std::integral_constant<int, SRZ_SHADER_NORMAL>{});
                else if constexpr (BUMPY) {
                  if (sh0 == SRZ_SHADER_BUMP)
                    run(std::integral_constant<int, SRZ_SHADER_BUMP>{});
                  else
                    run(std::integral_constant<int, SRZ_SHADER_DISPLACEMENT>{});
                }
                todo = false;
              }
            }
          } else {
            const SRZ_CAS ShadeDescG *g = sdesc + tf.batch;
            sd.shader = g->shader, sd.tw = g->tw, sd.th = g->th, sd.tex = as_const(g->tex);
            if constexpr (isV)
              shade_bary_v<M, -1, 0>(m, K, sd, at, alpha, beta, gamma, fx, fy, zz, r0, r1, r2);
            else
              shade_bary_s<M, -1, 0>(m, K, sd, at, alpha, beta, gamma, fx, fy, zz, r0, r1, r2);
          }
          if constexpr (std::is_same<M, FastMath>::value) bad |= m.is_bad();
          s_c[0][p] = r0, s_c[1][p] = r1, s_c[2][p] = r2;
        }
        return bad;
      };
      auto dense_passes = [&](auto policy, auto gen_c) -> bool {
        const bool bv = class_pass(policy, std::true_type{}, gen_c);
        const bool bs = class_pass(policy, std::false_type{}, gen_c);
        return bv | bs;
      };
      if constexpr (APPROX) {
        dense_passes(ApproxMath{}, std::false_type{});
      } else if constexpr (MODE == 2) {
        dense_passes(IeeeMath{}, std::true_type{});
      } else {
        // FastMath first; a tile where an operand left its range is shaded again with the IEEE expansions by the generic build — the
        // FAST builds hand it back (as k_shade's do: the IEEE instantiation inside them would cost each its register budget)
        const bool bad = dense_passes(FastMath{}, std::integral_constant<bool, MODE == 1>{});
        if (__ballot(bad) != 0ull && lane == 0) s_flag = 1u;
        __syncthreads();
        if (s_flag) { // (workgroup-uniform)
          if constexpr (MODE == 0) {
            if (tid == 0) a.redo_list[atomicAdd(a.redo_count, 1u)] = f * tpf + t;
            __syncthreads();
            return; // (the generic build writes the whole tile)
          } else {
            dense_passes(IeeeMath{}, std::true_type{});
          }
        }
      }
      __syncthreads();
    }
    // ---- 4. write-out: owned pixels z + colour (in place: colour only), the others the clear values with SRZ_FUSED_CLEAR
    const uint32_t bog = (a.in_place && fused) ? (uint32_t)s_bog[tid] : 0u; // (in place, fused: out-of-range ids get the clear values)
    if (in_tile && (any_own || (fused && !a.in_place) || bog != 0u)) {
      const bool own4 = own == 15u;
      float4 q[4];
      q[0] = *reinterpret_cast<const float4 *>(&s_in[0][p0]);
#pragma unroll
      for (int i = 0; i < 3; ++i) q[i + 1] = *reinterpret_cast<const float4 *>(&s_c[i][p0]);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (!(own & (1u << k))) {
          quad_at(q[0], k) = __builtin_inff();
#pragma unroll
          for (int i = 1; i < 4; ++i) quad_at(q[i], k) = 0.f;
        }
      if (a.in_place) {
        if (own4) {
          const float4 c[3] = {q[1], q[2], q[3]};
          quad_store(go + plane, plane, c, whole, x4, tx1);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (own & (1u << k)) {
#pragma unroll
              for (int i = 1; i < 4; ++i) go[i * plane + k] = quad_at(q[i], k);
            } else if (bog & (1u << k)) { // (an out-of-range id: nobody, whose words are not the clear values yet)
#pragma unroll
              for (int i = 0; i < 4; ++i) go[i * plane + k] = quad_at(q[i], k);
            }
          }
        }
      } else if (fused || own4) {
        quad_store(go, plane, q, whole, x4, tx1);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (own & (1u << k))
#pragma unroll
            for (int i = 0; i < 4; ++i) go[i * plane + k] = quad_at(q[i], k);
      }
    }
    __syncthreads(); // LDS is reused by the next tile
  };

  // the frames of this build's kind, tile by tile
  if (FAST || a.any_generic)
    pass_tiles(a, [&](uint32_t f, uint32_t t) {
      if (frame_kind(as_const(a.frames)[f].flags) != KIND) return; // (workgroup-uniform: another launch's frame)
      shade_tile(f, t, std::integral_constant<int, FAST ? 0 : 1>{});
    });
  if constexpr (!FAST) { // the tiles the FAST builds handed back (they ran before this kernel on the same stream)
    const uint32_t n_redo = *as_const(a.redo_count);
    for (uint32_t i = blockIdx.x; i < n_redo; i += gridDim.x) {
      const uint32_t it = as_const(a.redo_list)[i];
      shade_tile(it / tpf, it % tpf, std::integral_constant<int, 2>{});
    }
  }
}

// ================================================================================================================
// k_gbuffer — the G-BUFFER OF A VISIBILITY BUFFER (srz_frameset_gbuffer, include/srz.h): the attributes the built-in shaders are handed
// for each pixel's owner — shade_bary_v / _s up to the call of v_shade / s_shade, v_shade's prologue and fetch, s_texel — as planes.
// No work lists and no LDS: the grid walks every (frame, 32x32 tile) in k_shade_vis's XCD order, a thread owns 4 consecutive pixels of
// one row (k_visibility's deal), so every plane leaves as 16-byte non-temporal stores straight from registers.  Per thread: its 4 ids in
// one 16-byte load; α and β only for a quad with an owner; per owned pixel the owner's normals and / or texture coordinates (floats
// 9..23 of its record, never the positions) and its batch id, gathered; the texel only where ALBEDO asks for it.  Both classes share a
// wave: a pixel's arithmetic is tens of operations, computed per lane by class, always with IeeeMath (no flag-and-redo).  `what` is
// wave-uniform: one branch per group.  The floor is the memory system: 4 bytes of id per pixel, 8 of α and β + 62 of gather per owned
// pixel, 4 written per requested plane and pixel.
// ================================================================================================================
typedef float f32x2 __attribute__((ext_vector_type(2)));
struct GbufPixel {
  float n[3], uv[2], kd[3];
  uint32_t batch1;
};
__device__ __forceinline__ GbufPixel gbuf_pixel(uint32_t what, uint32_t id, float alpha, float beta, const SRZ_CAS srz_tri *tris,
                                                const SRZ_CAS uint16_t *tri_batch, const SRZ_CAS ShadeDescG *sdesc) {
  GbufPixel o = {{0.f, 0.f, 0.f}, {0.f, 0.f}, {1.f, 1.f, 1.f}, 0u};
  IeeeMath m;
  const bool isS = (id & S_CLASS_BIT) != 0u;
  const uint32_t idx = (id & ~S_CLASS_BIT) - 1u;
  const SRZ_CAS float *rec = reinterpret_cast<const SRZ_CAS float *>(tris + idx);
  const float gamma = isS ? 1.0f - alpha - beta : 1.0f - (alpha + beta); // (cover_s / cover_v)
  if (what & SRZ_GB_NORMAL) {
    const F3 n0 = ld3(rec + 9), n1 = ld3(rec + 12), n2 = ld3(rec + 15);
    float nx, ny, nz;
    if (isS) {
      nx = alpha * n0.x + beta * n1.x + gamma * n2.x;
      ny = alpha * n0.y + beta * n1.y + gamma * n2.y;
      nz = alpha * n0.z + beta * n1.z + gamma * n2.z;
      normalize3(m, nx, ny, nz);
    } else {
      nx = fmaf_(alpha, n0.x, fmaf_(beta, n1.x, gamma * n2.x));
      ny = fmaf_(alpha, n0.y, fmaf_(beta, n1.y, gamma * n2.y));
      nz = fmaf_(alpha, n0.z, fmaf_(beta, n1.z, gamma * n2.z));
      v_normalized(m, nx, ny, nz);
    }
    o.n[0] = nx, o.n[1] = ny, o.n[2] = nz;
  }
  if (what & (SRZ_GB_BATCH | SRZ_GB_ALBEDO)) o.batch1 = (uint32_t)tri_batch[idx] + 1u;
  if (what & (SRZ_GB_UV | SRZ_GB_ALBEDO)) {
    const f32x2 t0 = *reinterpret_cast<const SRZ_CAS f32x2 *>(rec + 18); // u0 v0
    const f32x4 t12 = *reinterpret_cast<const SRZ_CAS f32x4 *>(rec + 20); // u1 v1 u2 v2
    float u, v;
    if (isS) {
      u = alpha * t0.x + beta * t12.x + gamma * t12.z;
      v = alpha * t0.y + beta * t12.y + gamma * t12.w;
    } else {
      u = fmaf_(alpha, t0.x, fmaf_(beta, t12.x, gamma * t12.z));
      v = fmaf_(alpha, t0.y, fmaf_(beta, t12.y, gamma * t12.w));
    }
    o.uv[0] = u, o.uv[1] = v;
    if (what & SRZ_GB_ALBEDO) {
      const SRZ_CAS ShadeDescG *g = sdesc + (o.batch1 - 1u);
      ShadeDesc sd;
      sd.shader = g->shader, sd.tw = g->tw, sd.th = g->th, sd.tex = as_const(g->tex);
      if (isS) { // s_shade: every textured type fetches kd through getTextureColor(vec2)
        if (sd.shader == SRZ_SHADER_TEXTURE || sd.shader == SRZ_SHADER_BUMP || sd.shader == SRZ_SHADER_DISPLACEMENT)
          s_texel(m, sd, u, v, o.kd[0], o.kd[1], o.kd[2]);
      } else if (sd.shader == SRZ_SHADER_TEXTURE) { // v_shade's prologue and fetch (inline copy: it has no helper of its own)
        const float tw = (float)sd.tw, th = (float)sd.th;
        u = u * tw, v = v * th;
        u = sse_max(0.0f, sse_min(u, tw - 1.0f));
        v = sse_max(0.0f, sse_min(v, th - 1.0f));
        const int32_t xi = cvt_rne_i32(u), yi = cvt_rne_i32(v);
        const uint32_t texel = sd.tex[(size_t)yi * sd.tw + xi];
        const float inv255 = 1.0f / 255.0f;
        o.kd[0] = (float)(texel & 0xffu) * inv255, o.kd[1] = (float)((texel >> 8) & 0xffu) * inv255, o.kd[2] = (float)((texel >> 16) & 0xffu) * inv255;
      }
    }
  }
  return o;
}
__global__ __launch_bounds__(256) void k_gbuffer(GbufArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ly = wave * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
  const uint32_t tpf = a.n_local_bands * a.tiles_x, n_items = a.n_frames * tpf;
  const uint32_t what = a.what;
  // workgroup b walks the frames f ≡ b mod 8 tile by tile (fewer than 8 frames: every 8th tile): an inline copy of pass_walk
  const uint32_t sub = blockIdx.x & 7u, step = gridDim.x >> 3;
  for (uint32_t j = blockIdx.x >> 3;; j += step) {
    uint32_t f, t;
    if (a.n_frames >= 8u) {
      f = sub + 8u * (j / tpf), t = j % tpf;
      if (f >= a.n_frames) break;
    } else {
      const uint32_t i = j * 8u + sub;
      if (i >= n_items) break;
      f = i / tpf, t = i % tpf;
    }
    const SRZ_CAS FrameDesc *fd = as_const(a.frames) + f;
    const uint32_t lb = t / a.tiles_x, tx = t % a.tiles_x;
    const TileRect rc = tile_rect(a, fd, f, lb, tx);
    const int W = fd->width;
    const int y = rc.ty0 + ly, x4 = rc.tx0 + lx4;
    if (!(y <= rc.ty1 && x4 <= rc.tx1)) continue; // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool whole = (W & 3) == 0 && x4 + 3 <= rc.tx1;
    const bool fused = ((fd->flags | a.flags_or) & SRZ_FUSED_CLEAR) != 0;
    const size_t poff = (size_t)lb * BAND * (size_t)W + (size_t)ly * (size_t)W + (size_t)x4;
    const float *gv = a.vis + (size_t)f * a.vis_stride + poff; // plane 0 (z: never read)
    float *go = rc.out0 + (size_t)ly * (size_t)W + (size_t)x4;
    // ---- 1. owner ids (index + 1 | S class; 0 or an index outside the frame's triangles: nobody)
    uint32_t id[4] = {0u, 0u, 0u, 0u};
    if (whole) {
      const uint4 q = *reinterpret_cast<const uint4 *>(gv + rc.plane);
      id[0] = q.x, id[1] = q.y, id[2] = q.z, id[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x4 + k <= rc.tx1) id[k] = f2u(gv[rc.plane + k]);
    }
    const uint32_t n_tris = fd->n_tris;
    uint32_t own = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if ((id[k] & ~S_CLASS_BIT) - 1u >= n_tris) id[k] = 0u; // (0 and the bare class bit wrap to 0xffffffff)
      own |= id[k] != 0u ? 1u << k : 0u;
    }
    if (own == 0u && !fused) continue;
    // ---- 2. α, β of a quad with an owner; the owners' attributes
    float4 al = make_float4(0.f, 0.f, 0.f, 0.f), be = al;
    if (own != 0u) {
      if (whole) {
        al = *reinterpret_cast<const float4 *>(gv + 2 * rc.plane), be = *reinterpret_cast<const float4 *>(gv + 3 * rc.plane);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x4 + k <= rc.tx1) quad_at(al, k) = gv[2 * rc.plane + k], quad_at(be, k) = gv[3 * rc.plane + k];
      }
    }
    const SRZ_CAS srz_tri *tris = as_const(a.tris) + fd->tri_off;
    const SRZ_CAS uint16_t *tri_batch = as_const(a.tri_batch) + fd->tri_off;
    const SRZ_CAS ShadeDescG *sdesc = as_const(a.sdesc) + fd->batch_off;
    float4 qn[3], quv[2], qb[1], qk[3]; // nobody: zeros
#pragma unroll
    for (int i = 0; i < 3; ++i) qn[i] = qk[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    quv[0] = quv[1] = qb[0] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (id[k] == 0u) continue;
      const GbufPixel px = gbuf_pixel(what, id[k], quad_at(al, k), quad_at(be, k), tris, tri_batch, sdesc);
#pragma unroll
      for (int i = 0; i < 3; ++i) quad_at(qn[i], k) = px.n[i], quad_at(qk[i], k) = px.kd[i];
      quad_at(quv[0], k) = px.uv[0], quad_at(quv[1], k) = px.uv[1], quad_at(qb[0], k) = u2f_(px.batch1);
    }
    // ---- 3. the requested planes, group after group: whole quads (fused clear, or four owners), else the owned pixels only
    const bool quads = fused || own == 15u;
    auto put = [&](float *p, const auto &q) {
      constexpr int N = (int)(sizeof(q) / sizeof(float4));
      if (quads) {
        quad_store(p, rc.plane, q, whole, x4, rc.tx1);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (own & (1u << k))
#pragma unroll
            for (int i = 0; i < N; ++i) p[i * rc.plane + k] = quad_at(q[i], k);
      }
    };
    if (what & SRZ_GB_NORMAL) put(go, qn), go += 3 * rc.plane;
    if (what & SRZ_GB_UV) put(go, quv), go += 2 * rc.plane;
    if (what & SRZ_GB_BATCH) put(go, qb), go += rc.plane;
    if (what & SRZ_GB_ALBEDO) put(go, qk);
  }
}

// ================================================================================================================
// k_motion — THE MOTION PASS (srz_frameset_motion, include/srz.h): where the surface point under each pixel of frame f lies in
// frame g = f + delta of the same set, whose triangle t is frame f's triangle t.  The point is the owner's three positions IN FRAME g
// under the pixel's α, β, γ, each component interpolated as the owner's class interpolates z (cover_v: fma chain; cover_s: products
// and sums); FLOW is its x, y minus the pixel's, DEPTH its z, TARGET the raw id and z words of frame g's visibility buffer at the
// nearest sample (round half even; outside the frame, NaN included: id 0, z +inf — decided in float, before any index exists).
// k_gbuffer's shape: no work lists, no LDS, no barrier; the grid walks every (frame, 32x32 tile) in k_shade_vis's XCD order, a thread
// owns 4 consecutive pixels of one row, its 4 ids arrive in one 16-byte load, α and β only for a quad with an owner, per owned pixel
// one gather of 36 bytes (load_pos9) and, with TARGET, two dependent 4-byte loads; every plane leaves through quad_store.  `what` is
// wave-uniform: one branch per group.  Always the exact arithmetic.  A frame whose g lies outside the set has no owner anywhere.
// The floor is the memory system: 4 bytes of id per pixel; 8 of α and β, 36 of gather and (TARGET) 8 more per owned pixel; 4 written
// per requested plane and pixel.
// ================================================================================================================
struct MotionPixel {
  float dx, dy, z, tz;
  uint32_t tid;
};
__device__ __forceinline__ MotionPixel motion_pixel(uint32_t what, uint32_t id, float alpha, float beta, int x, int y, const SRZ_CAS float *tpos,
                                                    uint32_t pos_stride, const float *vis_g, size_t plane, int W, int H) {
  MotionPixel o = {0.f, 0.f, 0.f, __builtin_inff(), 0u};
  const bool isS = (id & S_CLASS_BIT) != 0u;
  const uint32_t idx = (id & ~S_CLASS_BIT) - 1u;
  float P[9]; // ax ay z0 bx by z1 cx cy z2 of the owner in frame g
  load_pos9(tpos + (size_t)idx * pos_stride, P);
  float xp, yp, zp;
  if (isS) { // (cover_s)
    const float gamma = 1.0f - alpha - beta;
    xp = alpha * P[0] + beta * P[3] + gamma * P[6];
    yp = alpha * P[1] + beta * P[4] + gamma * P[7];
    zp = alpha * P[2] + beta * P[5] + gamma * P[8];
  } else { // (cover_v)
    const float gamma = 1.0f - (alpha + beta);
    xp = fmaf_(alpha, P[0], fmaf_(beta, P[3], gamma * P[6]));
    yp = fmaf_(alpha, P[1], fmaf_(beta, P[4], gamma * P[7]));
    zp = fmaf_(alpha, P[2], fmaf_(beta, P[5], gamma * P[8]));
  }
  o.dx = xp - (float)x, o.dy = yp - (float)y, o.z = zp;
  if (what & SRZ_MV_TARGET) {
    const float tx = __builtin_rintf(xp), ty = __builtin_rintf(yp);
    // compared as floats: a NaN or a huge coordinate is outside and never becomes an index
    if (tx >= 0.0f && tx <= (float)(W - 1) && ty >= 0.0f && ty <= (float)(H - 1)) {
      const float *q = vis_g + (size_t)(int)ty * (size_t)W + (size_t)(int)tx;
      o.tid = f2u(q[plane]), o.tz = q[0];
    }
  }
  return o;
}
__global__ __launch_bounds__(256) void k_motion(MotionArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ly = wave * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
  const uint32_t tpf = a.n_local_bands * a.tiles_x, n_items = a.n_frames * tpf;
  const uint32_t what = a.what;
  // workgroup b walks the frames f ≡ b mod 8 tile by tile (fewer than 8 frames: every 8th tile): an inline copy of pass_walk
  const uint32_t sub = blockIdx.x & 7u, step = gridDim.x >> 3;
  for (uint32_t j = blockIdx.x >> 3;; j += step) {
    uint32_t f, t;
    if (a.n_frames >= 8u) {
      f = sub + 8u * (j / tpf), t = j % tpf;
      if (f >= a.n_frames) break;
    } else {
      const uint32_t i = j * 8u + sub;
      if (i >= n_items) break;
      f = i / tpf, t = i % tpf;
    }
    const SRZ_CAS FrameDesc *fd = as_const(a.frames) + f;
    const uint32_t lb = t / a.tiles_x, tx = t % a.tiles_x;
    const TileRect rc = tile_rect(a, fd, f, lb, tx);
    const int W = fd->width, H = fd->height;
    const int y = rc.ty0 + ly, x4 = rc.tx0 + lx4;
    if (!(y <= rc.ty1 && x4 <= rc.tx1)) continue; // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool whole = (W & 3) == 0 && x4 + 3 <= rc.tx1;
    const bool fused = ((fd->flags | a.flags_or) & SRZ_FUSED_CLEAR) != 0;
    const int g = (int)f + a.delta; // the target frame; outside the set: nobody owns a pixel of frame f
    const bool has_g = g >= 0 && g < (int)a.n_frames;
    if (!has_g && !fused) continue;
    const size_t poff = (size_t)lb * BAND * (size_t)W + (size_t)ly * (size_t)W + (size_t)x4;
    const float *gv = a.vis + (size_t)f * a.vis_stride + poff; // plane 0 (z: never read)
    float *go = rc.out0 + (size_t)ly * (size_t)W + (size_t)x4;
    // ---- 1. owner ids (index + 1 | S class; 0 or an index outside the frame's triangles: nobody)
    uint32_t id[4] = {0u, 0u, 0u, 0u};
    if (has_g) {
      if (whole) {
        const uint4 q = *reinterpret_cast<const uint4 *>(gv + rc.plane);
        id[0] = q.x, id[1] = q.y, id[2] = q.z, id[3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x4 + k <= rc.tx1) id[k] = f2u(gv[rc.plane + k]);
      }
    }
    const uint32_t n_tris = fd->n_tris;
    uint32_t own = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if ((id[k] & ~S_CLASS_BIT) - 1u >= n_tris) id[k] = 0u; // (0 and the bare class bit wrap to 0xffffffff)
      own |= id[k] != 0u ? 1u << k : 0u;
    }
    if (own == 0u && !fused) continue;
    // ---- 2. α, β of a quad with an owner; the owners' positions in frame g and, with TARGET, frame g's words at the nearest sample
    float4 al = make_float4(0.f, 0.f, 0.f, 0.f), be = al;
    float4 qf[2], qd[1], qt[2]; // nobody: zeros
    qf[0] = qf[1] = qd[0] = qt[0] = qt[1] = al;
    if (own != 0u) {
      if (whole) {
        al = *reinterpret_cast<const float4 *>(gv + 2 * rc.plane), be = *reinterpret_cast<const float4 *>(gv + 3 * rc.plane);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x4 + k <= rc.tx1) quad_at(al, k) = gv[2 * rc.plane + k], quad_at(be, k) = gv[3 * rc.plane + k];
      }
      const SRZ_CAS FrameDesc *fg = as_const(a.frames) + g;
      const SRZ_CAS float *tpos = as_const(a.tri_pos) + (size_t)fg->tri_off * a.pos_stride;
      const float *vis_g = a.vis + (size_t)g * a.vis_stride; // (TARGET: shard_world == 1, a local row is the frame's row)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (id[k] == 0u) continue;
        const MotionPixel px = motion_pixel(what, id[k], quad_at(al, k), quad_at(be, k), x4 + k, y, tpos, a.pos_stride, vis_g, rc.plane, W, H);
        quad_at(qf[0], k) = px.dx, quad_at(qf[1], k) = px.dy, quad_at(qd[0], k) = px.z;
        quad_at(qt[0], k) = u2f(px.tid), quad_at(qt[1], k) = px.tz;
      }
    }
    // ---- 3. the requested planes, group after group: whole quads (fused clear, or four owners), else the owned pixels only
    const bool quads = fused || own == 15u;
    auto put = [&](float *p, const auto &q) {
      constexpr int N = (int)(sizeof(q) / sizeof(float4));
      if (quads) {
        quad_store(p, rc.plane, q, whole, x4, rc.tx1);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (own & (1u << k))
#pragma unroll
            for (int i = 0; i < N; ++i) p[i * rc.plane + k] = quad_at(q[i], k);
      }
    };
    if (what & SRZ_MV_FLOW) put(go, qf), go += 2 * rc.plane;
    if (what & SRZ_MV_DEPTH) put(go, qd), go += rc.plane;
    if (what & SRZ_MV_TARGET) put(go, qt);
  }
}

// ================================================================================================================
// k_interp — CALLER ATTRIBUTES OVER A VISIBILITY BUFFER (srz_frameset_interpolate, include/srz.h): channel ch of the owner's three
// corner values [triangle][corner][channel] under the pixel's α, β, γ, interpolated as the owner's class interpolates uv
// (shade_bary_v: fma chain; shade_bary_s: products and sums).  k_gbuffer's shape: pass_walk, no LDS, no barrier; quad_ids, quad_bary,
// every plane leaves through quad_store_owned.  The ids, α, β and γ are loaded and formed once; a wave-uniform loop then runs over the channels in register chunks of ATTR_CHUNK, the tail chunk masked, so that 64
// channels cost the registers of 4.  The attribute array is only 4-byte aligned: 3 dwords per owned pixel and channel, gathered.
// The floor is the memory system: 4 bytes of id per pixel; 8 of α and β and 12 n_ch of gather per owned pixel; 4 n_ch written per
// pixel.
// ================================================================================================================
constexpr uint32_t ATTR_CHUNK = 4;
__device__ __forceinline__ float interp_ch(bool isS, float alpha, float beta, float gamma, float a, float b, float c) {
  return isS ? alpha * a + beta * b + gamma * c             // (shade_bary_s)
             : fmaf_(alpha, a, fmaf_(beta, b, gamma * c));  // (shade_bary_v)
}
__global__ __launch_bounds__(256) void k_interp(InterpArgs a) {
  const uint32_t C = a.n_ch;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const TileRect &rc = t.rc;
    const bool fused = t.fused(a.flags_or);
    const float *gv = a.vis + (size_t)t.f * a.vis_stride + t.poff; // plane 0 (z: never read)
    float *go = t.out;
    // ---- 1. owner ids
    uint32_t id[4];
    const uint32_t own = quad_ids(t, gv, id);
    if (own == 0u && !fused) return;
    // ---- 2. α, β of a quad with an owner, each owner's γ by its class
    float4 al, be, ga;
    quad_bary(t, gv, own, id, al, be, ga);
    const SRZ_CAS float *at = as_const(a.attr) + (size_t)t.f * a.attr_frame_stride;
    // ---- 3. the channels, ATTR_CHUNK at a time
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 q[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) q[i] = make_float4(0.f, 0.f, 0.f, 0.f); // nobody: zeros
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (id[k] == 0u) continue;
        const SRZ_CAS float *p = at + (size_t)((id[k] & ~S_CLASS_BIT) - 1u) * (3u * C) + c0;
        const bool isS = (id[k] & S_CLASS_BIT) != 0u;
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
          if (i < nc) quad_at(q[i], k) = interp_ch(isS, quad_at(al, k), quad_at(be, k), quad_at(ga, k), p[i], p[C + i], p[2u * C + i]);
      }
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
        if (i >= nc) break;
        quad_store_owned(go + (size_t)(c0 + i) * rc.plane, t, {q[i]}, fused, own);
      }
    }
  });
}

// ================================================================================================================
// k_interp_grad — THE BACKWARD OF k_interp (srz_frameset_interpolate_grad): per owned pixel and channel, w[corner] * gout added into
// the attribute gradient of the owner (gattr), and the gradient with respect to α and β (gbary: fma chain over the channels, from
// registers, no atomics).  The same walk and the same loads as k_interp, plus gout's quads, chunk by chunk.
// One global float atomic per (pixel, corner, channel) would be several times the forward pass's bytes at the ≈1.3 TB/s the chip adds
// at, and collapses further when the adds of a wave scatter; neighbouring pixels share owners, so the sums are combined before they
// leave the CU:
//   1. a thread adds up its quad, run of equal owner by run (one run almost always);
//   2. the quads of one owner that are neighbours in a tile row (8 lanes) are added up by a segmented scan on DPP row shifts; the
//      last lane of each run holds its sum;
//   3. that sum goes into the tile's table of distinct owners in LDS (open addressing on the triangle index, IG_PROBES probes, LDS
//      float adds, 3 * ATTR_CHUNK floats per slot); an owner that finds no slot adds straight to memory — correct, only slower;
//   4. after a barrier the table is flushed: the used slots are listed, so consecutive lanes add consecutive (corner, channel)
//      floats of one triangle, triangle after triangle, with global_atomic_add_f32.
// Global adds are thus per (tile, distinct owner, corner, channel).  The table's keys live for the whole tile, its values for one chunk.
// Every thread of the workgroup reaches every barrier: a thread outside the frame owns nothing instead of moving on.
// ================================================================================================================
constexpr uint32_t IG_SLOT_BITS = 7, IG_SLOTS = 1u << IG_SLOT_BITS, IG_PROBES = 4, IG_VALS = 3 * ATTR_CHUNK;
struct InterpTable {
  uint32_t key[IG_SLOTS];  // triangle index + 1; 0: free
  uint32_t used[IG_SLOTS]; // the slots taken, in arrival order
  uint32_t n_used;
  float val[IG_SLOTS * IG_VALS]; // [slot][corner][channel of the chunk]
};
// (no-return hardware add; the memory is the caller's ordinary device memory, include/srz.h says so)
__device__ __forceinline__ void global_add(float *p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ float quad_pick(const float4 &v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; } // (k: a variable)
template <int CTRL> __device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false); // (a lane without a source in its row: 0)
}
constexpr int DPP_ROW_SHL1 = 0x101, DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114;
template <int CTRL> __device__ __forceinline__ void ig_scan_step(float (&acc)[IG_VALS], uint32_t &stop) {
  const uint32_t up_stop = dpp_u32<CTRL>(stop);
#pragma unroll
  for (uint32_t e = 0; e < IG_VALS; ++e) {
    const float up = u2f(dpp_u32<CTRL>(f2u(acc[e])));
    if (!stop) acc[e] += up;
  }
  stop |= up_stop;
}
__device__ __forceinline__ void ig_emit(InterpTable &tb, uint32_t key, const float (&acc)[IG_VALS], uint32_t nc, float *gattr, uint32_t C,
                                        uint32_t c0) {
  uint32_t h = (key * 0x9e3779b1u) >> (32u - IG_SLOT_BITS);
  bool found = false;
  for (uint32_t p = 0; p < IG_PROBES && !found; ++p) {
    const uint32_t old = atomicCAS(&tb.key[h], 0u, key);
    if (old == 0u) tb.used[atomicAdd(&tb.n_used, 1u)] = h; // (each slot is taken once: n_used <= IG_SLOTS)
    found = old == 0u || old == key;
    if (!found) h = (h + 1u) & (IG_SLOTS - 1u);
  }
  if (found) {
#pragma unroll
    for (uint32_t e = 0; e < IG_VALS; ++e)
      if ((e % ATTR_CHUNK) < nc) atomicAdd(&tb.val[h * IG_VALS + e], acc[e]);
  } else {
    float *g = gattr + (size_t)(key - 1u) * (3u * C) + c0;
#pragma unroll
    for (uint32_t e = 0; e < IG_VALS; ++e)
      if ((e % ATTR_CHUNK) < nc) global_add(g + (e / ATTR_CHUNK) * C + (e % ATTR_CHUNK), acc[e]);
  }
}
__global__ __launch_bounds__(256) void k_interp_grad(InterpArgs a) {
  __shared__ InterpTable tb;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t C = a.n_ch;
  const bool want_attr = a.gattr != nullptr, want_bary = a.out != nullptr;
  if (want_attr) {
    for (uint32_t i = tid; i < IG_SLOTS; i += 256) tb.key[i] = 0u;
    for (uint32_t i = tid; i < IG_SLOTS * IG_VALS; i += 256) tb.val[i] = 0.0f;
    if (tid == 0) tb.n_used = 0u;
    __syncthreads();
  }
  pass_walk<true>(a, [&](const PassTile &t) { // (a thread outside the frame owns nothing, and still meets the barriers)
    const TileRect &rc = t.rc;
    const bool whole = t.whole;
    const float *gv = a.vis + (size_t)t.f * a.vis_stride + t.poff; // plane 0 (z: never read)
    const float *gg = a.gout + (size_t)t.f * a.gout_stride + t.poff;
    // ---- 1. owner ids
    uint32_t id[4], first = 0u;
    const uint32_t own = quad_ids(t, gv, id);
    bool one_owner = true; // every owned pixel of the quad has the same triangle (either class)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (id[k] == 0u) continue;
      const uint32_t key = id[k] & ~S_CLASS_BIT;
      one_owner = one_owner && (first == 0u || first == key);
      first = first == 0u ? key : first;
    }
    // ---- 2. α, β of a quad with an owner, each owner's γ by its class
    float4 al, be, ga;
    quad_bary(t, gv, own, id, al, be, ga);
    const SRZ_CAS float *at = as_const(a.attr) + (size_t)t.f * a.attr_frame_stride;
    float *gat = a.gattr + (size_t)t.f * a.attr_frame_stride;
    // the key a quad of one owner takes into the row's scan; 0: the quad emits its runs itself, or has none
    const uint32_t skey = want_attr && own != 0u && one_owner ? first : 0u;
    const bool scan = want_attr && __builtin_amdgcn_ballot_w64(skey != 0u) != 0ull; // (wave-uniform)
    const uint32_t pos = (uint32_t)lane & 7u;
    // (every lane executes both shifts: a lane that skipped one behind a short-circuit would be missing as its neighbour's source)
    const uint32_t key_left = dpp_u32<DPP_ROW_SHR1>(skey), key_right = dpp_u32<DPP_ROW_SHL1>(skey);
    const bool seg_head = (pos == 0u) | (key_left != skey) | (skey == 0u); // (a quad without a key takes no carry)
    const bool seg_last = (pos == 7u) | (key_right != skey);
    float4 da = make_float4(0.f, 0.f, 0.f, 0.f), db = da;
    uint32_t n_used = 0u;
    // ---- 3. the channels, ATTR_CHUNK at a time
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 g[ATTR_CHUNK]; // gout of the chunk's channels; words of nobody's pixels are loaded with their quad at most, never used
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (own != 0u) {
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
          if (i >= nc) break;
          const float *p = gg + (size_t)(c0 + i) * rc.plane;
          if (whole) {
            g[i] = *reinterpret_cast<const float4 *>(p);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (own & (1u << k)) quad_at(g[i], k) = p[k];
          }
        }
      }
      float acc[IG_VALS];
#pragma unroll
      for (uint32_t e = 0; e < IG_VALS; ++e) acc[e] = 0.0f;
      if (want_bary) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (id[k] == 0u) continue;
          const SRZ_CAS float *p = at + (size_t)((id[k] & ~S_CLASS_BIT) - 1u) * (3u * C) + c0;
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) {
              const float gi = quad_at(g[i], k), c = p[2u * C + i];
              quad_at(da, k) = fmaf_(gi, p[i] - c, quad_at(da, k)), quad_at(db, k) = fmaf_(gi, p[C + i] - c, quad_at(db, k));
            }
        }
      }
      if (want_attr) {
        uint32_t cur = 0u; // the open run's key
        if (skey != 0u) { // one owner: the quad is one run, summed from the registers as they stand
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (id[k] != 0u)
#pragma unroll
              for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
                if (i < nc) {
                  const float gi = quad_at(g[i], k);
                  acc[i] += quad_at(al, k) * gi, acc[ATTR_CHUNK + i] += quad_at(be, k) * gi, acc[2 * ATTR_CHUNK + i] += quad_at(ga, k) * gi;
                }
        } else if (own != 0u) { // several owners (an edge crosses the quad): pixel after pixel, a run that ends goes into the table
#pragma nounroll
          for (int k = 0; k < 4; ++k) {
            const uint32_t idk = k == 0 ? id[0] : k == 1 ? id[1] : k == 2 ? id[2] : id[3];
            if (idk == 0u) continue;
            const uint32_t key = idk & ~S_CLASS_BIT;
            if (cur != 0u && key != cur) {
              ig_emit(tb, cur, acc, nc, gat, C, c0);
#pragma unroll
              for (uint32_t e = 0; e < IG_VALS; ++e) acc[e] = 0.0f;
            }
            cur = key;
            const float wa = quad_pick(al, k), wb = quad_pick(be, k), wc = quad_pick(ga, k);
#pragma unroll
            for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
              if (i < nc) {
                const float gi = quad_pick(g[i], k);
                acc[i] += wa * gi, acc[ATTR_CHUNK + i] += wb * gi, acc[2 * ATTR_CHUNK + i] += wc * gi;
              }
          }
        }
        if (scan) { // inclusive segmented scan over the 8 quads of the tile row (Hillis-Steele: a lane past a head takes no carry)
          uint32_t stop = seg_head ? 1u : 0u; // (position p < d has stop set before the step of distance d: position 0 is a head)
          ig_scan_step<DPP_ROW_SHR1>(acc, stop);
          ig_scan_step<DPP_ROW_SHR2>(acc, stop);
          ig_scan_step<DPP_ROW_SHR4>(acc, stop);
        }
        // the last quad of a row's run holds the run's sum; a quad of several owners (a head: the scan left it alone) its last run
        const uint32_t ekey = skey != 0u ? (seg_last ? skey : 0u) : cur;
        if (ekey != 0u) ig_emit(tb, ekey, acc, nc, gat, C, c0);
        // ---- 4. the table's values of this chunk into memory: lanes in (corner, channel) order within a triangle
        __syncthreads();
        n_used = tb.n_used;
        for (uint32_t i = tid; i < n_used * IG_VALS; i += 256) {
          const uint32_t s = tb.used[i / IG_VALS], e = i % IG_VALS;
          const float v = tb.val[s * IG_VALS + e];
          tb.val[s * IG_VALS + e] = 0.0f;
          if ((e % ATTR_CHUNK) < nc) global_add(gat + (size_t)(tb.key[s] - 1u) * (3u * C) + (e / ATTR_CHUNK) * C + c0 + (e % ATTR_CHUNK), v);
        }
        __syncthreads();
      }
    }
    if (want_attr) { // the tile's keys go; every thread has read n_used before the chunk's last barrier
      for (uint32_t i = tid; i < n_used; i += 256) tb.key[tb.used[i]] = 0u;
      if (tid == 0) tb.n_used = 0u;
      __syncthreads();
    }
    // ---- 5. dα, dβ
    const bool fused = t.fused(a.flags_or);
    if (want_bary && t.inside && (own != 0u || fused)) quad_store_owned(t.out, t, {da, db}, fused, own);
  });
}

// ================================================================================================================
// k_pos_grad — GRADIENTS TO VERTEX POSITIONS FROM A VISIBILITY BUFFER (srz_frameset_position_grad, include/srz.h): the step behind
// k_interp_grad's gbary.  With owners held fixed a pixel's α, β, γ are affine in its sample point (cover_v / cover_s's cross
// products over the area), ∇α = (by − cy, cx − bx) / area, ∇β = (cy − ay, ax − cx) / area, and moving corner k moves them by
// −w_k times that gradient.  Per owned pixel, from dα, dβ (gbary) and / or the gradient of the depth plane (gz):
//   g = (gx, gy), the gradient with respect to the sample point (gpix: from registers, deterministic, bit for bit);
//   −w_k gx, −w_k gy and, with gz, w_k gz ADDED into the owner's nine floats of gpos (ax ay z0 bx by z1 cx cy z2).
// k_interp_grad's walk and loads, the gradient quads in place of gout, and load_pos9 of the owner as k_motion has it — once for a
// quad of one owner.  The nine sums take k_interp_grad's four stages with nine values per owner where it has 3 * ATTR_CHUNK (quad
// runs; the segmented DPP row scan, every lane executing every shift; the tile's LDS table of distinct owners, an owner without a
// slot adding straight to memory; the dense flush with global_atomic_add_f32).  pg_scan_step, pg_emit and the flush are COPIES of
// ig_scan_step, ig_emit and k_interp_grad's step 4 (a helper templated on the value count would be inlined into k_interp_grad too
// and may move its registers: the project's rule for helpers); a fix goes into both.  What differs, there being no channel loop:
// the table is emptied by the flush itself — a slot's key is read and zeroed by ONE lane, which hands it to the slot's other eight
// lanes of the same wave through ds_bpermute; the slot counter alternates between two words by the tile's parity, the idle one
// zeroed between the barriers — so a tile costs one pair of barriers.
// Every thread of the workgroup reaches every barrier: a thread outside the frame owns nothing instead of moving on.
// has_gb / has_gz / want_pos / want_pix are kernel arguments: every branch on them is wave-uniform.
// The floor is the memory system: 4 bytes of id per pixel; 8 of α and β, 36 of gather and 8 / 4 of gradient planes per owned pixel;
// 8 written per pixel (gpix); 36 bytes of adds per distinct (tile, owner) pair, at the add rate.
// ================================================================================================================
constexpr uint32_t PG_VALS = 9, PG_SLOTS_PER_WAVE = 64 / PG_VALS;
struct PosGradTable {
  uint32_t key[IG_SLOTS];  // triangle index + 1; 0: free
  uint32_t used[IG_SLOTS]; // the slots taken, in arrival order
  uint32_t n_used[2];      // [tile parity]
  float val[IG_SLOTS * PG_VALS]; // [slot][corner][x, y, z]
};
// what a pixel needs of its owner: the edge differences of ∇α and ∇β, 1 / area, and z0 − z2, z1 − z2
struct PosGradTri {
  float by_cy, cy_ay, cx_bx, ax_cx, r, z0_z2, z1_z2;
};
__device__ __forceinline__ PosGradTri pg_tri(const SRZ_CAS float *p) {
  float P[9]; // ax ay z0 bx by z1 cx cy z2
  load_pos9(p, P);
  const float area = (P[3] - P[0]) * (P[7] - P[1]) - (P[4] - P[1]) * (P[6] - P[0]);
  return {P[4] - P[7], P[7] - P[1], P[6] - P[3], P[0] - P[6], 1.0f / area, P[2] - P[8], P[5] - P[8]}; // (the IEEE division)
}
// one owned pixel: (gx, gy) from dα, dβ (0 without gbary) and gz; with ACC its nine terms onto acc
template <bool ACC>
__device__ __forceinline__ void pg_pixel(const PosGradTri &T, bool has_gz, float da, float db, float gz, float wa, float wb, float wc, float &gx,
                                         float &gy, float (&acc)[PG_VALS]) {
  if (has_gz) da = fmaf_(gz, T.z0_z2, da), db = fmaf_(gz, T.z1_z2, db);
  gx = (da * T.by_cy + db * T.cy_ay) * T.r, gy = (da * T.cx_bx + db * T.ax_cx) * T.r;
  if (ACC) {
    acc[0] += (-wa) * gx, acc[1] += (-wa) * gy, acc[3] += (-wb) * gx, acc[4] += (-wb) * gy, acc[6] += (-wc) * gx, acc[7] += (-wc) * gy;
    if (has_gz) acc[2] += wa * gz, acc[5] += wb * gz, acc[8] += wc * gz;
  }
}
__device__ __forceinline__ void quad_put(float4 &v, int k, float x) { // (k: a variable)
  v.x = k == 0 ? x : v.x, v.y = k == 1 ? x : v.y, v.z = k == 2 ? x : v.z, v.w = k == 3 ? x : v.w;
}
template <int CTRL> __device__ __forceinline__ void pg_scan_step(float (&acc)[PG_VALS], uint32_t &stop) { // (ig_scan_step)
  const uint32_t up_stop = dpp_u32<CTRL>(stop);
#pragma unroll
  for (uint32_t e = 0; e < PG_VALS; ++e) {
    const float up = u2f(dpp_u32<CTRL>(f2u(acc[e])));
    if (!stop) acc[e] += up;
  }
  stop |= up_stop;
}
// (ig_emit; without gz the z slots take no add, here and in the flush)
__device__ __forceinline__ void pg_emit(PosGradTable &tb, uint32_t par, uint32_t key, const float (&acc)[PG_VALS], bool has_gz, float *gpos) {
  uint32_t h = (key * 0x9e3779b1u) >> (32u - IG_SLOT_BITS);
  bool found = false;
  for (uint32_t p = 0; p < IG_PROBES && !found; ++p) {
    const uint32_t old = atomicCAS(&tb.key[h], 0u, key);
    if (old == 0u) tb.used[atomicAdd(&tb.n_used[par], 1u)] = h; // (each slot is taken once: n_used <= IG_SLOTS)
    found = old == 0u || old == key;
    if (!found) h = (h + 1u) & (IG_SLOTS - 1u);
  }
  if (found) {
#pragma unroll
    for (uint32_t e = 0; e < PG_VALS; ++e)
      if (has_gz || e % 3u != 2u) atomicAdd(&tb.val[h * PG_VALS + e], acc[e]);
  } else {
    float *g = gpos + (size_t)(key - 1u) * PG_VALS;
#pragma unroll
    for (uint32_t e = 0; e < PG_VALS; ++e)
      if (has_gz || e % 3u != 2u) global_add(g + e, acc[e]);
  }
}
__global__ __launch_bounds__(256) void k_pos_grad(PosGradArgs a) {
  __shared__ PosGradTable tb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ly = wave * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
  const uint32_t tpf = a.n_local_bands * a.tiles_x, n_items = a.n_frames * tpf;
  const bool want_pos = a.gpos != nullptr, want_pix = a.out != nullptr, has_gb = a.gbary != nullptr, has_gz = a.gz != nullptr;
  if (want_pos) {
    for (uint32_t i = tid; i < IG_SLOTS; i += 256) tb.key[i] = 0u;
    for (uint32_t i = tid; i < IG_SLOTS * PG_VALS; i += 256) tb.val[i] = 0.0f;
    if (tid < 2) tb.n_used[tid] = 0u;
    __syncthreads();
  }
  uint32_t par = 0u; // the tile's parity in this workgroup's walk (the same in every thread: nobody skips a tile)
  // workgroup b walks the frames f ≡ b mod 8 tile by tile (fewer than 8 frames: every 8th tile): an inline copy of pass_walk
  const uint32_t sub = blockIdx.x & 7u, step = gridDim.x >> 3;
  for (uint32_t j = blockIdx.x >> 3;; j += step) {
    uint32_t f, t;
    if (a.n_frames >= 8u) {
      f = sub + 8u * (j / tpf), t = j % tpf;
      if (f >= a.n_frames) break;
    } else {
      const uint32_t i = j * 8u + sub;
      if (i >= n_items) break;
      f = i / tpf, t = i % tpf;
    }
    const SRZ_CAS FrameDesc *fd = as_const(a.frames) + f;
    const uint32_t lb = t / a.tiles_x, tx = t % a.tiles_x;
    const TileRect rc = tile_rect(a, fd, f, lb, tx);
    const int W = fd->width;
    const int y = rc.ty0 + ly, x4 = rc.tx0 + lx4;
    const bool inside = y <= rc.ty1 && x4 <= rc.tx1; // (a thread outside the frame owns nothing, and still meets the barriers)
    const bool whole = (W & 3) == 0 && x4 + 3 <= rc.tx1;
    const bool fused = ((fd->flags | a.flags_or) & SRZ_FUSED_CLEAR) != 0;
    const size_t poff = (size_t)lb * BAND * (size_t)W + (size_t)ly * (size_t)W + (size_t)x4;
    const float *gv = a.vis + (size_t)f * a.vis_stride + poff; // plane 0 (z: never read)
    // ---- 1. owner ids (index + 1 | S class; 0 or an index outside the frame's triangles: nobody)
    uint32_t id[4] = {0u, 0u, 0u, 0u};
    if (inside) {
      if (whole) {
        const uint4 q = *reinterpret_cast<const uint4 *>(gv + rc.plane);
        id[0] = q.x, id[1] = q.y, id[2] = q.z, id[3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x4 + k <= rc.tx1) id[k] = f2u(gv[rc.plane + k]);
      }
    }
    const uint32_t n_tris = fd->n_tris;
    uint32_t own = 0u, first = 0u;
    bool one_owner = true; // every owned pixel of the quad has the same triangle (either class)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if ((id[k] & ~S_CLASS_BIT) - 1u >= n_tris) id[k] = 0u; // (0 and the bare class bit wrap to 0xffffffff)
      if (id[k] == 0u) continue;
      own |= 1u << k;
      const uint32_t key = id[k] & ~S_CLASS_BIT;
      one_owner = one_owner && (first == 0u || first == key);
      first = first == 0u ? key : first;
    }
    // ---- 2. α, β and the gradient quads of a quad with an owner, each owner's γ by its class; words of nobody's pixels are loaded
    //         with their quad at most, never used
    float4 al = make_float4(0.f, 0.f, 0.f, 0.f), be = al, ga = al, qa = al, qb = al, qz = al;
    if (own != 0u) {
      const float *gg = a.gbary + (size_t)f * a.frame_stride + poff, *gz = a.gz + (size_t)f * a.gz_stride + poff;
      if (whole) {
        al = *reinterpret_cast<const float4 *>(gv + 2 * rc.plane), be = *reinterpret_cast<const float4 *>(gv + 3 * rc.plane);
        if (has_gb) qa = *reinterpret_cast<const float4 *>(gg), qb = *reinterpret_cast<const float4 *>(gg + rc.plane);
        if (has_gz) qz = *reinterpret_cast<const float4 *>(gz);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (own & (1u << k)) {
            quad_at(al, k) = gv[2 * rc.plane + k], quad_at(be, k) = gv[3 * rc.plane + k];
            if (has_gb) quad_at(qa, k) = gg[k], quad_at(qb, k) = gg[rc.plane + k];
            if (has_gz) quad_at(qz, k) = gz[k];
          }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) // (cover_s / cover_v)
        quad_at(ga, k) = (id[k] & S_CLASS_BIT) ? 1.0f - quad_at(al, k) - quad_at(be, k) : 1.0f - (quad_at(al, k) + quad_at(be, k));
    }
    const SRZ_CAS float *tpos = as_const(a.tri_pos) + (size_t)fd->tri_off * a.pos_stride;
    float *gpo = a.gpos + (size_t)f * a.gpos_stride;
    // the key a quad of one owner takes into the row's scan; 0: the quad emits its runs itself, or has none
    const uint32_t skey = want_pos && own != 0u && one_owner ? first : 0u;
    const bool scan = want_pos && __builtin_amdgcn_ballot_w64(skey != 0u) != 0ull; // (wave-uniform)
    const uint32_t pos = (uint32_t)lane & 7u;
    // (every lane executes both shifts: a lane that skipped one behind a short-circuit would be missing as its neighbour's source)
    const uint32_t key_left = dpp_u32<DPP_ROW_SHR1>(skey), key_right = dpp_u32<DPP_ROW_SHL1>(skey);
    const bool seg_head = (pos == 0u) | (key_left != skey) | (skey == 0u); // (a quad without a key takes no carry)
    const bool seg_last = (pos == 7u) | (key_right != skey);
    // ---- 3. the pixels: (gx, gy) into qx, qy, the nine terms onto the open run's sums
    float4 qx = make_float4(0.f, 0.f, 0.f, 0.f), qy = qx; // nobody: zeros
    float acc[PG_VALS];
#pragma unroll
    for (uint32_t e = 0; e < PG_VALS; ++e) acc[e] = 0.0f;
    uint32_t cur = 0u; // the open run's key (a quad of several owners)
    if (own != 0u && one_owner) { // one owner: one gather, the quad is one run
      const PosGradTri T = pg_tri(tpos + (size_t)(first - 1u) * a.pos_stride);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (id[k] == 0u) continue;
        float gx, gy;
        if (want_pos)
          pg_pixel<true>(T, has_gz, quad_at(qa, k), quad_at(qb, k), quad_at(qz, k), quad_at(al, k), quad_at(be, k), quad_at(ga, k), gx, gy, acc);
        else
          pg_pixel<false>(T, has_gz, quad_at(qa, k), quad_at(qb, k), quad_at(qz, k), quad_at(al, k), quad_at(be, k), quad_at(ga, k), gx, gy, acc);
        quad_at(qx, k) = gx, quad_at(qy, k) = gy;
      }
    } else if (own != 0u) { // several owners (an edge crosses the quad): pixel after pixel, a run that ends goes into the table
      PosGradTri T = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; // the open run's owner
#pragma nounroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t idk = k == 0 ? id[0] : k == 1 ? id[1] : k == 2 ? id[2] : id[3];
        if (idk == 0u) continue;
        const uint32_t key = idk & ~S_CLASS_BIT;
        if (want_pos && cur != 0u && key != cur) {
          pg_emit(tb, par, cur, acc, has_gz, gpo);
#pragma unroll
          for (uint32_t e = 0; e < PG_VALS; ++e) acc[e] = 0.0f;
        }
        if (key != cur) T = pg_tri(tpos + (size_t)(key - 1u) * a.pos_stride);
        cur = key;
        float gx, gy;
        if (want_pos)
          pg_pixel<true>(T, has_gz, quad_pick(qa, k), quad_pick(qb, k), quad_pick(qz, k), quad_pick(al, k), quad_pick(be, k), quad_pick(ga, k), gx, gy, acc);
        else
          pg_pixel<false>(T, has_gz, quad_pick(qa, k), quad_pick(qb, k), quad_pick(qz, k), quad_pick(al, k), quad_pick(be, k), quad_pick(ga, k), gx, gy, acc);
        quad_put(qx, k, gx), quad_put(qy, k, gy);
      }
    }
    if (want_pos) {
      if (scan) { // inclusive segmented scan over the 8 quads of the tile row (Hillis-Steele: a lane past a head takes no carry)
        uint32_t stop = seg_head ? 1u : 0u; // (position p < d has stop set before the step of distance d: position 0 is a head)
        pg_scan_step<DPP_ROW_SHR1>(acc, stop);
        pg_scan_step<DPP_ROW_SHR2>(acc, stop);
        pg_scan_step<DPP_ROW_SHR4>(acc, stop);
      }
      // the last quad of a row's run holds the run's sum; a quad of several owners (a head: the scan left it alone) its last run
      const uint32_t ekey = skey != 0u ? (seg_last ? skey : 0u) : cur;
      if (ekey != 0u) pg_emit(tb, par, ekey, acc, has_gz, gpo);
      // ---- 4. the table into memory, and emptied: PG_SLOTS_PER_WAVE slots per wave and pass, a slot's nine floats on nine
      //         consecutive lanes; the slot's first lane reads and frees the key, the others get it from that lane
      __syncthreads();
      const uint32_t n_used = tb.n_used[par];
      if (tid == 0) tb.n_used[par ^ 1u] = 0u; // (last read before the previous tile's second barrier, next added to behind this tile's)
      const uint32_t sl = (uint32_t)lane / PG_VALS, e = (uint32_t)lane - sl * PG_VALS;
      for (uint32_t base = (uint32_t)wave * PG_SLOTS_PER_WAVE; base < n_used; base += 4u * PG_SLOTS_PER_WAVE) { // (wave-uniform)
        const bool on = sl < PG_SLOTS_PER_WAVE && base + sl < n_used;
        uint32_t s = 0u, key = 0u;
        if (on) s = tb.used[base + sl];
        if (on && e == 0u) key = tb.key[s], tb.key[s] = 0u;
        key = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(sl * PG_VALS) << 2, (int)key); // (every lane executes it)
        if (on) {
          const float v = tb.val[s * PG_VALS + e];
          tb.val[s * PG_VALS + e] = 0.0f;
          if (has_gz || e % 3u != 2u) global_add(gpo + (size_t)(key - 1u) * PG_VALS + e, v);
        }
      }
      __syncthreads();
      par ^= 1u;
    }
    // ---- 5. gx, gy: whole quads (fused clear, or four owners), else the owned pixels only
    if (want_pix && inside && (own != 0u || fused)) {
      float *go = rc.out0 + (size_t)ly * (size_t)W + (size_t)x4;
      if (fused || own == 15u) {
        quad_store(go, rc.plane, {qx, qy}, whole, x4, rc.tx1);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (own & (1u << k)) go[k] = quad_at(qx, k), go[rc.plane + k] = quad_at(qy, k);
      }
    }
  }
}

// ================================================================================================================
// k_antialias / k_antialias_grad — SILHOUETTE ANTIALIASING OF A VISIBILITY BUFFER (srz_frameset_antialias / _antialias_grad,
// include/srz.h states the rule).  Where two 4-neighbours have different owners, the nearer owner's edge is intersected with the
// segment between the two sample points; the pixel on whose side of the midpoint the crossing does not lie takes that share of
// the other's value.  The forward is a gather (out[p] from in[p] and in[q] of its four neighbours), so is gin; gpos is the one
// scatter: per pair four no-return global_atomic_add_f32, from the thread that holds the pair's left or upper pixel.
// k_interp's shape: the XCD-ordered grid walk, four pixels of a row per thread, 16-byte id loads, quad_store, the channel loop
// wave-uniform in register chunks of ATTR_CHUNK.  No LDS and no barrier.
// THE NEIGHBOUR ROWS COME FROM THE CACHES, not from an LDS tile with a halo: a thread reads the id quads of the rows above and below
// and the two words beside its quad straight from memory.  The rows of a tile are read by the lanes of one workgroup within a few
// instructions of each other (a wave holds eight consecutive rows), so every id line is fetched from HBM once and its two re-reads
// hit the vector L1 or L2; ids are 4 of the 4 + 8 n_ch bytes a pixel moves.  A tile in LDS would need the same 132 halo words from
// memory, a barrier per tile, and would put that barrier into the path of the quads that only copy — nearly all of them.
// FAST PATH: the 14 keys (the quad, left, right, the quads above and below; key = index + 1 of an owner, 0 for nobody: the class bit
// and the flavour of a nobody id do not tell pixels apart) are one value → the quad's planes are copied; no z, no position is read.
// SLOW PATH: the z words of the 14 pixels, then the quad's 13 pairs one after the other in ONE loop (its body, aa_pair, exists once
// in the code; the keys and depths are picked with short select chains, the weights put back the same way: no indexed register array, no
// scratch): load_pos9 of N, and of F once an edge is found and F has an owner.  Each pair's weight lands in the slots of the quad's
// pixels it touches (16 weights: pixel x neighbour in the rule's order left, right, up, down; masks say whose target it is).  In
// the backward the pairs whose left or upper pixel is the thread's own (8 of the 13) also form D over the channels and add.
// The floor is the memory system: 4 bytes of id per pixel plus 8 n_ch per pixel.
// ================================================================================================================
constexpr int AA_PAIRS = 13;
// the 14 values a quad's pairs are decided from: the pixel left of the quad, the quad, the pixel right of it, the quads above and below
// (scalars, not arrays: an array picked from by a variable index is put into scratch)
template <class T> struct AaHood {
  T l, c0, c1, c2, c3, r, u0, u1, u2, u3, d0, d1, d2, d3;
};
template <class T> __device__ __forceinline__ T aa_pick4(T v0, T v1, T v2, T v3, int k) { return k == 0 ? v0 : k == 1 ? v1 : k == 2 ? v2 : v3; } // (k: a variable)
// A and B of pair e of the quad: [0..4] left | 0 | 1 | 2 | 3 | right (k = e - 1: A's pixel), [5..8] above k | k, [9..12] k | below k
template <class T> __device__ __forceinline__ void aa_pick(const AaHood<T> &h, bool horiz, bool above, int k, T &va, T &vb) {
  const T ck = aa_pick4(h.c0, h.c1, h.c2, h.c3, k), ck1 = aa_pick4(h.c0, h.c1, h.c2, h.c3, k + 1);
  const T uk = aa_pick4(h.u0, h.u1, h.u2, h.u3, k), dk = aa_pick4(h.d0, h.d1, h.d2, h.d3, k);
  va = horiz ? (k < 0 ? h.l : ck) : above ? uk : ck;
  vb = horiz ? (k == 3 ? h.r : ck1) : above ? ck : dk;
}
__device__ __forceinline__ void aa_put(float (&v)[16], int i, float x) { // (i: a variable)
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = i == j ? x : v[j];
}
__device__ __forceinline__ uint32_t aa_key(uint32_t id, uint32_t n_tris) { // index + 1 of an owner, 0 for nobody
  const uint32_t k = id & ~S_CLASS_BIT;
  return k - 1u < n_tris ? k : 0u; // (0 and the bare class bit wrap to 0xffffffff)
}
struct AaPair {
  uint32_t tgt;   // 0: nothing; 1: A (the left or upper pixel) is the target; 2: B
  float w;
  uint32_t n_key; // N's triangle index + 1
  uint32_t c0;    // the edge's first corner
  bool to_f;      // a > 0
  float s, k, d, n0, n1, u0, u1;
};
__device__ __forceinline__ bool aa_same_vertex(float x, float y, float z, const float (&Q)[9]) {
  const uint32_t a = f2u(x), b = f2u(y), c = f2u(z);
  return (a == f2u(Q[0]) && b == f2u(Q[1]) && c == f2u(Q[2])) || (a == f2u(Q[3]) && b == f2u(Q[4]) && c == f2u(Q[5])) ||
         (a == f2u(Q[6]) && b == f2u(Q[7]) && c == f2u(Q[8]));
}
// the pair of A at (xa, ya) with B at (xa + 1, ya) (horiz) or (xa, ya + 1); ka != kb are their keys, za, zb their depths
__device__ __forceinline__ AaPair aa_pair(const SRZ_CAS float *tpos, uint32_t pos_stride, uint32_t ka, uint32_t kb, float za, float zb, int xa,
                                          int ya, bool horiz) {
  AaPair r = {0u, 0.0f, 0u, 0u, false, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const bool n_is_b = ka == 0u || (kb != 0u && zb < za); // (a nobody is farther than any owner; ties and NaN: A)
  const uint32_t kn = n_is_b ? kb : ka, kf = n_is_b ? ka : kb;
  const float s = n_is_b ? -1.0f : 1.0f;
  const float xn = (float)(xa + (horiz && n_is_b ? 1 : 0)), yn = (float)(ya + (!horiz && n_is_b ? 1 : 0));
  float P[9];
  load_pos9(tpos + (size_t)(kn - 1u) * pos_stride, P);
  float u[3], n[3];
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const float dx = P[3 * v] - xn, dy = P[3 * v + 1] - yn;
    u[v] = horiz ? s * dx : s * dy, n[v] = horiz ? dy : dx;
  }
  bool found = false;
  float t = 0.0f, v0x = 0.0f, v0y = 0.0f, v0z = 0.0f, v1x = 0.0f, v1y = 0.0f, v1z = 0.0f;
#pragma unroll
  for (int e = 0; e < 3; ++e) { // the first edge that straddles N's line and crosses it between the two sample points
    const int e1 = (e + 1) % 3;
    const float n0 = n[e], n1 = n[e1];
    const bool straddle = (n0 <= 0.0f && n1 > 0.0f) || (n1 <= 0.0f && n0 > 0.0f);
    const float d = n0 - n1, k = n0 / d; // (the IEEE division)
    const float te = u[e] + k * (u[e1] - u[e]);
    if (!found && straddle && 0.0f <= te && te <= 1.0f) {
      found = true, t = te;
      r.c0 = (uint32_t)e, r.k = k, r.d = d, r.n0 = n0, r.n1 = n1, r.u0 = u[e], r.u1 = u[e1];
      v0x = P[3 * e], v0y = P[3 * e + 1], v0z = P[3 * e + 2], v1x = P[3 * e1], v1y = P[3 * e1 + 1], v1z = P[3 * e1 + 2];
    }
  }
  if (!found) return r;
  if (kf != 0u) { // the two owners share this edge: an interior edge of a mesh
    float Q[9];
    load_pos9(tpos + (size_t)(kf - 1u) * pos_stride, Q);
    if (aa_same_vertex(v0x, v0y, v0z, Q) && aa_same_vertex(v1x, v1y, v1z, Q)) return r;
  }
  const float a = t - 0.5f;
  r.n_key = kn, r.s = s, r.to_f = a > 0.0f;
  if (a > 0.0f) r.tgt = n_is_b ? 1u : 2u, r.w = a;
  else if (a < 0.0f) r.tgt = n_is_b ? 2u : 1u, r.w = -a;
  return r;
}
// pixels x4 .. x4 + 3 of a row at p: one 16-byte load if the quad is whole, else the pixels up to tx1 (the others: 0)
__device__ __forceinline__ float4 aa_quad(const float *p, bool whole, int x4, int tx1) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (whole) {
    v = *reinterpret_cast<const float4 *>(p);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x4 + k <= tx1) quad_at(v, k) = p[k];
  }
  return v;
}
template <bool GRAD> __device__ __forceinline__ void aa_body(const AntialiasArgs &a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ly = wave * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
  const uint32_t tpf = a.n_local_bands * a.tiles_x, n_items = a.n_frames * tpf;
  const uint32_t C = a.n_ch;
  const bool want_out = !GRAD || a.out != nullptr, want_pos = GRAD && a.gpos != nullptr; // (kernel arguments: wave-uniform)
  // workgroup b walks the frames f ≡ b mod 8 tile by tile (fewer than 8 frames: every 8th tile): an inline copy of pass_walk
  const uint32_t sub = blockIdx.x & 7u, step = gridDim.x >> 3;
  for (uint32_t j = blockIdx.x >> 3;; j += step) {
    uint32_t f, t;
    if (a.n_frames >= 8u) {
      f = sub + 8u * (j / tpf), t = j % tpf;
      if (f >= a.n_frames) break;
    } else {
      const uint32_t i = j * 8u + sub;
      if (i >= n_items) break;
      f = i / tpf, t = i % tpf;
    }
    const SRZ_CAS FrameDesc *fd = as_const(a.frames) + f;
    const uint32_t lb = t / a.tiles_x, tx = t % a.tiles_x;
    const TileRect rc = tile_rect(a, fd, f, lb, tx);
    const int W = fd->width, H = fd->height;
    const int y = rc.ty0 + ly, x4 = rc.tx0 + lx4;
    if (!(y <= rc.ty1 && x4 <= rc.tx1)) continue; // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool whole = (W & 3) == 0 && x4 + 3 <= rc.tx1;
    // (the shard is the whole frame — the host refuses anything else — so local row = frame row and y +- 1 is the row beside it)
    const size_t poff = (size_t)lb * BAND * (size_t)W + (size_t)ly * (size_t)W + (size_t)x4;
    const float *gz = a.vis + (size_t)f * a.vis_stride + poff; // plane 0 (z: read by the slow path only)
    const float *gi = gz + rc.plane;                           // plane 1 (ids)
    const bool up = y > 0, down = y < H - 1, left = x4 > 0, right = x4 + 4 <= W - 1;
    // ---- 1. the 14 keys
    const uint32_t n_tris = fd->n_tris;
    uint32_t kc[4] = {0u, 0u, 0u, 0u}, ku[4] = {0u, 0u, 0u, 0u}, kd[4] = {0u, 0u, 0u, 0u}, kl = 0u, kr = 0u; // (constant indices only)
    if (whole) {
      const uint4 q = *reinterpret_cast<const uint4 *>(gi);
      kc[0] = q.x, kc[1] = q.y, kc[2] = q.z, kc[3] = q.w;
      if (up) {
        const uint4 v = *reinterpret_cast<const uint4 *>(gi - W);
        ku[0] = v.x, ku[1] = v.y, ku[2] = v.z, ku[3] = v.w;
      }
      if (down) {
        const uint4 v = *reinterpret_cast<const uint4 *>(gi + W);
        kd[0] = v.x, kd[1] = v.y, kd[2] = v.z, kd[3] = v.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x4 + k <= rc.tx1) {
          kc[k] = f2u(gi[k]);
          if (up) ku[k] = f2u(gi[k - W]);
          if (down) kd[k] = f2u(gi[k + W]);
        }
    }
    if (left) kl = f2u(gi[-1]);
    if (right) kr = f2u(gi[4]);
    kl = aa_key(kl, n_tris), kr = aa_key(kr, n_tris);
#pragma unroll
    for (int k = 0; k < 4; ++k) kc[k] = aa_key(kc[k], n_tris), ku[k] = aa_key(ku[k], n_tris), kd[k] = aa_key(kd[k], n_tris);
    // a neighbour outside the frame, and a pixel of the quad beyond the frame's edge, take the key beside them: no pair there
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (x4 + k > rc.tx1) kc[k] = kc[k - 1];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!up || x4 + k > rc.tx1) ku[k] = kc[k];
      if (!down || x4 + k > rc.tx1) kd[k] = kc[k];
    }
    if (!left) kl = kc[0];
    if (!right) kr = kc[3];
    bool slow = kl != kc[0] || kr != kc[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) slow = slow || kc[k] != kc[0] || ku[k] != kc[0] || kd[k] != kc[0];
    const AaHood<uint32_t> key = {kl, kc[0], kc[1], kc[2], kc[3], kr, ku[0], ku[1], ku[2], ku[3], kd[0], kd[1], kd[2], kd[3]};
    // ---- 2. a quad with a differing pair: the depths, then the 13 pairs — [0..4] horizontal (left | 0 | 1 | 2 | 3 | right),
    //         [5..8] the pixel above with pixel k, [9..12] pixel k with the pixel below
    float wt[16]; // [pixel][left, right, up, down]: the weight of the pair with that neighbour, if it has a target
#pragma unroll
    for (int i = 0; i < 16; ++i) wt[i] = 0.0f;
    uint32_t mine = 0u, theirs = 0u; // bit 4 k + j: that pair's target is pixel k / is its neighbour
    if (slow) {
      const float4 zc = aa_quad(gz, whole, x4, rc.tx1);
      float4 zu = make_float4(0.f, 0.f, 0.f, 0.f), zd = zu;
      if (up) zu = aa_quad(gz - W, whole, x4, rc.tx1);
      if (down) zd = aa_quad(gz + W, whole, x4, rc.tx1);
      const AaHood<float> z = {left ? gz[-1] : 0.0f, zc.x, zc.y, zc.z, zc.w, right ? gz[4] : 0.0f, zu.x, zu.y, zu.z, zu.w, zd.x, zd.y, zd.z, zd.w};
      const SRZ_CAS float *tpos = as_const(a.tri_pos) + (size_t)fd->tri_off * a.pos_stride;
#pragma nounroll
      for (int e = 0; e < AA_PAIRS; ++e) {
        const bool horiz = e < 5, above = !horiz && e < 9;
        const int k = horiz ? e - 1 : (e - 5) & 3; // the quad's pixel of the pair: horizontal: A's (-1: A is the left neighbour)
        uint32_t ka, kb;
        aa_pick(key, horiz, above, k, ka, kb);
        if (ka == kb) continue; // (two nobodies, one triangle, or no neighbour there)
        const int xa = x4 + k, ya = above ? y - 1 : y;
        float za, zb;
        aa_pick(z, horiz, above, k, za, zb);
        const AaPair pr = aa_pair(tpos, a.pos_stride, ka, kb, za, zb, xa, ya, horiz);
        if (pr.tgt == 0u) continue;
        // the slot of A's pair with B (A one of the quad's pixels), and of B's with A
        const int sa = horiz ? (e >= 1 ? 4 * k + 1 : -1) : (above ? -1 : 4 * k + 3);
        const int sb = horiz ? (e <= 3 ? 4 * (k + 1) + 0 : -1) : (above ? 4 * k + 2 : -1);
        if (sa >= 0) aa_put(wt, sa, pr.w), (pr.tgt == 1u ? mine : theirs) |= 1u << sa;
        if (sb >= 0) aa_put(wt, sb, pr.w), (pr.tgt == 2u ? mine : theirs) |= 1u << sb;
        if (GRAD) {
          if (want_pos && sa >= 0) { // each pair adds once: from its left or upper pixel
            const ptrdiff_t oa = (ptrdiff_t)k, ob = oa + (horiz ? (ptrdiff_t)1 : (ptrdiff_t)W);
            const ptrdiff_t ot = pr.tgt == 1u ? oa : ob, os = pr.tgt == 1u ? ob : oa;
            const float *pin = a.in + (size_t)f * a.frame_stride + poff, *pg = a.gout + (size_t)f * a.frame_stride + poff;
            float D = 0.0f;
            for (uint32_t ch = 0; ch < C; ++ch) {
              const size_t o = (size_t)ch * rc.plane;
              D = fmaf_(pg[(ptrdiff_t)o + ot], pin[(ptrdiff_t)o + os] - pin[(ptrdiff_t)o + ot], D);
            }
            const float g = pr.to_f ? D : -D;
            const float ed = pr.u1 - pr.u0;
            const float qq = (g * ed) / (pr.d * pr.d); // (the IEEE division)
            const float g_u0 = pr.s * (g * (1.0f - pr.k)), g_u1 = pr.s * (g * pr.k), g_n0 = qq * (-pr.n1), g_n1 = qq * pr.n0;
            float *gp = a.gpos + (size_t)f * a.gpos_stride + (size_t)(pr.n_key - 1u) * 9u;
            const uint32_t c0 = 3u * pr.c0, c1 = pr.c0 == 2u ? 0u : c0 + 3u;
            global_add(gp + c0, horiz ? g_u0 : g_n0), global_add(gp + c1, horiz ? g_u1 : g_n1);
            global_add(gp + c0 + 1u, horiz ? g_n0 : g_u0), global_add(gp + c1 + 1u, horiz ? g_n1 : g_u1);
          }
        }
      }
    }
    if (!want_out) continue;
    // ---- 3. the channels, ATTR_CHUNK at a time: the quad's words, blended where a pair has a target (forward: the planes; backward:
    //         gout into gin)
    const float *src = (GRAD ? a.gout : a.in) + (size_t)f * a.frame_stride + poff;
    float *go = rc.out0 + (size_t)ly * (size_t)W + (size_t)x4;
    const uint32_t any = mine | (GRAD ? theirs : 0u);
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 q[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
        q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < nc) q[i] = aa_quad(src + (size_t)(c0 + i) * rc.plane, whole, x4, rc.tx1);
      }
      if (any != 0u) {
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
          if (i >= nc) break;
          const float *p = src + (size_t)(c0 + i) * rc.plane;
          const float4 own = q[i];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (((any >> (4 * k)) & 15u) == 0u) continue;
            const float pv = quad_at(own, k);
            float acc = pv;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) { // (x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)
              const uint32_t bit = 1u << (4 * k + nb);
              if (!(any & bit)) continue;
              const float qv = nb == 0 ? (k > 0 ? quad_at(own, k > 0 ? k - 1 : 0) : p[-1])
                             : nb == 1 ? (k < 3 ? quad_at(own, k < 3 ? k + 1 : 3) : p[4])
                             : nb == 2 ? p[k - W] : p[k + W];
              const float w = wt[4 * k + nb];
              if (!GRAD) acc = fmaf_(w, qv - pv, acc);
              else if (mine & bit) acc = fmaf_(-w, pv, acc);
              else acc = fmaf_(w, qv, acc);
            }
            quad_at(q[i], k) = acc;
          }
        }
      }
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
        if (i >= nc) break;
        quad_store(go + (size_t)(c0 + i) * rc.plane, rc.plane, {q[i]}, whole, x4, rc.tx1);
      }
    }
  }
}
__global__ __launch_bounds__(256) void k_antialias(AntialiasArgs a) { aa_body<false>(a); }
__global__ __launch_bounds__(256) void k_antialias_grad(AntialiasArgs a) { aa_body<true>(a); }

// ================================================================================================================
// k_tex — CALLER TEXTURES OVER A VISIBILITY BUFFER (srz_frameset_texture, include/srz.h states the rule): a float texture of the
// caller's, [frame][row][column][channel], sampled bilinearly at the uv planes interpolate (or gbuffer(UV)) wrote.  k_interp's shape:
// no LDS, no barrier; the XCD-ordered walk over (frame, tile), 4 pixels of a row per thread, one 16-byte id load, u and v only for a
// quad with an owner, every plane leaves through quad_store.  The four texel indices and the two fractions of a pixel are formed
// once; the wave-uniform channel loop then gathers 4 * nc floats per sampled pixel, ATTR_CHUNK channels at a time, the tail masked.
// Every float -> int conversion follows the clamp (CLAMP) or the fraction (WRAP): no uv leaves the texture.
// ================================================================================================================
struct TexTap {
  uint32_t i00, i01, i10, i11; // texel indices row * tex_w + column of the corners (y0, x0), (y0, x1), (y1, x0), (y1, x1)
  float tx, ty;
  bool in_x, in_y;             // CLAMP: the coordinate lies strictly inside the texel centres' range (else its derivative is 0)
};
__device__ __forceinline__ bool tex_finite(float u) { return __builtin_fabsf(u) < __builtin_inff(); }
// one axis of the rule: coordinate u over n texels -> the two texel coordinates, the fraction, and whether u moves the sample
__device__ __forceinline__ void tex_axis(float u, uint32_t n, bool wrap, int &i0, int &i1, float &t, bool &in) {
  const float nf = (float)n, hi = (float)(n - 1u);
  if (wrap) u = u - __builtin_floorf(u);
  float fx = u * nf - 0.5f;
  in = true;
  if (!wrap) {
    in = fx > 0.0f && fx < hi;
    fx = __builtin_fminf(__builtin_fmaxf(fx, 0.0f), hi);
  }
  const float f0 = __builtin_floorf(fx);
  t = fx - f0;
  i0 = (int)f0, i1 = i0 + 1;
  if (!wrap) {
    i1 = min(i1, (int)n - 1);
  } else {
    if (i0 < 0) i0 += (int)n;
    if (i1 >= (int)n) i1 -= (int)n;
  }
}
__device__ __forceinline__ TexTap tex_tap(float u, float v, uint32_t tw, uint32_t th, bool wrap) {
  int x0, x1, y0, y1;
  TexTap p;
  tex_axis(u, tw, wrap, x0, x1, p.tx, p.in_x);
  tex_axis(v, th, wrap, y0, y1, p.ty, p.in_y);
  p.i00 = (uint32_t)y0 * tw + (uint32_t)x0, p.i01 = (uint32_t)y0 * tw + (uint32_t)x1;
  p.i10 = (uint32_t)y1 * tw + (uint32_t)x0, p.i11 = (uint32_t)y1 * tw + (uint32_t)x1;
  return p;
}
// what k_tex and k_tex_grad do alike in front of their channel loops: the ids, the owners, u and v of a quad with an owner, the
// taps of the sampled pixels (an owner whose u and v are both finite) -> `own` and `smp`, one bit per pixel
template <class A>
__device__ __forceinline__ void tex_quad(const A &a, const SRZ_CAS FrameDesc *fd, const TileRect &rc, uint32_t f, size_t poff, bool inside,
                                         bool whole, int x4, TexTap (&tap)[4], uint32_t &own, uint32_t &smp) {
  const float *gv = a.vis + (size_t)f * a.vis_stride + poff; // plane 0 (z: never read)
  uint32_t id[4] = {0u, 0u, 0u, 0u};
  if (inside) {
    if (whole) {
      const uint4 q = *reinterpret_cast<const uint4 *>(gv + rc.plane);
      id[0] = q.x, id[1] = q.y, id[2] = q.z, id[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x4 + k <= rc.tx1) id[k] = f2u(gv[rc.plane + k]);
    }
  }
  const uint32_t n_tris = fd->n_tris;
  own = 0u, smp = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if ((id[k] & ~S_CLASS_BIT) - 1u < n_tris) own |= 1u << k; // (0 and the bare class bit wrap to 0xffffffff)
  if (own == 0u) return;
  float4 uv[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  quad_load(a.uv + (size_t)f * a.uv_stride + poff, rc.plane, uv, whole, x4, rc.tx1);
  const bool wrap = a.mode == SRZ_TEX_WRAP;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float u = quad_at(uv[0], k), v = quad_at(uv[1], k);
    if (!(own & (1u << k)) || !tex_finite(u) || !tex_finite(v)) continue;
    smp |= 1u << k;
    tap[k] = tex_tap(u, v, a.tex_w, a.tex_h, wrap);
  }
}
__global__ __launch_bounds__(256) void k_tex(TexArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ly = wave * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
  const uint32_t tpf = a.n_local_bands * a.tiles_x, n_items = a.n_frames * tpf;
  const uint32_t C = a.n_ch;
  // workgroup b walks the frames f ≡ b mod 8 tile by tile (fewer than 8 frames: every 8th tile): an inline copy of pass_walk
  const uint32_t sub = blockIdx.x & 7u, step = gridDim.x >> 3;
  for (uint32_t j = blockIdx.x >> 3;; j += step) {
    uint32_t f, t;
    if (a.n_frames >= 8u) {
      f = sub + 8u * (j / tpf), t = j % tpf;
      if (f >= a.n_frames) break;
    } else {
      const uint32_t i = j * 8u + sub;
      if (i >= n_items) break;
      f = i / tpf, t = i % tpf;
    }
    const SRZ_CAS FrameDesc *fd = as_const(a.frames) + f;
    const uint32_t lb = t / a.tiles_x, tx = t % a.tiles_x;
    const TileRect rc = tile_rect(a, fd, f, lb, tx);
    const int W = fd->width;
    const int y = rc.ty0 + ly, x4 = rc.tx0 + lx4;
    if (!(y <= rc.ty1 && x4 <= rc.tx1)) continue; // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool whole = (W & 3) == 0 && x4 + 3 <= rc.tx1;
    const bool fused = ((fd->flags | a.flags_or) & SRZ_FUSED_CLEAR) != 0;
    const size_t poff = (size_t)lb * BAND * (size_t)W + (size_t)ly * (size_t)W + (size_t)x4;
    float *go = rc.out0 + (size_t)ly * (size_t)W + (size_t)x4;
    // ---- 1. owners, u and v, the taps
    TexTap tap[4] = {};
    uint32_t own, smp;
    tex_quad(a, fd, rc, f, poff, true, whole, x4, tap, own, smp);
    if (own == 0u && !fused) continue;
    const SRZ_CAS float *tex = as_const(a.tex) + (size_t)f * a.tex_frame_stride;
    const bool quads = fused || own == 15u; // whole quads (fused clear, or four owners), else the owned pixels only
    // ---- 2. the channels, ATTR_CHUNK at a time
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 q[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) q[i] = make_float4(0.f, 0.f, 0.f, 0.f); // nobody, and an owner that is not sampled: zeros
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(smp & (1u << k))) continue;
        const SRZ_CAS float *p00 = tex + (size_t)tap[k].i00 * C + c0, *p01 = tex + (size_t)tap[k].i01 * C + c0;
        const SRZ_CAS float *p10 = tex + (size_t)tap[k].i10 * C + c0, *p11 = tex + (size_t)tap[k].i11 * C + c0;
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
          if (i < nc) {
            const float t00 = p00[i], t01 = p01[i], t10 = p10[i], t11 = p11[i];
            const float top = fmaf_(tap[k].tx, t01 - t00, t00), bot = fmaf_(tap[k].tx, t11 - t10, t10);
            quad_at(q[i], k) = fmaf_(tap[k].ty, bot - top, top);
          }
      }
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
        if (i >= nc) break;
        float *p = go + (size_t)(c0 + i) * rc.plane;
        if (quads) {
          quad_store(p, rc.plane, {q[i]}, whole, x4, rc.tx1);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (own & (1u << k)) p[k] = quad_at(q[i], k);
        }
      }
    }
  }
}

// ================================================================================================================
// k_tex_grad — THE BACKWARD OF k_tex (srz_frameset_texture_grad): per sampled pixel and channel, four adds w[corner] * gout into the
// texture gradient (gtex), and the gradient with respect to u and v (guv: fma chains over the channels, from registers, no atomics).
// The same walk and the same loads as k_tex, plus gout's quads, chunk by chunk.
// Neighbouring pixels share texels (a magnified texture: dozens of pixels per texel; one texel per pixel: every texel is a corner of
// four pixels), so the adds are combined before they leave the CU, as k_interp_grad combines its owners':
//   1. in front of the channel loop every (pixel, corner) finds its texel's slot in the tile's table in LDS: open addressing on the
//      texel index, TG_PROBES probes, TG_SLOTS slots.  A HASHED table, not a dense window anchored at the tile's smallest texel: the
//      uv of a tile are whatever the mesh's charts are — a seam, a WRAP border or a minified texture spreads a tile's texels over
//      the whole image, where a window holds nothing, while the table's capacity counts DISTINCT texels wherever they lie;
//   2. per chunk the adds go to the slot's ATTR_CHUNK floats with LDS float adds; a corner that found no slot adds straight to
//      memory — correct, only slower;
//   3. after a barrier the chunk's values are flushed: the used slots are listed, so consecutive lanes add the consecutive
//      channels of one texel, texel after texel, with global_atomic_add_f32.
// Global adds are thus per (tile, distinct texel, channel).  The table's keys live for the whole tile, its values for one chunk.
// Every thread of the workgroup reaches every barrier: a thread outside the frame samples nothing instead of moving on.
// ================================================================================================================
constexpr uint32_t TG_SLOT_BITS = 11, TG_SLOTS = 1u << TG_SLOT_BITS, TG_PROBES = 8, TG_NONE = 0xffffffffu;
__device__ __forceinline__ void lds_add(float *p, float v) { unsafeAtomicAdd(p, v); }
// The table, for every kernel that scatters into a caller's texture.  WHO is the kernel's argument struct and only a tag: it gives
// each kernel its own instantiation of the members, and with that the registers it had with a copy of its own, where the same
// helpers shared by name moved them (DESIGN.md §4 has the figures, and what the pieces below cost in instructions).  VALS: the
// values per slot, ATTR_CHUNK (49 156 bytes of LDS), or 1 for k_shadow_grad's one channel (24 KB).  A key is the 32-bit number,
// below 2^32 - 1, that names a texel to the kernel: a texel index (below SRZ_TEX_MAX_SIZE^2 = 2^28; a cube's below 6 * 2^28), an
// offset in a cube's pyramid or a (slot, texel) pair (both below 2^31).
// Every thread of the workgroup calls init (a barrier follows it), flush and release (they hold their barriers).
// The helpers take plain values and are straight-line per channel; the chunk's loops stay in the kernels.  That is measured, not
// taste: an adder that took its destination as a closure, or a helper that held the loop over the chunk, changed the registers of
// half the kernels (k_background_grad 169 -> 101 VGPRs with 3 more spilled SGPRs; one form did not compile), these do not.
template <class WHO, uint32_t VALS> struct TexelTable {
  uint32_t key[TG_SLOTS];  // the texel's key + 1; 0: free
  uint32_t used[TG_SLOTS]; // the slots taken, in arrival order
  uint32_t n_used;
  float val[TG_SLOTS * VALS]; // [slot][channel of the chunk]
  __device__ __forceinline__ void init(uint32_t tid) {
    for (uint32_t i = tid; i < TG_SLOTS; i += 256) key[i] = 0u;
    for (uint32_t i = tid; i < TG_SLOTS * VALS; i += 256) val[i] = 0.0f;
    if (tid == 0) n_used = 0u;
  }
  // the slot of texel `idx`, taken if need be; TG_NONE: no room within TG_PROBES
  __device__ __forceinline__ uint32_t slot(uint32_t idx) {
    const uint32_t k = idx + 1u;
    uint32_t h = (k * 0x9e3779b1u) >> (32u - TG_SLOT_BITS);
    for (uint32_t p = 0; p < TG_PROBES; ++p) {
      const uint32_t old = atomicCAS(&key[h], 0u, k);
      if (old == 0u) used[atomicAdd(&n_used, 1u)] = h; // (each slot is taken once: n_used <= TG_SLOTS)
      if (old == 0u || old == k) return h;
      h = (h + 1u) & (TG_SLOTS - 1u);
    }
    return TG_NONE;
  }
  // v to value i of slot `s`; without a slot straight to memory, to channel ch of texel idx in `mem` (C channels a texel)
  __device__ __forceinline__ void add(uint32_t s, uint32_t i, float v, float *mem, uint32_t idx, uint32_t C, uint32_t ch) {
    if (s != TG_NONE) lds_add(&val[s * VALS + i], v);
    else global_add(mem + (size_t)idx * C + ch, v);
  }
  // step 4: the values of the chunk at channel c0 (nc of them) into memory, lanes in channel order within a texel, texel after
  // texel; at(idx): where texel idx lies in memory.  -> n_used, for release
  template <class At> __device__ __forceinline__ uint32_t flush(uint32_t tid, uint32_t c0, uint32_t nc, At at) {
    __syncthreads();
    const uint32_t n = n_used;
    for (uint32_t i = tid; i < n * VALS; i += 256) {
      const uint32_t s = used[i / VALS], e = i % VALS;
      const float v = val[s * VALS + e];
      val[s * VALS + e] = 0.0f;
      if (e < nc) global_add(at(key[s] - 1u) + c0 + e, v);
    }
    __syncthreads();
    return n;
  }
  // the tile's keys go; every thread has read n_used before the last flush's last barrier
  __device__ __forceinline__ void release(uint32_t tid, uint32_t n) {
    for (uint32_t i = tid; i < n; i += 256) key[used[i]] = 0u;
    if (tid == 0) n_used = 0u;
    __syncthreads();
  }
};
// THE CHANNEL LOOP'S PIECES
// gout of one channel for a thread's quad; words of pixels outside `mask` are loaded with their quad at most, never used
__device__ __forceinline__ void gout_quad(const float *p, bool whole, uint32_t mask, float4 &g) {
  if (whole) {
    g = *reinterpret_cast<const float4 *>(p);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (mask & (1u << k)) quad_at(g, k) = p[k];
  }
}
// one channel of the bilinear sample's derivatives: gi times d/dtx into au, times d/dty into av; -> the sample.  The products
// associate as the oracles have them
__device__ __forceinline__ float bilerp_chain(const SRZ_CAS float *p00, const SRZ_CAS float *p01, const SRZ_CAS float *p10, const SRZ_CAS float *p11,
                                              float tx, float ty, float gi, float &au, float &av) {
  const float t00 = *p00, t01 = *p01, t10 = *p10, t11 = *p11;
  const float top = fmaf_(tx, t01 - t00, t00), bot = fmaf_(tx, t11 - t10, t10);
  au = fmaf_(gi, fmaf_(ty, (t11 - t10) - (t01 - t00), t01 - t00), au);
  av = fmaf_(gi, bot - top, av);
  return fmaf_(ty, bot - top, top);
}
// the four corner-weight adds of one pixel and channel: w[corner] * gi into the corners' slots `s`, a corner without one straight
// to memory (TexelTable::add).  lw: the pixel's weight of this mip level
struct CornerW {
  float w00, w01, w10, w11;
};
__device__ __forceinline__ CornerW corner_weights(float tx, float ty) {
  return {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
}
__device__ __forceinline__ CornerW corner_weights(float tx, float ty, float lw) {
  const CornerW w = corner_weights(tx, ty);
  return {w.w00 * lw, w.w01 * lw, w.w10 * lw, w.w11 * lw};
}
template <class Table, class Tap>
__device__ __forceinline__ void corner_adds(Table &tb, const uint32_t *s, const Tap &p, const CornerW &w, float gi, uint32_t i, float *mem, uint32_t C,
                                            uint32_t ch) {
  tb.add(s[0], i, w.w00 * gi, mem, p.i00, C, ch);
  tb.add(s[1], i, w.w01 * gi, mem, p.i01, C, ch);
  tb.add(s[2], i, w.w10 * gi, mem, p.i10, C, ch);
  tb.add(s[3], i, w.w11 * gi, mem, p.i11, C, ch);
}
__global__ __launch_bounds__(256) void k_tex_grad(TexArgs a) {
  __shared__ TexelTable<TexArgs, ATTR_CHUNK> tb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ly = wave * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
  const uint32_t tpf = a.n_local_bands * a.tiles_x, n_items = a.n_frames * tpf;
  const uint32_t C = a.n_ch;
  const bool want_tex = a.gtex != nullptr, want_uv = a.out != nullptr;
  if (want_tex) {
    tb.init(tid);
    __syncthreads();
  }
  // workgroup b walks the frames f ≡ b mod 8 tile by tile (fewer than 8 frames: every 8th tile): an inline copy of pass_walk
  const uint32_t sub = blockIdx.x & 7u, step = gridDim.x >> 3;
  for (uint32_t j = blockIdx.x >> 3;; j += step) {
    uint32_t f, t;
    if (a.n_frames >= 8u) {
      f = sub + 8u * (j / tpf), t = j % tpf;
      if (f >= a.n_frames) break;
    } else {
      const uint32_t i = j * 8u + sub;
      if (i >= n_items) break;
      f = i / tpf, t = i % tpf;
    }
    const SRZ_CAS FrameDesc *fd = as_const(a.frames) + f;
    const uint32_t lb = t / a.tiles_x, tx = t % a.tiles_x;
    const TileRect rc = tile_rect(a, fd, f, lb, tx);
    const int W = fd->width;
    const int y = rc.ty0 + ly, x4 = rc.tx0 + lx4;
    const bool inside = y <= rc.ty1 && x4 <= rc.tx1; // (a thread outside the frame samples nothing, and still meets the barriers)
    const bool whole = (W & 3) == 0 && x4 + 3 <= rc.tx1;
    const bool fused = ((fd->flags | a.flags_or) & SRZ_FUSED_CLEAR) != 0;
    const size_t poff = (size_t)lb * BAND * (size_t)W + (size_t)ly * (size_t)W + (size_t)x4;
    const float *gg = a.gout + (size_t)f * a.gout_stride + poff;
    // ---- 1. owners, u and v, the taps
    TexTap tap[4] = {};
    uint32_t own, smp;
    tex_quad(a, fd, rc, f, poff, inside, whole, x4, tap, own, smp);
    const SRZ_CAS float *tex = as_const(a.tex) + (size_t)f * a.tex_frame_stride;
    float *gtex = a.gtex + (size_t)f * a.tex_frame_stride;
    // ---- 2. the slots of the sampled pixels' corners (two corners on one texel: one slot, both add)
    uint32_t slot[4][4] = {};
    if (want_tex) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (smp & (1u << k))
          slot[k][0] = tb.slot(tap[k].i00), slot[k][1] = tb.slot(tap[k].i01), slot[k][2] = tb.slot(tap[k].i10), slot[k][3] = tb.slot(tap[k].i11);
    }
    const auto at = [=](uint32_t idx) { return gtex + (size_t)idx * C; };
    float au[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t n_used = 0u;
    // ---- 3. the channels, ATTR_CHUNK at a time
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 g[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (smp != 0u) {
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
          if (i >= nc) break;
          gout_quad(gg + (size_t)(c0 + i) * rc.plane, whole, smp, g[i]);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(smp & (1u << k))) continue;
        if (want_uv) {
          const SRZ_CAS float *p00 = tex + (size_t)tap[k].i00 * C + c0, *p01 = tex + (size_t)tap[k].i01 * C + c0;
          const SRZ_CAS float *p10 = tex + (size_t)tap[k].i10 * C + c0, *p11 = tex + (size_t)tap[k].i11 * C + c0;
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) bilerp_chain(p00 + i, p01 + i, p10 + i, p11 + i, tap[k].tx, tap[k].ty, quad_at(g[i], k), au[k], av[k]);
        }
        if (want_tex) {
          const CornerW w = corner_weights(tap[k].tx, tap[k].ty);
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) corner_adds(tb, slot[k], tap[k], w, quad_at(g[i], k), i, gtex, C, c0 + i);
        }
      }
      if (want_tex) n_used = tb.flush(tid, c0, nc, at); // ---- 4. the table's values of this chunk into memory
    }
    if (want_tex) tb.release(tid, n_used);
    // ---- 5. du, dv: whole quads (fused clear, or four owners), else the owned pixels only; an owner that is not sampled: (0, 0)
    if (want_uv && inside && (own != 0u || fused)) {
      float4 du = make_float4(0.f, 0.f, 0.f, 0.f), dv = du;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (smp & (1u << k)) {
          quad_at(du, k) = tap[k].in_x ? au[k] * (float)a.tex_w : 0.0f;
          quad_at(dv, k) = tap[k].in_y ? av[k] * (float)a.tex_h : 0.0f;
        }
      float *go = rc.out0 + (size_t)ly * (size_t)W + (size_t)x4;
      if (fused || own == 15u) {
        quad_store(go, rc.plane, {du, dv}, whole, x4, rc.tx1);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (own & (1u << k)) go[k] = quad_at(du, k), go[rc.plane + k] = quad_at(dv, k);
      }
    }
  }
}

// ================================================================================================================
// k_cube — A CALLER'S CUBE MAP LOOKED UP BY DIRECTION OVER A VISIBILITY BUFFER (srz_frameset_texture_cube, include/srz.h states the
// rule): a float cube [frame][face][row][column][channel], faces n x n, sampled bilinearly and seamlessly at the direction planes
// interpolate wrote for a three-channel attribute.  k_tex's shape on the passes' helpers: pass_walk's XCD-ordered walk, 4 pixels of a
// row per thread, one 16-byte id load (quad_ids), the three direction words only for a quad with an owner, every plane leaves
// through quad_store_owned; no LDS, no barrier.  The face, the two fractions and the four RESOLVED texel indices of a pixel (a
// corner one step outside its face lands on the neighbouring face: cube_texel) are formed once, global over the cube — (face * n +
// row) * n + column < 6 * 2^28 —; the wave-uniform channel loop then gathers 4 * nc floats per sampled pixel, ATTR_CHUNK channels at
// a time, the tail masked: tex_quad's arithmetic from there on.
// Every float -> int conversion follows s, t in [-1, 1] (the IEEE division of a component by the largest), so x0, y0 lie in
// [-1, n - 1]; the integer clamp behind it never changes a value and keeps every index inside the cube whatever the division did.
// ================================================================================================================
struct CubeFace {
  float s, t, inv; // the in-face coordinates and 1 / |major component|
  uint32_t major;  // the major axis, bit 2: its component is positive
};
struct CubeTap {
  uint32_t i00, i01, i10, i11; // resolved texels (face * n + row) * n + column of the corners (y0, x0), (y0, x1), (y1, x0), (y1, x1)
  float tx, ty;
  CubeFace f;                  // the backward's
};
// srz_frameset_texture_cube_grad's chain from au, av at one level (half_n = 0.5f * (float)N of that level) to the direction
__device__ __forceinline__ void cube_gdir(const CubeFace &c, float au, float av, float half_n, float (&g)[3]) {
  const float gs = au * half_n, gt = av * half_n, inv = c.inv;
  const float g_sc = gs * inv, g_tc = gt * inv, g_ma = -(fmaf_(gs, c.s, gt * c.t) * inv);
  const uint32_t m = c.major & 3u;
  const bool pos = (c.major & 4u) != 0u;
  const float g_m = pos ? g_ma : -g_ma;
  // su, sv of the face, undone: +X (-z, -y)  -X (z, -y)  +Y (x, z)  -Y (x, -z)  +Z (x, -y)  -Z (-x, -y)
  g[0] = m == 0u ? g_m : m == 1u ? g_sc : (pos ? g_sc : -g_sc);
  g[1] = m == 1u ? g_m : -g_tc;
  g[2] = m == 0u ? (pos ? -g_sc : g_sc) : m == 1u ? (pos ? g_tc : -g_tc) : g_m;
}
// the seam rows of a face, one byte per side (x = -1, x = n, y = -1, y = n): the neighbour face | which of its indices is fixed
// (8: row, else column) | fixed at n - 1 (16, else 0) | the index along the edge mirrored (32).  tests/cube_ref.c holds the same
// 24 rows unpacked; tests/test_cube_ref.py derives them from the faces' axes
__device__ __forceinline__ uint32_t cube_seams(uint32_t face) {
  return face == 0u ? 0x13320514u : face == 1u ? 0x23020415u : face == 2u ? 0x0c2d2809u : face == 3u ? 0x3d1c1839u
       : face == 4u ? 0x0b1a0011u : 0x3b2a0110u;
}
// texel (x, y) of `face`, x and y in [-1, n] -> its index in the cube; one outside in both axes: the row clamped first, then across in x
__device__ __forceinline__ uint32_t cube_texel(uint32_t face, uint32_t seams, int x, int y, int n) {
  const bool ox = (unsigned)x >= (unsigned)n, oy = (unsigned)y >= (unsigned)n;
  if (ox && oy) y = y < 0 ? 0 : n - 1;
  uint32_t g = face;
  int rx = x, ry = y;
  if (ox || oy) {
    const uint32_t side = ox ? (x < 0 ? 0u : 1u) : (y < 0 ? 2u : 3u);
    const int along = ox ? y : x;
    const uint32_t r = (seams >> (8u * side)) & 0xffu;
    const int al = (r & 32u) ? n - 1 - along : along, e = (r & 16u) ? n - 1 : 0;
    g = r & 7u, rx = (r & 8u) ? al : e, ry = (r & 8u) ? e : al;
  }
  return (g * (uint32_t)n + (uint32_t)ry) * (uint32_t)n + (uint32_t)rx;
}
// one axis of the rule: in-face coordinate s in [-1, 1] over n texels -> the first texel coordinate, in [-1, n - 1], and the fraction
__device__ __forceinline__ void cube_axis(float s, int n, int &i0, float &t) {
  const float u = fmaf_(s, 0.5f, 0.5f), fx = u * (float)n - 0.5f;
  const float f0 = __builtin_floorf(fx);
  t = fx - f0;
  i0 = max(-1, min((int)f0, n - 1)); // (never changes a value: fx lies in [-0.5, n - 0.5])
}
// The tap of one direction in its two halves, so that the passes over a cube's mip pyramid share them: cube_face — what does not
// depend on the face size: the major axis (bit 2: its component is positive), the in-face coordinates s, t and 1 / |major
// component|; false: not sampled (a component not finite, or the zero vector) — and cube_corners — the fractions and the four
// resolved texels of that point on faces of N x N texels.
__device__ __forceinline__ bool cube_face(float dx, float dy, float dz, float &s, float &t, float &inv, uint32_t &major) {
  const float ax = __builtin_fabsf(dx), ay = __builtin_fabsf(dy), az = __builtin_fabsf(dz);
  if (!tex_finite(dx) || !tex_finite(dy) || !tex_finite(dz)) return false;
  if (__builtin_fmaxf(ax, __builtin_fmaxf(ay, az)) == 0.0f) return false;
  const uint32_t m = (ax >= ay && ax >= az) ? 0u : (ay >= az ? 1u : 2u);
  const float mc = m == 0u ? dx : m == 1u ? dy : dz;
  const bool pos = mc > 0.0f;
  const float ma = __builtin_fabsf(mc);
  // the components su and sv name, signed: +X (-z, -y)  -X (z, -y)  +Y (x, z)  -Y (x, -z)  +Z (x, -y)  -Z (-x, -y)
  const float sc = m == 0u ? (pos ? -dz : dz) : m == 1u ? dx : (pos ? dx : -dx);
  const float tc = m == 1u ? (pos ? dz : -dz) : -dy;
  s = sc / ma, t = tc / ma, inv = 1.0f / ma, major = m | (pos ? 4u : 0u);
  return true;
}
__device__ __forceinline__ void cube_corners(uint32_t major, float s, float t, uint32_t N, uint32_t &i00, uint32_t &i01, uint32_t &i10,
                                             uint32_t &i11, float &tx, float &ty) {
  const uint32_t face = 2u * (major & 3u) + ((major & 4u) ? 0u : 1u), seams = cube_seams(face);
  int x0, y0;
  cube_axis(s, (int)N, x0, tx);
  cube_axis(t, (int)N, y0, ty);
  i00 = cube_texel(face, seams, x0, y0, (int)N), i01 = cube_texel(face, seams, x0 + 1, y0, (int)N);
  i10 = cube_texel(face, seams, x0, y0 + 1, (int)N), i11 = cube_texel(face, seams, x0 + 1, y0 + 1, (int)N);
}
// the tap of one direction; false: not sampled
__device__ __forceinline__ bool cube_tap(float dx, float dy, float dz, uint32_t N, CubeTap &p) {
  if (!cube_face(dx, dy, dz, p.f.s, p.f.t, p.f.inv, p.f.major)) return false;
  cube_corners(p.f.major, p.f.s, p.f.t, N, p.i00, p.i01, p.i10, p.i11, p.tx, p.ty);
  return true;
}
// what k_cube and k_cube_grad do alike in front of their channel loops: the owners, the directions of a quad with an owner, the
// taps of the sampled pixels -> `own` and `smp`, one bit per pixel
__device__ __forceinline__ void cube_quad(const CubeArgs &a, const PassTile &t, CubeTap (&tap)[4], uint32_t &own, uint32_t &smp) {
  uint32_t id[4];
  own = quad_ids(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id), smp = 0u;
  if (own == 0u) return;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 d[3] = {zero4, zero4, zero4};
  quad_load(a.dir + (size_t)t.f * a.dir_stride + t.poff, t.rc.plane, d, t.whole, t.x4, t.rc.tx1);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!(own & (1u << k))) continue;
    if (cube_tap(quad_at(d[0], k), quad_at(d[1], k), quad_at(d[2], k), a.n, tap[k])) smp |= 1u << k;
  }
}
__global__ __launch_bounds__(256) void k_cube(CubeArgs a) {
  const uint32_t C = a.n_ch;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const TileRect &rc = t.rc;
    const bool fused = t.fused(a.flags_or);
    // ---- 1. owners, directions, the taps
    CubeTap tap[4] = {};
    uint32_t own, smp;
    cube_quad(a, t, tap, own, smp);
    if (own == 0u && !fused) return;
    const SRZ_CAS float *tex = as_const(a.tex) + (size_t)t.f * a.tex_frame_stride;
    // ---- 2. the channels, ATTR_CHUNK at a time (k_tex's loop)
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 q[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) q[i] = make_float4(0.f, 0.f, 0.f, 0.f); // nobody, and an owner that is not sampled: zeros
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(smp & (1u << k))) continue;
        const SRZ_CAS float *p00 = tex + (size_t)tap[k].i00 * C + c0, *p01 = tex + (size_t)tap[k].i01 * C + c0;
        const SRZ_CAS float *p10 = tex + (size_t)tap[k].i10 * C + c0, *p11 = tex + (size_t)tap[k].i11 * C + c0;
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
          if (i < nc) {
            const float t00 = p00[i], t01 = p01[i], t10 = p10[i], t11 = p11[i];
            const float top = fmaf_(tap[k].tx, t01 - t00, t00), bot = fmaf_(tap[k].tx, t11 - t10, t10);
            quad_at(q[i], k) = fmaf_(tap[k].ty, bot - top, top);
          }
      }
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
        if (i >= nc) break;
        quad_store_owned(t.out + (size_t)(c0 + i) * rc.plane, t, {q[i]}, fused, own);
      }
    }
  });
}

// ================================================================================================================
// k_cube_grad — THE BACKWARD OF k_cube (srz_frameset_texture_cube_grad): per sampled pixel and channel, four adds w[corner] * gout
// into the cube's gradient (gtex) at the RESOLVED texels — a tile that straddles a cube edge adds into both faces —, and the
// gradient with respect to the direction (gdir: k_tex_grad's au, av chains, then the chain through s = sc / ma, t = tc / ma; from
// registers, no atomics).  k_tex_grad's structure on the passes' helpers (pass_walk<true>: every thread of the workgroup reaches
// every barrier, one outside the frame samples nothing): the tile's open-addressed table of distinct texels in LDS (TexelTable,
// keyed on the cube-wide texel index), the slots found once in front of the channel loop, LDS float adds per chunk, the dense
// flush with global_atomic_add_f32, a corner without a slot adding straight to memory.
// ================================================================================================================
__global__ __launch_bounds__(256) void k_cube_grad(CubeArgs a) {
  __shared__ TexelTable<CubeArgs, ATTR_CHUNK> tb;
  const uint32_t tid = threadIdx.x;
  const uint32_t C = a.n_ch;
  const bool want_tex = a.gtex != nullptr, want_dir = a.out != nullptr;
  if (want_tex) {
    tb.init(tid);
    __syncthreads();
  }
  pass_walk<true>(a, [&](const PassTile &t) { // (a thread outside the frame owns nothing, and still meets the barriers)
    const TileRect &rc = t.rc;
    const bool fused = t.fused(a.flags_or);
    const float *gg = a.gout + (size_t)t.f * a.gout_stride + t.poff;
    // ---- 1. owners, directions, the taps
    CubeTap tap[4] = {};
    uint32_t own, smp;
    cube_quad(a, t, tap, own, smp);
    const SRZ_CAS float *tex = as_const(a.tex) + (size_t)t.f * a.tex_frame_stride;
    float *gtex = a.gtex + (size_t)t.f * a.tex_frame_stride;
    // ---- 2. the slots of the sampled pixels' corners (two corners on one texel: one slot, both add)
    uint32_t slot[4][4] = {};
    if (want_tex) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (smp & (1u << k))
          slot[k][0] = tb.slot(tap[k].i00), slot[k][1] = tb.slot(tap[k].i01), slot[k][2] = tb.slot(tap[k].i10), slot[k][3] = tb.slot(tap[k].i11);
    }
    const auto at = [=](uint32_t idx) { return gtex + (size_t)idx * C; };
    float au[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t n_used = 0u;
    // ---- 3. the channels, ATTR_CHUNK at a time
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 g[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (smp != 0u) {
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
          if (i >= nc) break;
          gout_quad(gg + (size_t)(c0 + i) * rc.plane, t.whole, smp, g[i]);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(smp & (1u << k))) continue;
        if (want_dir) {
          const SRZ_CAS float *p00 = tex + (size_t)tap[k].i00 * C + c0, *p01 = tex + (size_t)tap[k].i01 * C + c0;
          const SRZ_CAS float *p10 = tex + (size_t)tap[k].i10 * C + c0, *p11 = tex + (size_t)tap[k].i11 * C + c0;
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) bilerp_chain(p00 + i, p01 + i, p10 + i, p11 + i, tap[k].tx, tap[k].ty, quad_at(g[i], k), au[k], av[k]);
        }
        if (want_tex) {
          const CornerW w = corner_weights(tap[k].tx, tap[k].ty);
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) corner_adds(tb, slot[k], tap[k], w, quad_at(g[i], k), i, gtex, C, c0 + i);
        }
      }
      if (want_tex) n_used = tb.flush(tid, c0, nc, at); // ---- 4. the table's values of this chunk into memory
    }
    if (want_tex) tb.release(tid, n_used);
    // ---- 5. the direction's gradient: whole quads (fused clear, or four owners), else the owned pixels only; an owner that is not
    // sampled: (0, 0, 0)
    if (want_dir && t.inside && (own != 0u || fused)) {
      const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
      float4 gd[3] = {zero4, zero4, zero4};
      const float half_n = 0.5f * (float)a.n;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (smp & (1u << k)) {
          float gk[3];
          cube_gdir(tap[k].f, au[k], av[k], half_n, gk);
          quad_at(gd[0], k) = gk[0], quad_at(gd[1], k) = gk[1], quad_at(gd[2], k) = gk[2];
        }
      quad_store_owned(t.out, t, gd, fused, own);
    }
  });
}

// ================================================================================================================
// k_light — BLINN-PHONG UNDER POINT LIGHTS OVER A VISIBILITY BUFFER, FOR CALLER DATA (srz_frameset_light, include/srz.h states the
// rule): the normal, position and albedo planes interpolate / texture / gbuffer wrote, a parameter frame (eye, ka, ks, then the
// lights) and a host exponent -> three colour planes.  Nothing of the built-in shaders: true 1 / r² attenuation, a normalised half
// vector, no clamp.  k_cube's shape on the passes' helpers: pass_walk, quad_ids, the three or four plane triples of a quad with an
// owner in 16-byte loads, quad_store_owned; no LDS, no barrier.  The parameter frame is wave-uniform: scalar loads.
// light_px (what a lit pixel keeps across the lights) and light_term (one light at one pixel) are the rule's text; k_light and
// k_light_grad both go through them, so the backward differentiates the very words the forward computed.
// ================================================================================================================
struct LightPx {
  float N[3], P[3], Vd[3];
  float inl, iv;
  bool view;
};
struct LightTerm {
  float Lv[3], Ld[3], H[3], E[3];
  float ir, att, ih, cdr, cd, csr, cs, sp;
  bool spec;
};
__device__ __forceinline__ float l_dot(const float (&a)[3], const float (&b)[3]) { return fmaf_(a[0], b[0], fmaf_(a[1], b[1], a[2] * b[2])); }
__device__ __forceinline__ bool l_pos(float x) { return x > 0.0f && x < __builtin_inff(); }
__device__ __forceinline__ float l_rsqrt(float x) { return 1.0f / __builtin_sqrtf(x); } // (two roundings: the IEEE root, the IEEE division)
// false: not lit (the normal's squared length is 0, not finite or NaN)
__device__ __forceinline__ bool light_px(const float (&n)[3], const float (&P)[3], const SRZ_CAS float *par, LightPx &px) {
  const float nn = l_dot(n, n);
  if (!l_pos(nn)) return false;
  px.inl = l_rsqrt(nn);
  float V[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) px.N[i] = n[i] * px.inl, px.P[i] = P[i], V[i] = par[i] - P[i];
  const float vv = l_dot(V, V);
  px.view = l_pos(vv);
  px.iv = px.view ? l_rsqrt(vv) : 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) px.Vd[i] = px.view ? V[i] * px.iv : 0.0f;
  return true;
}
// lp: the light's {pos[3], intensity[3]}.  false: the light is skipped at this pixel
__device__ __forceinline__ bool light_term(const LightPx &px, const SRZ_CAS float *lp, uint32_t p, LightTerm &t) {
#pragma unroll
  for (int i = 0; i < 3; ++i) t.Lv[i] = lp[i] - px.P[i];
  const float r2 = l_dot(t.Lv, t.Lv);
  if (!l_pos(r2)) return false;
  t.ir = l_rsqrt(r2), t.att = 1.0f / r2;
  float Hs[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) t.Ld[i] = t.Lv[i] * t.ir, Hs[i] = t.Ld[i] + px.Vd[i], t.H[i] = 0.0f, t.E[i] = lp[3 + i] * t.att;
  t.cdr = l_dot(px.N, t.Ld), t.cd = t.cdr > 0.0f ? t.cdr : 0.0f;
  const float h2 = l_dot(Hs, Hs);
  t.spec = px.view && h2 > 0.0f;
  t.ih = t.csr = t.cs = t.sp = 0.0f;
  if (t.spec) {
    t.ih = l_rsqrt(h2);
#pragma unroll
    for (int i = 0; i < 3; ++i) t.H[i] = Hs[i] * t.ih;
    t.csr = l_dot(px.N, t.H), t.cs = t.csr > 0.0f ? t.csr : 0.0f;
    t.sp = pow_int_cr(t.cs, p);
  }
  return true;
}
// what k_light and k_light_grad do alike in front of the lights: the owners, the planes of a quad with an owner, the lit pixels'
// LightPx -> `own` and `lit`, one bit per pixel; kd: ones without an albedo buffer
__device__ __forceinline__ void light_quad(const LightArgs &a, const PassTile &t, const SRZ_CAS float *par, LightPx (&px)[4], float4 (&kd)[3],
                                           uint32_t &own, uint32_t &lit) {
  uint32_t id[4];
  own = quad_ids(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id), lit = 0u;
  kd[0] = kd[1] = kd[2] = make_float4(1.f, 1.f, 1.f, 1.f);
  if (own == 0u) return;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 n[3] = {zero4, zero4, zero4}, P[3] = {zero4, zero4, zero4};
  const size_t off = (size_t)t.f * a.frame_stride + t.poff;
  quad_load(a.nrm + off, t.rc.plane, n, t.whole, t.x4, t.rc.tx1);
  quad_load(a.pos + off, t.rc.plane, P, t.whole, t.x4, t.rc.tx1);
  if (a.kd) quad_load(a.kd + off, t.rc.plane, kd, t.whole, t.x4, t.rc.tx1);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!(own & (1u << k))) continue;
    const float nk[3] = {quad_at(n[0], k), quad_at(n[1], k), quad_at(n[2], k)}, Pk[3] = {quad_at(P[0], k), quad_at(P[1], k), quad_at(P[2], k)};
    if (light_px(nk, Pk, par, px[k])) lit |= 1u << k;
  }
}
__global__ __launch_bounds__(256) void k_light(LightArgs a) {
  const uint32_t L = a.n_lights;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool fused = t.fused(a.flags_or);
    const SRZ_CAS float *par = as_const(a.par) + (size_t)t.f * a.par_stride;
    LightPx px[4];
    float4 kd[3];
    uint32_t own, lit;
    light_quad(a, t, par, px, kd, own, lit);
    if (own == 0u && !fused) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 o[3] = {zero4, zero4, zero4}; // nobody, and an owner that is not lit: zeros
    if (lit != 0u) {
      const float ka[3] = {par[3], par[4], par[5]}, ks[3] = {par[6], par[7], par[8]};
      for (uint32_t l = 0; l < L; ++l) {
        const SRZ_CAS float *lp = par + 9u + 6u * l;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!(lit & (1u << k))) continue;
          LightTerm lt;
          if (!light_term(px[k], lp, a.p, lt)) continue;
#pragma unroll
          for (int c = 0; c < 3; ++c)
            quad_at(o[c], k) = quad_at(o[c], k) + (quad_at(kd[c], k) * fmaf_(lt.E[c], lt.cd, ka[c] * lp[3 + c]) + (ks[c] * lt.E[c]) * lt.sp);
        }
      }
    }
    quad_store_owned(t.out, t, o, fused, own);
  });
}

// ================================================================================================================
// k_light_grad — THE BACKWARD OF k_light (srz_frameset_light_grad): gout -> the gradient planes of the normal, the position and the
// albedo (per pixel, from registers, deterministic), and, WANT_PAR, the gradient of the parameter frame: every entry is the sum of a
// per-pixel float32 term over the frame's owned pixels, and this kernel leaves that sum per TILE in work[frame][tile][K], reduced in a
// FIXED tree (include/srz.h states it): a thread's four pixels left to right; the wave's 64 lanes by the xor butterfly 32, 16, 8, 4, 2,
// 1 (every lane ends with the same word: float addition commutes); the four waves through LDS, ((w0 + w1) + w2) + w3; ordinary
// vector stores, no atomics.  k_light_fold sums the tiles.  The lights are the OUTER loop: a light's six lane sums are reduced and put
// into LDS as its iteration ends, so a lane holds 6 of the up to 57 entries at a time, not all of them; eye, ka and ks — sums over
// the lights — follow after the loop.  pass_walk<true>'s shape through pass_tiles / pass_tile (the tile's index is the work row):
// every thread of the workgroup reaches every shuffle and barrier, one outside the frame owns nothing.  A tile without a lit pixel
// (one barrier tells) writes +0 partials and skips the lights.  The planes-only build has no LDS, no shuffle and no barrier.
// ================================================================================================================
__device__ __forceinline__ float light_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}
template <bool WANT_PAR> __global__ __launch_bounds__(256) void k_light_grad(LightArgs a) {
  __shared__ float s_part[WANT_PAR ? 4 : 1][WANT_PAR ? SRZ_LIGHT_PAR(SRZ_LIGHT_MAX) : 1];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t L = a.n_lights, K = SRZ_LIGHT_PAR(L), tpf = a.n_local_bands * a.tiles_x, p = a.p;
  const float pf = (float)p;
  pass_tiles(a, [&](uint32_t f, uint32_t ti) {
    const PassTile t = pass_tile(a, f, ti);
    const bool fused = t.fused(a.flags_or);
    const SRZ_CAS float *par = as_const(a.par) + (size_t)f * a.par_stride;
    const size_t off = (size_t)f * a.frame_stride + t.poff;
    // ---- 1. owners, planes, the lit pixels; gout of a quad with a lit pixel
    LightPx px[4];
    float4 kd[3];
    uint32_t own, lit;
    light_quad(a, t, par, px, kd, own, lit);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (WANT_PAR) {
      // a tile without a lit pixel (most tiles of a sparse frame): its partials are the empty sums, +0, what the tree below gives too,
      // without the shuffles; its planes are zeros where they are written at all
      if (!__syncthreads_or(lit != 0u)) {
        if (t.inside && (own != 0u || fused)) {
          const float4 z[3] = {zero4, zero4, zero4};
          if (a.gnrm) quad_store_owned(a.gnrm + off, t, z, fused, own);
          if (a.gpos) quad_store_owned(a.gpos + off, t, z, fused, own);
          if (a.gkd) quad_store_owned(a.gkd + off, t, z, fused, own);
        }
        if (tid < K) a.work[((size_t)f * tpf + ti) * K + tid] = 0.0f;
        return;
      }
    }
    float4 g[3] = {zero4, zero4, zero4};
    if (lit != 0u) quad_load(a.gout + off, t.rc.plane, g, t.whole, t.x4, t.rc.tx1);
    float4 gN[3] = {zero4, zero4, zero4}, gVd[3] = {zero4, zero4, zero4}, gP[3] = {zero4, zero4, zero4}, gkd[3] = {zero4, zero4, zero4};
    float4 tka[3] = {zero4, zero4, zero4}, tks[3] = {zero4, zero4, zero4};
    const float ka[3] = {par[3], par[4], par[5]}, ks[3] = {par[6], par[7], par[8]};
    // ---- 2. the lights
    for (uint32_t l = 0; l < L; ++l) {
      const SRZ_CAS float *lp = par + 9u + 6u * l;
      const float I[3] = {lp[3], lp[4], lp[5]};
      float tl[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; // this lane's sums of the light's terms: pos[3], intensity[3]
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(lit & (1u << k))) continue;
        LightTerm lt;
        if (!light_term(px[k], lp, p, lt)) continue;
        float gk[3], gs[3], ge[3], gLd[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float gc = quad_at(g[c], k), kc = quad_at(kd[c], k);
          gk[c] = gc * kc, gs[c] = gc * ks[c];
          quad_at(gkd[c], k) = quad_at(gkd[c], k) + gc * fmaf_(lt.E[c], lt.cd, ka[c] * I[c]);
          if (WANT_PAR) {
            quad_at(tka[c], k) = quad_at(tka[c], k) + gk[c] * I[c];
            quad_at(tks[c], k) = quad_at(tks[c], k) + (gc * lt.E[c]) * lt.sp;
            tl[3 + c] = tl[3 + c] + gc * (kc * fmaf_(lt.att, lt.cd, ka[c]) + (ks[c] * lt.att) * lt.sp);
          }
          ge[c] = gc * fmaf_(kc, lt.cd, ks[c] * lt.sp);
        }
        const float g_cd = lt.cdr > 0.0f ? l_dot(gk, lt.E) : 0.0f, g_sp = l_dot(gs, lt.E), g_att = l_dot(ge, I);
#pragma unroll
        for (int c = 0; c < 3; ++c) gLd[c] = g_cd * px[k].N[c], quad_at(gN[c], k) = quad_at(gN[c], k) + g_cd * lt.Ld[c];
        if (lt.spec && lt.csr > 0.0f) {
          const float g_cs = g_sp * (pf * pow_int_cr(lt.cs, p - 1u));
          float gH[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) gH[c] = g_cs * px[k].N[c], quad_at(gN[c], k) = quad_at(gN[c], k) + g_cs * lt.H[c];
          const float d = l_dot(gH, lt.H);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float gHs = (gH[c] - lt.H[c] * d) * lt.ih;
            gLd[c] = gLd[c] + gHs, quad_at(gVd[c], k) = quad_at(gVd[c], k) + gHs;
          }
        }
        const float d = l_dot(gLd, lt.Ld), two_g_r2 = 2.0f * (-((g_att * lt.att) * lt.att));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float gLv = fmaf_(lt.Lv[c], two_g_r2, (gLd[c] - lt.Ld[c] * d) * lt.ir);
          tl[c] = tl[c] + gLv, quad_at(gP[c], k) = quad_at(gP[c], k) - gLv;
        }
      }
      if (WANT_PAR) { // (every lane of the workgroup is here: the walk and the light count are uniform)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const float v = light_wave_sum(tl[j]);
          if (lane == 0u) s_part[wave][9u + 6u * l + (uint32_t)j] = v;
        }
      }
    }
    // ---- 3. behind the lights: the view direction's and the normal's normalisations; the eye's terms
    float te[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; // this lane's sums of eye[3], ka[3], ks[3]
    float4 gn[3] = {zero4, zero4, zero4};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(lit & (1u << k))) continue;
      if (px[k].view) {
        const float v[3] = {quad_at(gVd[0], k), quad_at(gVd[1], k), quad_at(gVd[2], k)};
        const float d = l_dot(v, px[k].Vd);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float gV = (v[c] - px[k].Vd[c] * d) * px[k].iv;
          te[c] = te[c] + gV, quad_at(gP[c], k) = quad_at(gP[c], k) - gV;
        }
      }
      const float v[3] = {quad_at(gN[0], k), quad_at(gN[1], k), quad_at(gN[2], k)};
      const float d = l_dot(v, px[k].N);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        quad_at(gn[c], k) = (v[c] - px[k].N[c] * d) * px[k].inl;
        te[3 + c] = te[3 + c] + quad_at(tka[c], k), te[6 + c] = te[6 + c] + quad_at(tks[c], k);
      }
    }
    // ---- 4. the planes: whole quads (fused clear, or four owners), else the owned pixels only; an owner that is not lit: zeros
    if (t.inside && (own != 0u || fused)) {
      if (a.gnrm) quad_store_owned(a.gnrm + off, t, gn, fused, own);
      if (a.gpos) quad_store_owned(a.gpos + off, t, gP, fused, own);
      if (a.gkd) quad_store_owned(a.gkd + off, t, gkd, fused, own);
    }
    // ---- 5. the tile's K partial sums
    if (WANT_PAR) {
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const float v = light_wave_sum(te[j]);
        if (lane == 0u) s_part[wave][j] = v;
      }
      __syncthreads();
      if (tid < K) a.work[((size_t)f * tpf + ti) * K + tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
      __syncthreads(); // s_part is the next tile's too
    }
  });
}
// k_light_fold — dst[o][k] = src[o][0][k] + src[o][1][k] + ... in that order from +0, k < K: a frame's tiles in tile order (o: the
// frame), then, for a parameter frame every frame shares, the frames in frame order (o: 0).  A workgroup of 64 per row of dst.
__global__ __launch_bounds__(64) void k_light_fold(const float *src, float *dst, uint32_t n_inner, uint32_t K) {
  const uint32_t k = threadIdx.x;
  if (k >= K) return;
  const float *p = src + (size_t)blockIdx.x * n_inner * K + k;
  float s = 0.0f;
  uint32_t i = 0;
  for (; i + 16u <= n_inner; i += 16u) { // sixteen loads in flight, then the adds in order: the sum is the serial one
    float v[16];
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) v[j] = p[(size_t)(i + j) * K];
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) s = s + v[j];
  }
  for (; i < n_inner; ++i) s = s + p[(size_t)i * K];
  dst[(size_t)blockIdx.x * K + k] = s;
}

// ================================================================================================================
// k_background — THE ENVIRONMENT BEHIND A VISIBILITY BUFFER, BY VIEW RAY (srz_frameset_background, include/srz.h states the rule):
// k_cube's body with three differences.  The direction is COMPUTED, not loaded: d = r0 + x rx + y ry at the pixel's integer corner
// (x, y), two fmafs per component, from the frame's nine ray words — wave-uniform, read through the constant address space: scalar
// loads, as k_light reads its parameter frame.  The pixel mask is INVERTED: the pass's pixels are those quad_ids calls nobody
// (SRZ_BG_NOBODY), or every pixel of the frame (SRZ_BG_ALL: the ids are not loaded, vis may be null).  And the owned pixels are the
// ones that keep their words: zeros with the fused clear, untouched without it — quad_store_owned with the pass's pixels as its
// mask.  A thread none of whose pixels is the pass's, without the fused clear, does nothing after its id load.  From the direction
// on everything is k_cube's: cube_tap, the channel loop, ATTR_CHUNK channels at a time.  No LDS, no barrier.
// ================================================================================================================
// what k_background and k_background_grad do alike in front of their channel loops: the pass's pixels of the quad, their directions
// and the taps of the sampled ones -> `px` and `smp`, one bit per pixel
__device__ __forceinline__ void bg_quad(const BgArgs &a, const PassTile &t, const SRZ_CAS float *ray, CubeTap (&tap)[4], float (&gx)[4],
                                        uint32_t &px, uint32_t &smp) {
  px = smp = 0u;
  uint32_t in = 0u;
  if (t.inside) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (t.x4 + k <= t.rc.tx1) in |= 1u << k;
  }
  if (a.where == SRZ_BG_ALL) {
    px = in;
  } else {
    uint32_t id[4];
    px = in & ~quad_ids(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id);
  }
  if (px == 0u) return;
  const float r0[3] = {ray[0], ray[1], ray[2]}, rx[3] = {ray[3], ray[4], ray[5]}, ry[3] = {ray[6], ray[7], ray[8]};
  const float fy = (float)t.y;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    gx[k] = (float)(t.x4 + k);
    if (!(px & (1u << k))) continue;
    const float dx = fmaf_(fy, ry[0], fmaf_(gx[k], rx[0], r0[0])), dy = fmaf_(fy, ry[1], fmaf_(gx[k], rx[1], r0[1]));
    const float dz = fmaf_(fy, ry[2], fmaf_(gx[k], rx[2], r0[2]));
    if (cube_tap(dx, dy, dz, a.n, tap[k])) smp |= 1u << k;
  }
}
__global__ __launch_bounds__(256) void k_background(BgArgs a) {
  const uint32_t C = a.n_ch;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const TileRect &rc = t.rc;
    const bool fused = t.fused(a.flags_or);
    // ---- 1. the pass's pixels, their directions, the taps
    CubeTap tap[4] = {};
    float gx[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t px, smp;
    bg_quad(a, t, as_const(a.ray) + (size_t)t.f * a.ray_stride, tap, gx, px, smp);
    if (px == 0u && !fused) return;
    const SRZ_CAS float *tex = as_const(a.tex) + (size_t)t.f * a.tex_frame_stride;
    // ---- 2. the channels, ATTR_CHUNK at a time (k_cube's loop)
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 q[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) q[i] = make_float4(0.f, 0.f, 0.f, 0.f); // an owner under the fused clear, and a pixel that is not sampled: zeros
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(smp & (1u << k))) continue;
        const SRZ_CAS float *p00 = tex + (size_t)tap[k].i00 * C + c0, *p01 = tex + (size_t)tap[k].i01 * C + c0;
        const SRZ_CAS float *p10 = tex + (size_t)tap[k].i10 * C + c0, *p11 = tex + (size_t)tap[k].i11 * C + c0;
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
          if (i < nc) {
            const float t00 = p00[i], t01 = p01[i], t10 = p10[i], t11 = p11[i];
            const float top = fmaf_(tap[k].tx, t01 - t00, t00), bot = fmaf_(tap[k].tx, t11 - t10, t10);
            quad_at(q[i], k) = fmaf_(tap[k].ty, bot - top, top);
          }
      }
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
        if (i >= nc) break;
        quad_store_owned(t.out + (size_t)(c0 + i) * rc.plane, t, {q[i]}, fused, px); // (the mask: the pass's pixels)
      }
    }
  });
}

// ================================================================================================================
// k_background_grad — THE BACKWARD OF k_background (srz_frameset_background_grad): k_cube_grad's table and flush for the cube's
// gradient (the tile's open-addressed table of distinct texels in LDS, the dense flush with float atomics, a corner without a slot
// adding straight to memory) together with k_light_grad's per-tile partials for the ray block's:
// per sampled pixel gdir exactly as k_cube_grad forms it, its nine terms gdir_c, x gdir_c, y gdir_c summed in the FIXED tree — a
// thread's four pixels left to right from +0, the xor butterfly, the four waves through LDS, a row of 9 per tile in work;
// k_light_fold sums the tiles and, for a shared block, the frames.  pass_tiles / pass_tile as in k_light_grad (the tile's index is
// the work row): every thread of the workgroup reaches every shuffle and barrier, one outside the frame samples nothing.  WANT_RAY:
// a tile without a sampled pixel (one barrier tells) writes +0 partials and skips the rest.  The build without WANT_RAY has no
// partials, no shuffle and no barrier beyond the table's.
// ================================================================================================================
template <bool WANT_RAY> __global__ __launch_bounds__(256) void k_background_grad(BgArgs a) {
  __shared__ TexelTable<BgArgs, ATTR_CHUNK> tb;
  __shared__ float s_part[WANT_RAY ? 4 : 1][WANT_RAY ? 9 : 1];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t C = a.n_ch, tpf = a.n_local_bands * a.tiles_x;
  const bool want_tex = a.gtex != nullptr;
  if (want_tex) {
    tb.init(tid);
    __syncthreads();
  }
  pass_tiles(a, [&](uint32_t f, uint32_t ti) {
    const PassTile t = pass_tile(a, f, ti);
    const TileRect &rc = t.rc;
    const float *gg = a.gout + (size_t)f * a.gout_stride + t.poff;
    // ---- 1. the pass's pixels, their directions, the taps
    CubeTap tap[4] = {};
    float gx[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t px, smp;
    bg_quad(a, t, as_const(a.ray) + (size_t)f * a.ray_stride, tap, gx, px, smp);
    if (WANT_RAY) {
      // a tile without a sampled pixel (every tile inside the object): its partials are the empty sums, +0, what the tree below gives
      // too, without the shuffles; it adds nothing to the cube
      if (!__syncthreads_or(smp != 0u)) {
        if (tid < 9u) a.work[((size_t)f * tpf + ti) * 9u + tid] = 0.0f;
        return;
      }
    }
    const SRZ_CAS float *tex = as_const(a.tex) + (size_t)f * a.tex_frame_stride;
    float *gtex = a.gtex + (size_t)f * a.tex_frame_stride;
    // ---- 2. the slots of the sampled pixels' corners (two corners on one texel: one slot, both add)
    uint32_t slot[4][4] = {};
    if (want_tex) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (smp & (1u << k))
          slot[k][0] = tb.slot(tap[k].i00), slot[k][1] = tb.slot(tap[k].i01), slot[k][2] = tb.slot(tap[k].i10), slot[k][3] = tb.slot(tap[k].i11);
    }
    const auto at = [=](uint32_t idx) { return gtex + (size_t)idx * C; };
    float au[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t n_used = 0u;
    // ---- 3. the channels, ATTR_CHUNK at a time (k_cube_grad's loop)
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 g[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (smp != 0u) {
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
          if (i >= nc) break;
          gout_quad(gg + (size_t)(c0 + i) * rc.plane, t.whole, smp, g[i]);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(smp & (1u << k))) continue;
        if (WANT_RAY) {
          const SRZ_CAS float *p00 = tex + (size_t)tap[k].i00 * C + c0, *p01 = tex + (size_t)tap[k].i01 * C + c0;
          const SRZ_CAS float *p10 = tex + (size_t)tap[k].i10 * C + c0, *p11 = tex + (size_t)tap[k].i11 * C + c0;
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) bilerp_chain(p00 + i, p01 + i, p10 + i, p11 + i, tap[k].tx, tap[k].ty, quad_at(g[i], k), au[k], av[k]);
        }
        if (want_tex) {
          const CornerW w = corner_weights(tap[k].tx, tap[k].ty);
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) corner_adds(tb, slot[k], tap[k], w, quad_at(g[i], k), i, gtex, C, c0 + i);
        }
      }
      if (want_tex) n_used = tb.flush(tid, c0, nc, at); // ---- 4. the table's values of this chunk into memory
    }
    if (want_tex) tb.release(tid, n_used);
    // ---- 5. the ray block's nine partial sums of the tile
    if (WANT_RAY) {
      float tr[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; // this lane's sums of r0[3], rx[3], ry[3]
      const float half_n = 0.5f * (float)a.n, fy = (float)t.y;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (smp & (1u << k)) {
          float gd[3]; // (k_cube_grad's gdir)
          cube_gdir(tap[k].f, au[k], av[k], half_n, gd);
#pragma unroll
          for (int c = 0; c < 3; ++c)
            tr[c] = tr[c] + gd[c], tr[3 + c] = tr[3 + c] + gx[k] * gd[c], tr[6 + c] = tr[6 + c] + fy * gd[c];
        }
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const float v = light_wave_sum(tr[j]);
        if (lane == 0u) s_part[wave][j] = v;
      }
      __syncthreads();
      if (tid < 9u) a.work[((size_t)f * tpf + ti) * 9u + tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
      __syncthreads(); // s_part is the next tile's too
    }
  });
}

// ================================================================================================================
// k_microfacet — COOK-TORRANCE UNDER POINT LIGHTS OVER A VISIBILITY BUFFER, FOR CALLER DATA (srz_frameset_microfacet, include/srz.h
// states the rule): the normal, position and base colour planes, a two-plane material (roughness, metallic) and a parameter frame
// (eye, amb, then the lights) -> three colour planes.  GGX distribution, separable Schlick-Smith visibility, Schlick Fresnel; no
// transcendental function: /, sqrtf, fmaf and a fifth power by multiplication.  k_light's shape on the passes' helpers: pass_walk,
// quad_ids, quad_load, quad_store_owned; no LDS, no barrier.  The parameter frame is wave-uniform: scalar loads.
// mf_px (what a lit pixel keeps across the lights: light_px's part, then the material) and mf_term (one light at one pixel) are the
// rule's text; k_microfacet and k_microfacet_grad both go through them.
// ================================================================================================================
#define MF_INV_PI 0x1.45f306p-2f
#define MF_RMIN 0.0625f
struct MfPx {
  LightPx g; // N, P, Vd, inl, iv, view: light_px's, exactly
  float base[3], F0[3], cdif[3];
  float rc, mc, al, a2, k, omk, om, nv;
  bool r_in, m_in;
};
struct MfTerm {
  float Lv[3], Ld[3], H[3], E[3], F[3], f[3];
  float ir, att, ih, nl, nhr, nh, vhr, vh, t, tt, D, gl, gv, Vs, DV, x4, x5;
  bool spec;
};
// false: not lit
__device__ __forceinline__ bool mf_px(const float (&n)[3], const float (&P)[3], const float (&base)[3], float r, float m,
                                      const SRZ_CAS float *par, MfPx &px) {
  if (!light_px(n, P, par, px.g)) return false;
  px.rc = r > MF_RMIN ? (r < 1.0f ? r : 1.0f) : MF_RMIN, px.r_in = r > MF_RMIN && r < 1.0f;
  px.mc = m > 0.0f ? (m < 1.0f ? m : 1.0f) : 0.0f, px.m_in = m > 0.0f && m < 1.0f;
  px.al = px.rc * px.rc, px.a2 = px.al * px.al, px.k = 0.5f * px.al, px.omk = 1.0f - px.k, px.om = 1.0f - px.mc;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    px.base[c] = base[c];
    px.F0[c] = fmaf_(px.mc, base[c] - 0.04f, 0.04f);
    px.cdif[c] = base[c] * px.om;
  }
  px.nv = px.g.view ? l_dot(px.g.N, px.g.Vd) : 0.0f;
  return true;
}
// lp: the light's {pos[3], intensity[3]}.  false: the light adds nothing at this pixel (skipped, or nl not above 0)
__device__ __forceinline__ bool mf_term(const MfPx &px, const SRZ_CAS float *lp, MfTerm &t) {
#pragma unroll
  for (int i = 0; i < 3; ++i) t.Lv[i] = lp[i] - px.g.P[i];
  const float r2 = l_dot(t.Lv, t.Lv);
  if (!l_pos(r2)) return false;
  t.ir = l_rsqrt(r2), t.att = 1.0f / r2;
  float Hs[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) t.Ld[i] = t.Lv[i] * t.ir, Hs[i] = t.Ld[i] + px.g.Vd[i], t.E[i] = lp[3 + i] * t.att;
  t.nl = l_dot(px.g.N, t.Ld);
  if (!(t.nl > 0.0f)) return false;
  const float h2 = l_dot(Hs, Hs);
  t.spec = px.g.view && h2 > 0.0f && px.nv > 0.0f;
  if (t.spec) {
    t.ih = l_rsqrt(h2);
#pragma unroll
    for (int i = 0; i < 3; ++i) t.H[i] = Hs[i] * t.ih;
    t.nhr = l_dot(px.g.N, t.H), t.nh = t.nhr > 0.0f ? (t.nhr < 1.0f ? t.nhr : 1.0f) : 0.0f;
    t.vhr = l_dot(px.g.Vd, t.H), t.vh = t.vhr > 0.0f ? (t.vhr < 1.0f ? t.vhr : 1.0f) : 0.0f;
    t.t = fmaf_(t.nh * t.nh, px.a2 - 1.0f, 1.0f), t.tt = t.t * t.t, t.D = (px.a2 * MF_INV_PI) / t.tt;
    t.gl = fmaf_(t.nl, px.omk, px.k), t.gv = fmaf_(px.nv, px.omk, px.k), t.Vs = 0.25f / (t.gl * t.gv);
    t.DV = t.D * t.Vs;
    const float x = 1.0f - t.vh, x2 = x * x;
    t.x4 = x2 * x2, t.x5 = t.x4 * x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      t.F[c] = fmaf_(1.0f - px.F0[c], t.x5, px.F0[c]);
      t.f[c] = fmaf_(px.cdif[c] * MF_INV_PI, 1.0f - t.F[c], t.F[c] * t.DV);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) t.f[c] = px.cdif[c] * MF_INV_PI;
  }
  return true;
}
// what k_microfacet and k_microfacet_grad do alike in front of the lights: the owners (`own`, one bit per pixel) and the planes of a quad
// with an owner (base: ones without a base colour buffer) — mf_quad_load —, then pixel k's MfPx — mf_quad_px; false: not owned or not lit
struct MfQuad {
  float4 n[3], P[3], b[3], m[2];
  uint32_t own;
};
__device__ __forceinline__ void mf_quad_load(const MicrofacetArgs &a, const PassTile &t, MfQuad &q) {
  uint32_t id[4];
  q.own = quad_ids(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f), one4 = make_float4(1.f, 1.f, 1.f, 1.f);
  q.n[0] = q.n[1] = q.n[2] = q.P[0] = q.P[1] = q.P[2] = q.m[0] = q.m[1] = zero4, q.b[0] = q.b[1] = q.b[2] = one4;
  if (q.own == 0u) return;
  const size_t off = (size_t)t.f * a.frame_stride + t.poff;
  quad_load(a.nrm + off, t.rc.plane, q.n, t.whole, t.x4, t.rc.tx1);
  quad_load(a.pos + off, t.rc.plane, q.P, t.whole, t.x4, t.rc.tx1);
  if (a.base) quad_load(a.base + off, t.rc.plane, q.b, t.whole, t.x4, t.rc.tx1);
  quad_load(a.mat + (size_t)t.f * a.mat_stride + t.poff, t.rc.plane, q.m, t.whole, t.x4, t.rc.tx1);
}
__device__ __forceinline__ bool mf_quad_px(const MfQuad &q, int k, const SRZ_CAS float *par, MfPx &px) { // (k: a constant)
  if (!(q.own & (1u << k))) return false;
  const float nk[3] = {quad_at(q.n[0], k), quad_at(q.n[1], k), quad_at(q.n[2], k)}, Pk[3] = {quad_at(q.P[0], k), quad_at(q.P[1], k), quad_at(q.P[2], k)};
  const float bk[3] = {quad_at(q.b[0], k), quad_at(q.b[1], k), quad_at(q.b[2], k)};
  return mf_px(nk, Pk, bk, quad_at(q.m[0], k), quad_at(q.m[1], k), par, px);
}
__global__ __launch_bounds__(256) void k_microfacet(MicrofacetArgs a) {
  const uint32_t L = a.n_lights;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool fused = t.fused(a.flags_or);
    const SRZ_CAS float *par = as_const(a.par) + (size_t)t.f * a.par_stride;
    MfQuad q;
    mf_quad_load(a, t, q);
    const uint32_t own = q.own;
    if (own == 0u && !fused) return;
    MfPx px[4];
    uint32_t lit = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (mf_quad_px(q, k, par, px[k])) lit |= 1u << k;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 o[3] = {zero4, zero4, zero4}; // nobody, and an owner that is not lit: zeros
    if (lit != 0u) {
      for (uint32_t l = 0; l < L; ++l) {
        const SRZ_CAS float *lp = par + 6u + 6u * l;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!(lit & (1u << k))) continue;
          MfTerm lt;
          if (!mf_term(px[k], lp, lt)) continue;
#pragma unroll
          for (int c = 0; c < 3; ++c) quad_at(o[c], k) = quad_at(o[c], k) + (lt.f[c] * lt.E[c]) * lt.nl;
        }
      }
      const float amb[3] = {par[3], par[4], par[5]};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(lit & (1u << k))) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) quad_at(o[c], k) = fmaf_(amb[c], px[k].base[c], quad_at(o[c], k));
      }
    }
    quad_store_owned(t.out, t, o, fused, own);
  });
}

// ================================================================================================================
// k_microfacet_grad — THE BACKWARD OF k_microfacet (srz_frameset_microfacet_grad; include/srz.h fixes the order of operations): gout ->
// the gradient planes of the normal, the position, the base colour and the material (per pixel, from registers, deterministic), and,
// WANT_PAR, the gradient of the parameter frame in k_light_grad's fixed tree, word for word: a thread's four pixels left to right, the
// xor butterfly, the four waves through LDS, a row of work per tile; k_light_fold sums the tiles.  The lights are the OUTER loop: a
// light's six lane sums are reduced and put into LDS as its iteration ends; eye and amb follow after the loop.  pass_tiles / pass_tile:
// every thread of the workgroup reaches every shuffle and barrier, one outside the frame owns nothing.  A tile without a lit pixel
// (one barrier tells) writes +0 partials and skips the lights.  The planes-only build has no LDS, no shuffle and no barrier, and walks
// the quad TWO PIXELS AT A TIME (the lights' loop twice): a pixel's arithmetic is the same words either way, and half the live state
// fits two waves per SIMD where four pixels at once overflow the 256 VGPRs into the accumulator file at one wave.
// ================================================================================================================
template <bool WANT_PAR> __global__ __launch_bounds__(256) void k_microfacet_grad(MicrofacetArgs a) {
  __shared__ float s_part[WANT_PAR ? 4 : 1][WANT_PAR ? SRZ_MICROFACET_PAR(SRZ_LIGHT_MAX) : 1];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t L = a.n_lights, K = SRZ_MICROFACET_PAR(L), tpf = a.n_local_bands * a.tiles_x;
  pass_tiles(a, [&](uint32_t f, uint32_t ti) {
    const PassTile t = pass_tile(a, f, ti);
    const bool fused = t.fused(a.flags_or);
    const SRZ_CAS float *par = as_const(a.par) + (size_t)f * a.par_stride;
    const size_t off = (size_t)f * a.frame_stride + t.poff, moff = (size_t)f * a.mat_stride + t.poff;
    // ---- 1. owners and planes; then, PIX pixels of the quad at a time (planes only: two — half the registers, two waves per SIMD —;
    //         with the parameter sums: all four, a lane's sums of a light being over its four pixels): the lit pixels, gout
    MfQuad quad;
    mf_quad_load(a, t, quad);
    const uint32_t own = quad.own;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 g[3] = {zero4, zero4, zero4};
    float4 gN[3] = {zero4, zero4, zero4}, gVd[3] = {zero4, zero4, zero4}, gP[3] = {zero4, zero4, zero4}, gb[3] = {zero4, zero4, zero4};
    float4 g_a2 = zero4, g_k = zero4, g_nv = zero4, g_om = zero4, g_mc = zero4;
    float4 gn[3] = {zero4, zero4, zero4}, gm[2] = {zero4, zero4};
    const float amb[3] = {par[3], par[4], par[5]};
    float te[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; // this lane's sums of eye[3], amb[3]
    constexpr int PIX = WANT_PAR ? 4 : 2;
    if (!WANT_PAR && own != 0u) quad_load(a.gout + off, t.rc.plane, g, t.whole, t.x4, t.rc.tx1);
#pragma unroll
    for (int h0 = 0; h0 < 4; h0 += PIX) {
      MfPx px[4];
      uint32_t lit = 0u;
#pragma unroll
      for (int k = h0; k < h0 + PIX; ++k)
        if (mf_quad_px(quad, k, par, px[k])) lit |= 1u << k;
      if (WANT_PAR) {
        // a tile without a lit pixel: its partials are the empty sums, +0; its planes are zeros where they are written at all
        if (!__syncthreads_or(lit != 0u)) {
          if (t.inside && (own != 0u || fused)) {
            const float4 z[3] = {zero4, zero4, zero4}, z2[2] = {zero4, zero4};
            if (a.gnrm) quad_store_owned(a.gnrm + off, t, z, fused, own);
            if (a.gpos) quad_store_owned(a.gpos + off, t, z, fused, own);
            if (a.gbase) quad_store_owned(a.gbase + off, t, z, fused, own);
            if (a.gmat) quad_store_owned(a.gmat + moff, t, z2, fused, own);
          }
          if (tid < K) a.work[((size_t)f * tpf + ti) * K + tid] = 0.0f;
          return;
        }
        if (lit != 0u) quad_load(a.gout + off, t.rc.plane, g, t.whole, t.x4, t.rc.tx1);
      }
#pragma unroll
      for (int k = h0; k < h0 + PIX; ++k) {
        if (!(lit & (1u << k))) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          quad_at(gb[c], k) = quad_at(g[c], k) * amb[c];
          te[3 + c] = te[3 + c] + quad_at(g[c], k) * px[k].base[c];
        }
      }
      // ---- 2. the lights
      for (uint32_t l = 0; l < L; ++l) {
        const SRZ_CAS float *lp = par + 6u + 6u * l;
        const float I[3] = {lp[3], lp[4], lp[5]};
        float tl[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; // this lane's sums of the light's terms: pos[3], intensity[3]
#pragma unroll
        for (int k = h0; k < h0 + PIX; ++k) {
          if (!(lit & (1u << k))) continue;
          const MfPx &p = px[k];
          MfTerm lt;
          if (!mf_term(p, lp, lt)) continue;
          const float gk[3] = {quad_at(g[0], k), quad_at(g[1], k), quad_at(g[2], k)};
          float gf[3], ge[3], q[3], gcd[3], gLd[3] = {0.f, 0.f, 0.f};
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float gq = gk[c] * lt.nl;
            gf[c] = gq * lt.E[c], ge[c] = gq * lt.f[c], q[c] = lt.f[c] * lt.E[c];
            if (WANT_PAR) tl[3 + c] = tl[3 + c] + ge[c] * lt.att;
          }
          float g_nl = l_dot(gk, q);
          const float g_att = l_dot(ge, I);
          if (lt.spec) {
            float gF[3], gF0[3], omF0[3], bm[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              gcd[c] = (gf[c] * (1.0f - lt.F[c])) * MF_INV_PI;
              gF[c] = gf[c] * (lt.DV - p.cdif[c] * MF_INV_PI);
              gF0[c] = gF[c] * (1.0f - lt.x5);
              omF0[c] = 1.0f - p.F0[c], bm[c] = p.base[c] - 0.04f;
              quad_at(gb[c], k) = quad_at(gb[c], k) + gF0[c] * p.mc;
            }
            quad_at(g_mc, k) = quad_at(g_mc, k) + l_dot(gF0, bm);
            const float gDV = l_dot(gf, lt.F), gD = gDV * lt.Vs, gVs = gDV * lt.D;
            const float gx = l_dot(gF, omF0) * (5.0f * lt.x4);
            const float g_vhr = lt.vhr > 0.0f && lt.vhr < 1.0f ? -gx : 0.0f;
            const float gw = -(gVs * lt.Vs), ggl = gw / lt.gl, ggv = gw / lt.gv;
            g_nl = fmaf_(ggl, p.omk, g_nl);
            quad_at(g_nv, k) = fmaf_(ggv, p.omk, quad_at(g_nv, k));
            quad_at(g_k, k) = quad_at(g_k, k) + fmaf_(ggl, 1.0f - lt.nl, ggv * (1.0f - p.nv));
            const float g_t = -((2.0f * (gD * lt.D)) / lt.t);
            quad_at(g_a2, k) = quad_at(g_a2, k) + fmaf_(g_t, lt.nh * lt.nh, gD * (MF_INV_PI / lt.tt));
            const float g_nhr = lt.nhr > 0.0f && lt.nhr < 1.0f ? g_t * ((2.0f * lt.nh) * (p.a2 - 1.0f)) : 0.0f;
            float gH[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              gH[c] = fmaf_(g_nhr, p.g.N[c], g_vhr * p.g.Vd[c]);
              quad_at(gN[c], k) = quad_at(gN[c], k) + g_nhr * lt.H[c];
              quad_at(gVd[c], k) = quad_at(gVd[c], k) + g_vhr * lt.H[c];
            }
            const float d = l_dot(gH, lt.H);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const float gHs = (gH[c] - lt.H[c] * d) * lt.ih;
              gLd[c] = gHs, quad_at(gVd[c], k) = quad_at(gVd[c], k) + gHs;
            }
          } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) gcd[c] = gf[c] * MF_INV_PI;
          }
          quad_at(g_om, k) = quad_at(g_om, k) + l_dot(gcd, p.base);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            quad_at(gb[c], k) = quad_at(gb[c], k) + gcd[c] * p.om;
            gLd[c] = fmaf_(g_nl, p.g.N[c], gLd[c]);
            quad_at(gN[c], k) = quad_at(gN[c], k) + g_nl * lt.Ld[c];
          }
          const float d = l_dot(gLd, lt.Ld), two_g_r2 = 2.0f * (-((g_att * lt.att) * lt.att));
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float gLv = fmaf_(lt.Lv[c], two_g_r2, (gLd[c] - lt.Ld[c] * d) * lt.ir);
            tl[c] = tl[c] + gLv, quad_at(gP[c], k) = quad_at(gP[c], k) - gLv;
          }
        }
        if (WANT_PAR) { // (every lane of the workgroup is here: the walk and the light count are uniform)
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            const float v = light_wave_sum(tl[j]);
            if (lane == 0u) s_part[wave][6u + 6u * l + (uint32_t)j] = v;
          }
        }
      }
      // ---- 3. behind the lights: nv's share, the view direction's and the normal's normalisations, the eye's terms, the material
#pragma unroll
      for (int k = h0; k < h0 + PIX; ++k) {
        if (!(lit & (1u << k))) continue;
        const MfPx &p = px[k];
        float vN[3] = {quad_at(gN[0], k), quad_at(gN[1], k), quad_at(gN[2], k)};
        if (p.g.view) {
          float v[3] = {quad_at(gVd[0], k), quad_at(gVd[1], k), quad_at(gVd[2], k)};
#pragma unroll
          for (int c = 0; c < 3; ++c) vN[c] = fmaf_(quad_at(g_nv, k), p.g.Vd[c], vN[c]), v[c] = fmaf_(quad_at(g_nv, k), p.g.N[c], v[c]);
          const float d = l_dot(v, p.g.Vd);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float gV = (v[c] - p.g.Vd[c] * d) * p.g.iv;
            te[c] = te[c] + gV, quad_at(gP[c], k) = quad_at(gP[c], k) - gV;
          }
        }
        const float d = l_dot(vN, p.g.N);
#pragma unroll
        for (int c = 0; c < 3; ++c) quad_at(gn[c], k) = (vN[c] - p.g.N[c] * d) * p.g.inl;
        const float g_al = fmaf_(quad_at(g_a2, k), 2.0f * p.al, 0.5f * quad_at(g_k, k));
        quad_at(gm[0], k) = p.r_in ? g_al * (2.0f * p.rc) : 0.0f;
        quad_at(gm[1], k) = p.m_in ? quad_at(g_mc, k) - quad_at(g_om, k) : 0.0f;
      }
    } // (the next PIX pixels)
    // ---- 4. the planes: whole quads (fused clear, or four owners), else the owned pixels only; an owner that is not lit: zeros
    if (t.inside && (own != 0u || fused)) {
      if (a.gnrm) quad_store_owned(a.gnrm + off, t, gn, fused, own);
      if (a.gpos) quad_store_owned(a.gpos + off, t, gP, fused, own);
      if (a.gbase) quad_store_owned(a.gbase + off, t, gb, fused, own);
      if (a.gmat) quad_store_owned(a.gmat + moff, t, gm, fused, own);
    }
    // ---- 5. the tile's K partial sums
    if (WANT_PAR) {
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const float v = light_wave_sum(te[j]);
        if (lane == 0u) s_part[wave][j] = v;
      }
      __syncthreads();
      if (tid < K) a.work[((size_t)f * tpf + ti) * K + tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
      __syncthreads(); // s_part is the next tile's too
    }
  });
}

// ================================================================================================================
// k_reflect / k_reflect_grad — THE REFLECTION VECTOR AND n.v OVER A VISIBILITY BUFFER, FOR CALLER DATA (srz_frameset_reflect and its
// backward, include/srz.h states the rule and the backward's order of operations): the normal and position planes and the eye ->
// R = 2 (N.Vd) N - Vd in three planes and the raw N.Vd in a fourth.  light_px is the rule's front part, word for word (the eye is
// where k_light's parameter frame has it: wave-uniform, scalar loads).  k_microfacet's shape on the passes' helpers: pass_walk,
// quad_ids, quad_load, quad_store_owned; no LDS, no barrier, no atomics; every output is per pixel, from registers.
// ================================================================================================================
struct RfQuad {
  float4 n[3], P[3];
  uint32_t own;
};
__device__ __forceinline__ void rf_quad_load(const ReflectArgs &a, const PassTile &t, RfQuad &q) {
  uint32_t id[4];
  q.own = quad_ids(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id);
  q.n[0] = q.n[1] = q.n[2] = q.P[0] = q.P[1] = q.P[2] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q.own == 0u) return;
  const size_t off = (size_t)t.f * a.nrm_stride + t.poff;
  quad_load(a.nrm + off, t.rc.plane, q.n, t.whole, t.x4, t.rc.tx1);
  quad_load(a.pos + off, t.rc.plane, q.P, t.whole, t.x4, t.rc.tx1);
}
// false: not owned, not lit or no view — four zeros, no gradient; nv: the raw cosine
__device__ __forceinline__ bool rf_quad_px(const RfQuad &q, int k, const SRZ_CAS float *eye, LightPx &px, float &nv) { // (k: a constant)
  if (!(q.own & (1u << k))) return false;
  const float nk[3] = {quad_at(q.n[0], k), quad_at(q.n[1], k), quad_at(q.n[2], k)}, Pk[3] = {quad_at(q.P[0], k), quad_at(q.P[1], k), quad_at(q.P[2], k)};
  if (!light_px(nk, Pk, eye, px) || !px.view) return false;
  nv = l_dot(px.N, px.Vd);
  return true;
}
__global__ __launch_bounds__(256) void k_reflect(ReflectArgs a) {
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool fused = t.fused(a.flags_or);
    const SRZ_CAS float *eye = as_const(a.eye) + (size_t)t.f * a.eye_stride;
    RfQuad q;
    rf_quad_load(a, t, q);
    if (q.own == 0u && !fused) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 o[4] = {zero4, zero4, zero4, zero4}; // nobody, an owner that is not lit, one without a view: zeros
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      LightPx px;
      float nv;
      if (!rf_quad_px(q, k, eye, px, nv)) continue;
      const float t2 = 2.0f * nv;
#pragma unroll
      for (int c = 0; c < 3; ++c) quad_at(o[c], k) = fmaf_(t2, px.N[c], -px.Vd[c]);
      quad_at(o[3], k) = nv;
    }
    quad_store_owned(t.out, t, o, fused, q.own);
  });
}
__global__ __launch_bounds__(256) void k_reflect_grad(ReflectArgs a) {
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool fused = t.fused(a.flags_or);
    const SRZ_CAS float *eye = as_const(a.eye) + (size_t)t.f * a.eye_stride;
    RfQuad q;
    rf_quad_load(a, t, q);
    if (q.own == 0u && !fused) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 g[4] = {zero4, zero4, zero4, zero4}, gn[3] = {zero4, zero4, zero4}, gP[3] = {zero4, zero4, zero4};
    if (q.own != 0u) quad_load(a.gout + (size_t)t.f * a.frame_stride + t.poff, t.rc.plane, g, t.whole, t.x4, t.rc.tx1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      LightPx px;
      float nv;
      if (!rf_quad_px(q, k, eye, px, nv)) continue;
      const float gR[3] = {quad_at(g[0], k), quad_at(g[1], k), quad_at(g[2], k)}, t2 = 2.0f * nv;
      const float g_nv = fmaf_(2.0f, l_dot(gR, px.N), quad_at(g[3], k));
      float gN[3], gVd[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) gN[c] = fmaf_(g_nv, px.Vd[c], gR[c] * t2), gVd[c] = fmaf_(g_nv, px.N[c], -gR[c]);
      const float dv = l_dot(gVd, px.Vd), dn = l_dot(gN, px.N);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        quad_at(gP[c], k) = -((gVd[c] - px.Vd[c] * dv) * px.iv);
        quad_at(gn[c], k) = (gN[c] - px.N[c] * dn) * px.inl;
      }
    }
    const size_t off = (size_t)t.f * a.nrm_stride + t.poff;
    if (a.gnrm) quad_store_owned(a.gnrm + off, t, gn, fused, q.own);
    if (a.gpos) quad_store_owned(a.gpos + off, t, gP, fused, q.own);
  });
}

// ================================================================================================================
// k_brdf_table — THE SPLIT-SUM ENVIRONMENT BRDF OF k_microfacet's OWN SPECULAR LOBE (srz_brdf_table, include/srz.h states the
// quadrature and the order of its sums): entry (i, j) of [n][n][2] is (A, B) at nv = i / (n - 1), roughness RMIN + 0.9375 j / (n - 1),
// so that F0 A + B is the directional albedo of the lobe mf_term shades with.  m rings of 2 m samples over the projected half vector,
// rational throughout: /, sqrtf, fmaf.  One wave per entry, the lanes over the rings (ring a on lane a mod 64): a lane sums its ring's
// 2 m samples in sequence from +0, the ring sums meet in LDS, and lane 0 folds them in ring order with the ring weights — the order
// is the rule's, whatever the launch shape, so the words are the CPU reference's.
// ================================================================================================================
constexpr uint32_t BRDF_M_MAX = 256u;
__global__ __launch_bounds__(64) void k_brdf_table(float *tab, uint32_t n, uint32_t m) {
  __shared__ float s_ring[3][BRDF_M_MAX]; // the ring's A sum, its B sum, its weight
  const uint32_t i = blockIdx.x / n, j = blockIdx.x % n, lane = threadIdx.x;
  const float nv = (float)i / (float)(n - 1u), rc = fmaf_(0.9375f, (float)j / (float)(n - 1u), MF_RMIN);
  const float al = rc * rc, a2 = al * al, k = 0.5f * al, omk = 1.0f - k;
  const float vx = __builtin_sqrtf(fmaf_(-nv, nv, 1.0f)), gv = fmaf_(nv, omk, k), fm = (float)m;
  for (uint32_t ra = lane; ra < m; ra += 64u) {
    const float u = ((float)ra + 0.5f) / fm, q = 1.0f - u, xi = fmaf_(-q, q, 1.0f);
    const float s = (a2 * xi) / fmaf_(-xi, 1.0f - a2, 1.0f), r = __builtin_sqrtf(s), hz = __builtin_sqrtf(1.0f - s);
    float sa = 0.0f, sb = 0.0f;
    for (uint32_t b = 0; b < m; ++b) {
      const float t = ((float)b + 0.5f) / fm, tt = t * t, den = 1.0f + tt, c = (1.0f - tt) / den, wa = (2.0f / den) / fm;
#pragma unroll
      for (int sgn = 0; sgn < 2; ++sgn) {
        const float hx = sgn ? -(r * c) : r * c;
        const float vh = fmaf_(vx, hx, nv * hz), nl = fmaf_(2.0f * vh, hz, -nv);
        const bool take = vh > 0.0f && nl > 0.0f;
        const float gl = fmaf_(nl, omk, k), f = (nl * vh) / (hz * (gl * gv));
        const float x = 1.0f - (vh < 1.0f ? vh : 1.0f), x2 = x * x, x4 = x2 * x2, x5 = x4 * x;
        sa = sa + (take ? (f * (1.0f - x5)) * wa : 0.0f), sb = sb + (take ? (f * x5) * wa : 0.0f);
      }
    }
    s_ring[0][ra] = sa, s_ring[1][ra] = sb, s_ring[2][ra] = (2.0f * q) / fm;
  }
  __syncthreads();
  if (lane == 0u) {
    float A = 0.0f, B = 0.0f;
    for (uint32_t ra = 0; ra < m; ++ra) A = fmaf_(s_ring[0][ra], s_ring[2][ra], A), B = fmaf_(s_ring[1][ra], s_ring[2][ra], B);
    tab[2u * blockIdx.x] = A * MF_INV_PI, tab[2u * blockIdx.x + 1u] = B * MF_INV_PI;
  }
}

// ================================================================================================================
// k_ibl / k_ibl_grad — THE SPLIT-SUM COMBINE OVER A VISIBILITY BUFFER, FOR CALLER DATA (srz_frameset_ibl and its backward,
// include/srz.h states the rule and the backward's order of operations): base colour, material (roughness, metallic: mf_px's clamps,
// word for word), nv, the irradiance and the prefiltered specular planes and the table [n][n][2] ->
// out = cdif irr + spec (F0 A + B), (A, B) bilinear at (nv, roughness) in tex_bilinear's three-fmaf form.  The clamps hold the cell
// inside the table whatever the planes hold.  k_microfacet's shape on the passes' helpers.  ibl_px is the rule's text; both kernels go
// through it.  The backward's planes are per pixel, from registers; WANT_TAB, the table's gradient is summed per WORKGROUP in LDS
// (the whole table fits: 32 KiB at n = 64; ds float adds) over every tile the workgroup walks, then one global float add per word
// the workgroup touched: not bit-reproducible, within texture_grad's bound.  That build's grid is capped lower, so that a workgroup
// walks several tiles per clear and flush of its table.
// ================================================================================================================
struct IblPx {
  float base[3], F0[3], cdif[3], irr[3], spec[3], sc[3];
  float mc, om, tx, ty, A, B, dAx, dBx, dAy, dBy;
  bool r_in, m_in, nv_in;
  uint32_t at; // the cell's first word pair: x0 * n + y0
};
__device__ __forceinline__ void ibl_px(const float (&base)[3], float r, float m, float nv, const float (&irr)[3], const float (&spec)[3],
                                       const float *tab, uint32_t n, float sx, float sy, IblPx &p) {
  const float rc = r > MF_RMIN ? (r < 1.0f ? r : 1.0f) : MF_RMIN;
  p.r_in = r > MF_RMIN && r < 1.0f;
  p.mc = m > 0.0f ? (m < 1.0f ? m : 1.0f) : 0.0f, p.m_in = m > 0.0f && m < 1.0f;
  const float nvc = nv > 0.0f ? (nv < 1.0f ? nv : 1.0f) : 0.0f;
  p.nv_in = nv > 0.0f && nv < 1.0f;
  const float x = nvc * sx, y = (rc - MF_RMIN) * sy; // (both in [0, n - 1 + an ulp]: the clamps leave no NaN)
  const int fx = (int)__builtin_floorf(x), fy = (int)__builtin_floorf(y), last = (int)n - 2;
  const int x0 = fx < last ? fx : last, y0 = fy < last ? fy : last;
  p.tx = x - (float)x0, p.ty = y - (float)y0;
  p.at = (uint32_t)x0 * n + (uint32_t)y0;
  const float *t00 = tab + 2u * p.at, *t10 = t00 + 2u * n;
  float v[2], dx[2], dy[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float d0 = t00[2 + e] - t00[e], d1 = t10[2 + e] - t10[e];
    const float top = fmaf_(p.ty, d0, t00[e]), bot = fmaf_(p.ty, d1, t10[e]);
    dx[e] = bot - top, v[e] = fmaf_(p.tx, dx[e], top), dy[e] = fmaf_(p.tx, d1 - d0, d0);
  }
  p.A = v[0], p.B = v[1], p.dAx = dx[0], p.dBx = dx[1], p.dAy = dy[0], p.dBy = dy[1];
  p.om = 1.0f - p.mc;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    p.base[c] = base[c], p.irr[c] = irr[c], p.spec[c] = spec[c];
    p.F0[c] = fmaf_(p.mc, base[c] - 0.04f, 0.04f);
    p.cdif[c] = base[c] * p.om;
    p.sc[c] = fmaf_(p.F0[c], p.A, p.B);
  }
}
struct IblQuad {
  float4 b[3], m[2], nv[1], irr[3], spec[3];
  uint32_t own;
};
__device__ __forceinline__ void ibl_quad_load(const IblArgs &a, const PassTile &t, IblQuad &q) {
  uint32_t id[4];
  q.own = quad_ids(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f), one4 = make_float4(1.f, 1.f, 1.f, 1.f);
  q.m[0] = q.m[1] = q.nv[0] = q.irr[0] = q.irr[1] = q.irr[2] = q.spec[0] = q.spec[1] = q.spec[2] = zero4, q.b[0] = q.b[1] = q.b[2] = one4;
  if (q.own == 0u) return;
  const size_t off = (size_t)t.f * a.frame_stride + t.poff;
  if (a.base) quad_load(a.base + off, t.rc.plane, q.b, t.whole, t.x4, t.rc.tx1);
  quad_load(a.mat + (size_t)t.f * a.mat_stride + t.poff, t.rc.plane, q.m, t.whole, t.x4, t.rc.tx1);
  quad_load(a.nv + (size_t)t.f * a.nv_stride + t.poff, t.rc.plane, q.nv, t.whole, t.x4, t.rc.tx1);
  quad_load(a.irr + off, t.rc.plane, q.irr, t.whole, t.x4, t.rc.tx1);
  quad_load(a.spec + off, t.rc.plane, q.spec, t.whole, t.x4, t.rc.tx1);
}
__device__ __forceinline__ void ibl_quad_px(const IblArgs &a, const IblQuad &q, int k, float sx, float sy, IblPx &p) { // (k: a constant)
  const float bk[3] = {quad_at(q.b[0], k), quad_at(q.b[1], k), quad_at(q.b[2], k)};
  const float ik[3] = {quad_at(q.irr[0], k), quad_at(q.irr[1], k), quad_at(q.irr[2], k)};
  const float sk[3] = {quad_at(q.spec[0], k), quad_at(q.spec[1], k), quad_at(q.spec[2], k)};
  ibl_px(bk, quad_at(q.m[0], k), quad_at(q.m[1], k), quad_at(q.nv[0], k), ik, sk, a.tab, a.n, sx, sy, p);
}
__global__ __launch_bounds__(256) void k_ibl(IblArgs a) {
  const float sx = (float)(a.n - 1u), sy = (float)(a.n - 1u) / 0.9375f;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool fused = t.fused(a.flags_or);
    IblQuad q;
    ibl_quad_load(a, t, q);
    if (q.own == 0u && !fused) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 o[3] = {zero4, zero4, zero4}; // nobody: zeros
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(q.own & (1u << k))) continue;
      IblPx p;
      ibl_quad_px(a, q, k, sx, sy, p);
#pragma unroll
      for (int c = 0; c < 3; ++c) quad_at(o[c], k) = fmaf_(p.cdif[c], p.irr[c], p.spec[c] * p.sc[c]);
    }
    quad_store_owned(t.out, t, o, fused, q.own);
  });
}
constexpr uint32_t IBL_TAB_MAX = 64u; // SRZ_BRDF_TABLE_MAX: the table's words fit LDS
template <bool WANT_TAB> __global__ __launch_bounds__(256) void k_ibl_grad(IblArgs a) {
  __shared__ float s_tab[WANT_TAB ? 2u * IBL_TAB_MAX * IBL_TAB_MAX : 1u];
  const uint32_t tid = threadIdx.x, n_words = 2u * a.n * a.n; // (the host has checked n <= 64)
  const float sx = (float)(a.n - 1u), sy = (float)(a.n - 1u) / 0.9375f;
  if (WANT_TAB) {
    for (uint32_t i = tid; i < n_words; i += 256u) s_tab[i] = 0.0f;
    __syncthreads();
  }
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier inside the walk: a thread outside the frame just moves on)
    const bool fused = t.fused(a.flags_or);
    IblQuad q;
    ibl_quad_load(a, t, q);
    if (q.own == 0u && !fused) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 g[3] = {zero4, zero4, zero4}, gb[3] = {zero4, zero4, zero4}, gi[3] = {zero4, zero4, zero4}, gsp[3] = {zero4, zero4, zero4};
    float4 gm[2] = {zero4, zero4}, gn[1] = {zero4};
    const size_t off = (size_t)t.f * a.frame_stride + t.poff;
    if (q.own != 0u) quad_load(a.gout + off, t.rc.plane, g, t.whole, t.x4, t.rc.tx1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(q.own & (1u << k))) continue;
      IblPx p;
      ibl_quad_px(a, q, k, sx, sy, p);
      const float gk[3] = {quad_at(g[0], k), quad_at(g[1], k), quad_at(g[2], k)};
      float gcd[3], gs[3], gF0[3], bm[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        gcd[c] = gk[c] * p.irr[c], quad_at(gi[c], k) = gk[c] * p.cdif[c];
        gs[c] = gk[c] * p.spec[c], quad_at(gsp[c], k) = gk[c] * p.sc[c];
        gF0[c] = gs[c] * p.A, bm[c] = p.base[c] - 0.04f;
        quad_at(gb[c], k) = fmaf_(gF0[c], p.mc, gcd[c] * p.om);
      }
      const float gA = l_dot(gs, p.F0), gB = l_dot(gk, p.spec);
      const float g_mc = l_dot(gF0, bm), g_om = l_dot(gcd, p.base);
      const float g_x = fmaf_(gA, p.dAx, gB * p.dBx), g_y = fmaf_(gA, p.dAy, gB * p.dBy);
      quad_at(gm[0], k) = p.r_in ? g_y * sy : 0.0f;
      quad_at(gm[1], k) = p.m_in ? g_mc - g_om : 0.0f;
      quad_at(gn[0], k) = p.nv_in ? g_x * sx : 0.0f;
      if (WANT_TAB) {
        const float ux = 1.0f - p.tx, uy = 1.0f - p.ty;
        const float w[4] = {ux * uy, ux * p.ty, p.tx * uy, p.tx * p.ty};
        const uint32_t at[4] = {p.at, p.at + 1u, p.at + a.n, p.at + a.n + 1u}; // (x0, y0 <= n - 2: all four inside the table)
#pragma unroll
        for (int c = 0; c < 4; ++c) atomicAdd(&s_tab[2u * at[c]], w[c] * gA), atomicAdd(&s_tab[2u * at[c] + 1u], w[c] * gB);
      }
    }
    if (a.gbase) quad_store_owned(a.gbase + off, t, gb, fused, q.own);
    if (a.gmat) quad_store_owned(a.gmat + (size_t)t.f * a.mat_stride + t.poff, t, gm, fused, q.own);
    if (a.gnv) quad_store_owned(a.gnv + (size_t)t.f * a.nv_stride + t.poff, t, gn, fused, q.own);
    if (a.girr) quad_store_owned(a.girr + off, t, gi, fused, q.own);
    if (a.gspec) quad_store_owned(a.gspec + off, t, gsp, fused, q.own);
  });
  if (WANT_TAB) { // (the walk's exit is uniform over the workgroup: every thread is here)
    __syncthreads();
    for (uint32_t i = tid; i < n_words; i += 256u) {
      const float v = s_tab[i];
      if (v != 0.0f) global_add(a.gtab + i, v); // (a NaN is not 0: it goes too)
    }
  }
}

// ================================================================================================================
// k_normal_map / k_normal_map_grad — TANGENT-SPACE NORMAL MAPPING OVER A VISIBILITY BUFFER, FOR CALLER DATA (srz_frameset_normal_map
// and its backward, include/srz.h states the rule and the backward's order of operations): the interpolated normal (3 planes), the
// interpolated tangent with its handedness (4 planes) and the tangent-space normal m (3 planes) -> the unit shading normal k_light
// and k_cube take.  k_light's shape on the passes' helpers: pass_walk, quad_ids, the planes of a quad with an owner in 16-byte
// loads, quad_store_owned; no LDS, no barrier, no atomics; every output is per pixel, from registers.  nm_px is the rule's text;
// both kernels go through it, so the backward differentiates the very words the forward computed.
// ================================================================================================================
enum : int { NM_UNLIT = 0, NM_PLAIN = 1, NM_MAPPED = 2 }; // out = 0; out = N (no frame, or R = 0); out = R / |R|
struct NmPx {
  float N[3], T[3], B[3], o[3]; // o: the output
  float inl, d, it, hw, ir;
};
__device__ __forceinline__ void nm_cross(const float (&u)[3], const float (&w)[3], float (&c)[3]) {
  c[0] = u[1] * w[2] - u[2] * w[1], c[1] = u[2] * w[0] - u[0] * w[2], c[2] = u[0] * w[1] - u[1] * w[0];
}
__device__ __forceinline__ int nm_px(const float (&n)[3], const float (&t)[4], const float (&m)[3], NmPx &px) {
  px.o[0] = px.o[1] = px.o[2] = 0.0f;
  const float nn = l_dot(n, n);
  if (!l_pos(nn)) return NM_UNLIT;
  px.inl = l_rsqrt(nn);
#pragma unroll
  for (int i = 0; i < 3; ++i) px.N[i] = n[i] * px.inl, px.o[i] = px.N[i];
  const float t3[3] = {t[0], t[1], t[2]};
  px.d = l_dot(px.N, t3);
  float Tp[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) Tp[i] = t3[i] - px.N[i] * px.d;
  const float tt = l_dot(Tp, Tp);
  if (!l_pos(tt)) return NM_PLAIN;
  px.it = l_rsqrt(tt), px.hw = t[3] < 0.0f ? -1.0f : 1.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) px.T[i] = Tp[i] * px.it;
  float Cr[3], R[3];
  nm_cross(px.N, px.T, Cr);
#pragma unroll
  for (int i = 0; i < 3; ++i) px.B[i] = Cr[i] * px.hw, R[i] = fmaf_(m[0], px.T[i], fmaf_(m[1], px.B[i], m[2] * px.N[i]));
  const float rr = l_dot(R, R);
  if (!l_pos(rr)) return NM_PLAIN;
  px.ir = l_rsqrt(rr);
#pragma unroll
  for (int i = 0; i < 3; ++i) px.o[i] = R[i] * px.ir;
  return NM_MAPPED;
}
// the owners of the thread's quad and, for a quad with one, its ten input planes -> `own`
__device__ __forceinline__ uint32_t normal_map_quad(const NormalMapArgs &a, const PassTile &t, float4 (&n)[3], float4 (&tn)[4], float4 (&m)[3]) {
  uint32_t id[4];
  const uint32_t own = quad_ids(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  n[0] = n[1] = n[2] = m[0] = m[1] = m[2] = tn[0] = tn[1] = tn[2] = tn[3] = zero4;
  if (own == 0u) return own;
  const size_t off = (size_t)t.f * a.frame_stride + t.poff;
  quad_load(a.nrm + off, t.rc.plane, n, t.whole, t.x4, t.rc.tx1);
  quad_load(a.tan + (size_t)t.f * a.tan_stride + t.poff, t.rc.plane, tn, t.whole, t.x4, t.rc.tx1);
  quad_load(a.m + off, t.rc.plane, m, t.whole, t.x4, t.rc.tx1);
  return own;
}
__global__ __launch_bounds__(256) void k_normal_map(NormalMapArgs a) {
  pass_walk<false>(a, [&](const PassTile &t) {
    const bool fused = t.fused(a.flags_or);
    float4 n[3], tn[4], m[3];
    const uint32_t own = normal_map_quad(a, t, n, tn, m);
    if (own == 0u && !fused) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 o[3] = {zero4, zero4, zero4}; // nobody, and an owner without a normal: zeros
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(own & (1u << k))) continue;
      const float nk[3] = {quad_at(n[0], k), quad_at(n[1], k), quad_at(n[2], k)}, mk[3] = {quad_at(m[0], k), quad_at(m[1], k), quad_at(m[2], k)};
      const float tk[4] = {quad_at(tn[0], k), quad_at(tn[1], k), quad_at(tn[2], k), quad_at(tn[3], k)};
      NmPx px;
      nm_px(nk, tk, mk, px);
#pragma unroll
      for (int c = 0; c < 3; ++c) quad_at(o[c], k) = px.o[c];
    }
    quad_store_owned(t.out, t, o, fused, own);
  });
}
__global__ __launch_bounds__(256) void k_normal_map_grad(NormalMapArgs a) {
  pass_walk<false>(a, [&](const PassTile &t) {
    const bool fused = t.fused(a.flags_or);
    float4 n[3], tn[4], m[3];
    const uint32_t own = normal_map_quad(a, t, n, tn, m);
    if (own == 0u && !fused) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const size_t off = (size_t)t.f * a.frame_stride + t.poff, off4 = (size_t)t.f * a.tan_stride + t.poff;
    float4 g[3] = {zero4, zero4, zero4};
    if (own != 0u) quad_load(a.gout + off, t.rc.plane, g, t.whole, t.x4, t.rc.tx1);
    float4 gn[3] = {zero4, zero4, zero4}, gt[4] = {zero4, zero4, zero4, zero4}, gm[3] = {zero4, zero4, zero4};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(own & (1u << k))) continue;
      const float nk[3] = {quad_at(n[0], k), quad_at(n[1], k), quad_at(n[2], k)}, mk[3] = {quad_at(m[0], k), quad_at(m[1], k), quad_at(m[2], k)};
      const float tk[4] = {quad_at(tn[0], k), quad_at(tn[1], k), quad_at(tn[2], k), quad_at(tn[3], k)};
      NmPx px;
      const int mode = nm_px(nk, tk, mk, px);
      if (mode == NM_UNLIT) continue;
      float gN[3] = {quad_at(g[0], k), quad_at(g[1], k), quad_at(g[2], k)};
      if (mode == NM_MAPPED) {
        const float gk[3] = {gN[0], gN[1], gN[2]};
        const float dq = l_dot(gk, px.o);
        float gR[3], gT[3], gC[3], X[3], Y[3], gTp[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) gR[c] = (gk[c] - px.o[c] * dq) * px.ir;
        quad_at(gm[0], k) = l_dot(gR, px.T), quad_at(gm[1], k) = l_dot(gR, px.B), quad_at(gm[2], k) = l_dot(gR, px.N);
#pragma unroll
        for (int c = 0; c < 3; ++c) gT[c] = mk[0] * gR[c], gC[c] = (mk[1] * gR[c]) * px.hw, gN[c] = mk[2] * gR[c];
        nm_cross(px.T, gC, X), nm_cross(gC, px.N, Y);
#pragma unroll
        for (int c = 0; c < 3; ++c) gN[c] = gN[c] + X[c], gT[c] = gT[c] + Y[c];
        const float dT = l_dot(gT, px.T);
#pragma unroll
        for (int c = 0; c < 3; ++c) gTp[c] = (gT[c] - px.T[c] * dT) * px.it;
        const float gd = -l_dot(gTp, px.N);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          gN[c] = (gN[c] - gTp[c] * px.d) + gd * tk[c];
          quad_at(gt[c], k) = gTp[c] + gd * px.N[c];
        }
      }
      const float dn = l_dot(gN, px.N);
#pragma unroll
      for (int c = 0; c < 3; ++c) quad_at(gn[c], k) = (gN[c] - px.N[c] * dn) * px.inl;
    }
    if (a.gnrm) quad_store_owned(a.gnrm + off, t, gn, fused, own);
    if (a.gtan) quad_store_owned(a.gtan + off4, t, gt, fused, own);
    if (a.gm) quad_store_owned(a.gm + off, t, gm, fused, own);
  });
}

// ================================================================================================================
// k_mip_build / k_mip_fold — THE MIP PYRAMID OF A CALLER TEXTURE (srz_texture_mip_build, srz_texture_mip_fold; include/srz.h states
// the geometry and the arithmetic).  The build is one launch per level, each from the level above it: a workgroup walks rows of the
// level it writes, its threads the row's (texel, channel) elements — consecutive lanes, consecutive floats.  The fold is the build's
// transpose as a GATHER: per element of level 0 the chain of its ancestors, coarsest first, one fma per level — no atomics.
// Both are bound by memory: the build reads 4 (2) floats per float it writes, the fold's ancestors come from cache.
// ================================================================================================================
__global__ __launch_bounds__(256) void k_mip_build(const float *src, float *dst, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h,
                                                   uint32_t C, uint32_t n_rows) {
  const bool both = src_w > 1u && src_h > 1u, along_x = src_w > 1u;
  const size_t row = (size_t)src_w * C;
  const uint32_t per_row = dst_w * C; // (<= 8192 * 64)
  for (uint32_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const uint32_t ft = r / dst_h, y = r % dst_h;
    const float *s = src + ((size_t)ft * src_h + (src_h > 1u ? 2u * y : 0u)) * row;
    float *d = dst + (size_t)r * per_row;
    for (uint32_t i = threadIdx.x; i < per_row; i += 256u) {
      const uint32_t x = i / C, ch = i % C;
      const float *p = s + (size_t)(along_x ? 2u * x : 0u) * C + ch;
      d[i] = both ? ((p[0] + p[C]) + (p[row] + p[row + C])) * 0.25f : (p[0] + p[along_x ? (size_t)C : row]) * 0.5f;
    }
  }
}
__global__ __launch_bounds__(256) void k_mip_fold(const float *gmip, float *gtex, uint32_t W, uint32_t H, uint32_t C, uint32_t TF, uint32_t L) {
  const uint32_t n_rows = TF * H, per_row = W * C;
  const size_t total = (size_t)mip_texels_before(W, H, L) * TF * C; // the floats of the levels 1 .. L - 1
  for (uint32_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const uint32_t ft = r / H, y = r % H;
    float *d = gtex + (size_t)r * per_row;
    for (uint32_t i = threadIdx.x; i < per_row; i += 256u) {
      const uint32_t x = i / C, ch = i % C;
      size_t end = total;
      float acc = 0.0f;
      for (uint32_t l = L - 1u; l >= 1u; --l) { // (wave-uniform: the levels' sizes and places are scalars)
        const uint32_t wl = mip_extent(W, l), hl = mip_extent(H, l);
        const size_t off = end - (size_t)wl * hl * TF * C;
        const float g = gmip[off + (((size_t)ft * hl + (y >> l)) * wl + (x >> l)) * C + ch];
        acc = l == L - 1u ? g : fmaf_(mip_factor(W, H, l + 1u), acc, g);
        end = off;
      }
      d[i] = fmaf_(mip_factor(W, H, 1u), acc, d[i]);
    }
  }
}

// ================================================================================================================
// k_prefilter — A CUBE CONVOLVED WITH A COSINE OR GGX LOBE, AND THE TRANSPOSE (srz_cube_prefilter, srz_cube_prefilter_grad;
// include/srz.h states the rule).  The one all-pairs kernel here, bound by the vector ALU: a lane OWNS one texel of one cube (the
// forward's output texel, the backward's source texel) with its direction in registers, and every lane WALKS the other cube's texels
// in the same order, so the walked direction, jac and channel values are wave-uniform and arrive through the scalar cache
// (k_light's parameter frame).  k_prefilter_table writes the walked cube's {d, jac} once per call; a lane computes its own texel
// with the same function, so both sides are the same words.  A pair costs the dot product, the clamp, the test and the weight
// (COSINE: one multiply; GGX: two fma's, two multiplies and the IEEE division) against n_ch + 1 fma's: the weight is generated per
// group of PREFILTER_CG channels, a wider cube walks again.  A skipped pair is a select that keeps the sums, never a product with 0.
// The walk is cut by blockIdx.y into pieces of whole rows (srz_device.h: prefilter_chunks) whose partial sums k_prefilter_rows and
// k_prefilter_fold add in the rule's order; the fold divides in the forward.  No LDS, no barrier, no atomics.
// ================================================================================================================
struct alignas(16) PfTexel {
  float x, y, z, jac;
};
__device__ __forceinline__ PfTexel pf_texel(uint32_t N, uint32_t texel) {
  const uint32_t f = texel / (N * N), r = texel % (N * N), y = r / N, x = r % N;
  const float s = (float)(2u * x + 1u) / (float)N - 1.0f, t = (float)(2u * y + 1u) / (float)N - 1.0f;
  const float r2 = fmaf_(s, s, fmaf_(t, t, 1.0f));
  const float inv = 1.0f / __builtin_sqrtf(r2);
  float px, py, pz; // n_f + s su_f + t sv_f by include/srz.h's table of the faces
  switch (f) {
  case 0u: px = 1.0f, py = -t, pz = -s; break;
  case 1u: px = -1.0f, py = -t, pz = s; break;
  case 2u: px = s, py = 1.0f, pz = t; break;
  case 3u: px = s, py = -1.0f, pz = -t; break;
  case 4u: px = s, py = -t, pz = 1.0f; break;
  default: px = -s, py = -t, pz = -1.0f; break;
  }
  return {px * inv, py * inv, pz * inv, (inv * inv) * inv};
}
__global__ __launch_bounds__(256) void k_prefilter_table(PfTexel *tab, uint32_t N) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < 6u * N * N) tab[i] = pf_texel(N, i);
}
// the backward's q = den > 0 ? gdst / den : 0, [frames][n_out][C]
__global__ __launch_bounds__(256) void k_prefilter_q(const float *gdst, const float *den, float *q, uint32_t n_out, uint32_t C, uint32_t frames) {
  const size_t per = (size_t)n_out * C, i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= per * frames) return;
  const float d = den[(i % per) / C];
  q[i] = d > 0.0f ? gdst[i] / d : 0.0f;
}
struct PfWalk {
  const PfTexel *tab; // the walked cube's table
  const float *val;   // the walked values [frame][6 n_walk^2][C]
  float *part;        // [chunk][frame][6 n_own^2][CS]
  uint32_t n_own, n_walk, C, CS, frames, chunks, kind;
  float a2m1, cmin;
};
// one lane's walk over the rows [g0, g1) of the 6 n_walk rows for NC channels from ch0
template <bool BWD, int NC>
__device__ __forceinline__ void pf_walk(const PfWalk &a, const PfTexel &me, uint32_t frame, uint32_t ch0, uint32_t g0, uint32_t g1, float (&cube)[NC],
                                        float &cube_den) {
  const SRZ_CAS PfTexel *tab = as_const(a.tab);
  const SRZ_CAS float *val = as_const(a.val) + (size_t)frame * 6u * a.n_walk * a.n_walk * a.C + ch0;
  const bool ggx = a.kind == SRZ_PREFILTER_GGX;
  for (int k = 0; k < NC; ++k) cube[k] = 0.0f;
  cube_den = 0.0f;
  for (uint32_t g = g0; g < g1;) {
    const uint32_t face_end = (g / a.n_walk + 1u) * a.n_walk, stop = face_end < g1 ? face_end : g1;
    float face[NC], face_den = 0.0f;
    for (int k = 0; k < NC; ++k) face[k] = 0.0f;
    for (; g < stop; ++g) {
      float row[NC], row_den = 0.0f;
      for (int k = 0; k < NC; ++k) row[k] = 0.0f;
      const size_t first = (size_t)g * a.n_walk;
#pragma unroll 4
      for (uint32_t x = 0; x < a.n_walk; ++x) {
        const SRZ_CAS PfTexel *t = tab + first + x;
        float c = fmaf_(me.x, t->x, fmaf_(me.y, t->y, me.z * t->z));
        c = c > 1.0f ? 1.0f : c;
        const bool take = c > a.cmin;
        float w = c * (BWD ? me.jac : t->jac);
        if (ggx) {
          const float nh2 = fmaf_(0.5f, c, 0.5f);
          const float u = fmaf_(nh2, a.a2m1, 1.0f);
          w = w / (u * u);
        }
        if (!BWD) row_den = take ? row_den + w : row_den;
        for (int k = 0; k < NC; ++k) row[k] = take ? fmaf_(w, val[(first + x) * a.C + k], row[k]) : row[k];
      }
      if (!BWD) face_den = face_den + row_den;
      for (int k = 0; k < NC; ++k) face[k] = face[k] + row[k];
    }
    if (!BWD) cube_den = cube_den + face_den;
    for (int k = 0; k < NC; ++k) cube[k] = cube[k] + face[k];
  }
}
template <bool BWD, int NC> __device__ __forceinline__ void pf_group(const PfWalk &a, const PfTexel &me, uint32_t own, bool live, uint32_t frame, uint32_t ch0) {
  const uint32_t per = 6u * a.n_walk / a.chunks; // rows per piece: the cube's, a face's, or one
  float cube[NC], den;
  pf_walk<BWD, NC>(a, me, frame, ch0, blockIdx.y * per, (blockIdx.y + 1u) * per, cube, den);
  if (!live) return;
  float *p = a.part + (((size_t)blockIdx.y * a.frames + frame) * (6u * a.n_own * a.n_own) + own) * a.CS;
  for (int k = 0; k < NC; ++k) p[ch0 + k] = cube[k];
  if (!BWD && ch0 == 0u) p[a.C] = den;
}
template <bool BWD> __global__ __launch_bounds__(256) void k_prefilter(PfWalk a) {
  const uint32_t n_own = 6u * a.n_own * a.n_own, own = blockIdx.x * 256u + threadIdx.x;
  const bool live = own < n_own; // (a lane past the cube walks with texel 0's direction and writes nothing)
  const PfTexel me = pf_texel(a.n_own, live ? own : 0u);
  const uint32_t groups = (a.C + PREFILTER_CG - 1u) / PREFILTER_CG;
  for (uint32_t fg = blockIdx.z; fg < a.frames * groups; fg += gridDim.z) { // (wave-uniform)
    const uint32_t frame = fg / groups, ch0 = (fg % groups) * PREFILTER_CG, nc = a.C - ch0;
    if (nc >= 4u) pf_group<BWD, 4>(a, me, own, live, frame, ch0);
    else if (nc == 3u) pf_group<BWD, 3>(a, me, own, live, frame, ch0);
    else if (nc == 2u) pf_group<BWD, 2>(a, me, own, live, frame, ch0);
    else pf_group<BWD, 1>(a, me, own, live, frame, ch0);
  }
}
// a walk cut into rows: every face's rows added in order, a thread per (face, frame, texel, slot) — consecutive threads, consecutive
// floats of a piece — into `faces`, the partial sums a walk cut into faces would have left
__global__ __launch_bounds__(256) void k_prefilter_rows(PfWalk a, float *faces) {
  const size_t piece = (size_t)a.frames * (6u * a.n_own * a.n_own) * a.CS, i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= 6u * piece) return;
  const uint32_t per_face = a.chunks / 6u;
  const float *p = a.part + (i / piece) * per_face * piece + i % piece;
  float face = 0.0f;
  for (uint32_t y = 0; y < per_face; ++y) face = face + p[(size_t)y * piece];
  faces[i] = face;
}
// slot `e` of texel `own` of `frame`: the cube's sum itself, or the six faces' partial sums added in order
__device__ __forceinline__ float pf_fold(const PfWalk &a, uint32_t frame, uint32_t own, uint32_t e) {
  const size_t piece = (size_t)a.frames * (6u * a.n_own * a.n_own) * a.CS;
  const float *p = a.part + ((size_t)frame * (6u * a.n_own * a.n_own) + own) * a.CS + e;
  if (a.chunks == 1u) return p[0];
  float cube = 0.0f;
  for (uint32_t f = 0; f < 6u; ++f) cube = cube + p[f * piece];
  return cube;
}
// out: the forward's dst (num / den, and den itself into den_out when non-null) or the backward's gsrc (the sum)
template <bool BWD> __global__ __launch_bounds__(256) void k_prefilter_fold(PfWalk a, float *out, float *den_out) {
  const uint32_t n_own = 6u * a.n_own * a.n_own;
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= (size_t)n_own * a.frames) return;
  const uint32_t frame = (uint32_t)(i / n_own), own = (uint32_t)(i % n_own);
  float den = 1.0f;
  if (!BWD) {
    den = pf_fold(a, frame, own, a.C);
    if (den_out && frame == 0u) den_out[own] = den;
  }
  for (uint32_t ch = 0; ch < a.C; ++ch) {
    const float num = pf_fold(a, frame, own, ch);
    out[i * a.C + ch] = BWD ? num : (den > 0.0f ? num / den : 0.0f);
  }
}

// ================================================================================================================
// SH9 LIGHTING (srz_cube_sh, srz_frameset_sh and their backwards; include/srz.h states the rules and the constants).
// sh_poly is the polynomials' text for both pieces; sh_yc / sh_h the constants by k.
//   k_cube_sh         a cube -> the row partials of its nine coefficients per channel and of the normaliser: ONE WAVE PER FACE ROW,
//                     lane j the columns j, j + 64, ..., pf_texel for the geometry (k_prefilter's, so the same words), the channels
//                     PREFILTER_CG at a time in registers, the butterfly, lane 0's ordinary stores into work[row][K].  k_light_fold adds
//                     a face's rows, then a frame's faces; k_cube_sh_finish divides.  No LDS, no barrier, no atomics.
//   k_cube_sh_grad    the backward, a gather: a lane per source texel, q (k_cube_sh_q wrote it) wave-uniform through the scalar cache.
//   k_sh              coefficients evaluated at each pixel's normal: k_light's shape on the passes' helpers, the coefficients read as
//                     k_light reads its parameter frame; no LDS, no barrier; 16 bytes read and 4 n_ch written per owned pixel.
//   k_sh_grad         gout -> gnrm (per pixel, from registers) and, WANT_SH, the tiles' partial sums of gsh in k_light_grad's fixed
//                     tree, word for word; the CHANNELS are the outer loop, so a lane holds nine sums at a time.  k_light_fold as there.
// ================================================================================================================
constexpr float SH_FOURPI = 12.566371f;
__device__ __forceinline__ float sh_yc(int k) {
  constexpr float c[5] = {0x1.20dd76p-2f, 0x1.f45438p-2f, 0x1.17b142p+0f, 0x1.42f602p-2f, 0x1.17b142p-1f};
  constexpr int idx[9] = {0, 1, 1, 1, 2, 2, 3, 2, 4};
  return c[idx[k]];
}
__device__ __forceinline__ float sh_h(int k) {
  constexpr float c[5] = {0x1.20dd76p-2f, 0x1.4d8d7ap-2f, 0x1.17b142p-2f, 0x1.42f602p-4f, 0x1.17b142p-3f};
  constexpr int idx[9] = {0, 1, 1, 1, 2, 2, 3, 2, 4};
  return c[idx[k]];
}
__device__ __forceinline__ void sh_poly(float x, float y, float z, float (&p)[9]) {
  p[0] = 1.0f, p[1] = y, p[2] = z, p[3] = x, p[4] = x * y, p[5] = y * z;
  p[6] = fmaf_(3.0f * z, z, -1.0f), p[7] = x * z, p[8] = fmaf_(x, x, -(y * y));
}
// w_k = jac * (Yc[k] * p_k(d)) of a texel
__device__ __forceinline__ void sh_texel_weights(const PfTexel &t, float (&w)[9]) {
  float p[9];
  sh_poly(t.x, t.y, t.z, p);
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = t.jac * (sh_yc(k) * p[k]);
}
// one wave, one face row (row: frame * 6 n + face * n + y), NC channels from ch0; den with the first group
template <int NC> __device__ __forceinline__ void cube_sh_row(const CubeShArgs &a, uint64_t row, uint32_t ch0, uint32_t lane) {
  const uint32_t n = a.n, C = a.n_ch, K = 9u * C + 1u;
  const uint32_t r = (uint32_t)(row % (6u * n)); // face * n + y: the row within its cube
  const float *src = a.src + ((size_t)(row / (6u * n)) * 6u * n * n + (size_t)r * n) * C + ch0;
  float acc[9][NC], den = 0.0f;
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[k][i] = 0.0f;
  for (uint32_t x = lane; x < n; x += 64u) {
    const PfTexel t = pf_texel(n, r * n + x);
    float w[9], v[NC];
    sh_texel_weights(t, w);
#pragma unroll
    for (int i = 0; i < NC; ++i) v[i] = src[(size_t)x * C + i];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
      for (int i = 0; i < NC; ++i) acc[k][i] = fmaf_(w[k], v[i], acc[k][i]);
    den = den + t.jac;
  }
  float *part = a.work + (size_t)row * K;
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const float s = light_wave_sum(acc[k][i]);
      if (lane == 0u) part[(uint32_t)k * C + ch0 + (uint32_t)i] = s;
    }
  if (ch0 == 0u) {
    const float s = light_wave_sum(den);
    if (lane == 0u) part[9u * C] = s;
  }
}
__global__ __launch_bounds__(256) void k_cube_sh(CubeShArgs a) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint64_t rows = (uint64_t)a.frames * 6u * a.n;
  for (uint64_t row = (uint64_t)blockIdx.x * 4u + wave; row < rows; row += (uint64_t)gridDim.x * 4u) // (wave-uniform)
    for (uint32_t ch0 = 0; ch0 < a.n_ch; ch0 += PREFILTER_CG) {
      const uint32_t nc = a.n_ch - ch0;
      if (nc >= 4u) cube_sh_row<4>(a, row, ch0, lane);
      else if (nc == 3u) cube_sh_row<3>(a, row, ch0, lane);
      else if (nc == 2u) cube_sh_row<2>(a, row, ch0, lane);
      else cube_sh_row<1>(a, row, ch0, lane);
    }
}
// cube: [frame][K] sums, the last slot den -> sh [frame][9][n_ch], and frame 0's den into den_out when non-null
__global__ __launch_bounds__(256) void k_cube_sh_finish(const float *cube, float *sh, float *den_out, uint32_t C, uint32_t frames) {
  const uint32_t per = 9u * C, i = blockIdx.x * 256u + threadIdx.x;
  if (i >= per * frames) return;
  const float *row = cube + (size_t)(i / per) * (per + 1u);
  const float den = row[per];
  sh[i] = (SH_FOURPI * row[i % per]) / den;
  if (den_out && i == 0u) den_out[0] = den;
}
// the backward's q = (FOURPI * gsh) / den, [frames][9][n_ch]
__global__ __launch_bounds__(256) void k_cube_sh_q(const float *gsh, const float *den, float *q, uint32_t count) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < count) q[i] = (SH_FOURPI * gsh[i]) / den[0];
}
__global__ __launch_bounds__(256) void k_cube_sh_grad(CubeShArgs a) {
  const uint32_t C = a.n_ch, texels = 6u * a.n * a.n, bpf = (texels + 255u) / 256u;
  const uint64_t total = (uint64_t)a.frames * bpf;
  for (uint64_t b = blockIdx.x; b < total; b += gridDim.x) {
    const uint32_t frame = (uint32_t)(b / bpf), texel = (uint32_t)(b % bpf) * 256u + threadIdx.x;
    if (texel >= texels) continue;
    const SRZ_CAS float *q = as_const(a.work) + (size_t)frame * 9u * C; // (wave-uniform: scalar loads)
    float w[9];
    sh_texel_weights(pf_texel(a.n, texel), w);
    float *g = a.dst + ((size_t)frame * texels + texel) * C;
    for (uint32_t c = 0; c < C; ++c) {
      float v = w[0] * q[c];
#pragma unroll
      for (uint32_t k = 1; k < 9u; ++k) v = fmaf_(w[k], q[k * C + c], v);
      g[c] = v;
    }
  }
}

struct ShPx {
  float N[3], inl;
  float e[9]; // e_k = K[k] * p_k(N), e_0 = K[0]
};
// what k_sh and k_sh_grad do alike in front of the channels: the owners, the normals of a quad with an owner, the lit pixels' ShPx
// -> `own` and `lit`, one bit per pixel
__device__ __forceinline__ void sh_quad(const ShArgs &a, const PassTile &t, ShPx (&px)[4], uint32_t &own, uint32_t &lit) {
  uint32_t id[4];
  own = quad_ids(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id), lit = 0u;
  if (own == 0u) return;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 n[3] = {zero4, zero4, zero4};
  quad_load(a.nrm + (size_t)t.f * a.nrm_stride + t.poff, t.rc.plane, n, t.whole, t.x4, t.rc.tx1);
  const bool rad = a.kind == SRZ_SH_RADIANCE;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!(own & (1u << k))) continue;
    const float nk[3] = {quad_at(n[0], k), quad_at(n[1], k), quad_at(n[2], k)};
    const float nn = l_dot(nk, nk);
    if (!l_pos(nn)) continue;
    lit |= 1u << k;
    ShPx &p = px[k];
    p.inl = l_rsqrt(nn);
#pragma unroll
    for (int i = 0; i < 3; ++i) p.N[i] = nk[i] * p.inl;
    float poly[9];
    sh_poly(p.N[0], p.N[1], p.N[2], poly);
    p.e[0] = rad ? sh_yc(0) : sh_h(0);
#pragma unroll
    for (int j = 1; j < 9; ++j) p.e[j] = (rad ? sh_yc(j) : sh_h(j)) * poly[j];
  }
}
__global__ __launch_bounds__(256) void k_sh(ShArgs a) {
  const uint32_t C = a.n_ch;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool fused = t.fused(a.flags_or);
    const SRZ_CAS float *sh = as_const(a.sh) + (size_t)t.f * a.sh_stride;
    ShPx px[4];
    uint32_t own, lit;
    sh_quad(a, t, px, own, lit);
    if (own == 0u && !fused) return;
    for (uint32_t c = 0; c < C; ++c) {
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f); // nobody, and an owner that is not lit: zeros
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(lit & (1u << k))) continue;
        float v = sh[c] * px[k].e[0];
#pragma unroll
        for (uint32_t j = 1; j < 9u; ++j) v = fmaf_(sh[j * C + c], px[k].e[j], v);
        quad_at(o, k) = v;
      }
      quad_store_owned(t.out + (size_t)c * t.rc.plane, t, {o}, fused, own);
    }
  });
}
template <bool WANT_SH> __global__ __launch_bounds__(256) void k_sh_grad(ShArgs a) {
  __shared__ float s_part[WANT_SH ? 4 : 1][WANT_SH ? 64 : 1];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t C = a.n_ch, K = 9u * C, tpf = a.n_local_bands * a.tiles_x;
  const bool rad = a.kind == SRZ_SH_RADIANCE;
  pass_tiles(a, [&](uint32_t f, uint32_t ti) {
    const PassTile t = pass_tile(a, f, ti);
    const bool fused = t.fused(a.flags_or);
    const SRZ_CAS float *sh = as_const(a.sh) + (size_t)f * a.sh_stride;
    float *gn_out = a.gnrm ? a.gnrm + (size_t)f * a.nrm_stride + t.poff : nullptr;
    // ---- 1. owners, normals, the lit pixels
    ShPx px[4];
    uint32_t own, lit;
    sh_quad(a, t, px, own, lit);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (WANT_SH) {
      // a tile without a lit pixel: its partials are the empty sums, +0, what the tree below gives too, without the shuffles
      if (!__syncthreads_or(lit != 0u)) {
        if (gn_out && t.inside && (own != 0u || fused)) {
          const float4 z[3] = {zero4, zero4, zero4};
          quad_store_owned(gn_out, t, z, fused, own);
        }
        if (tid < K) a.work[((size_t)f * tpf + ti) * K + tid] = 0.0f;
        return;
      }
    }
    // ---- 2. the channels: ge_k summed over them ascending; a channel's nine lane sums reduced and put into LDS as it ends
    float ge[4][9];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 9; ++j) ge[k][j] = 0.0f;
    for (uint32_t c = 0; c < C; ++c) {
      float4 g[1] = {zero4};
      if (lit != 0u) quad_load(a.gout + (size_t)f * a.frame_stride + (size_t)c * t.rc.plane + t.poff, t.rc.plane, g, t.whole, t.x4, t.rc.tx1);
      float tl[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; // this lane's sums of the channel's terms
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(lit & (1u << k))) continue;
        const float gc = quad_at(g[0], k);
#pragma unroll
        for (uint32_t j = 0; j < 9u; ++j) {
          if (WANT_SH) tl[j] = tl[j] + gc * px[k].e[j];
          if (j != 0u) ge[k][j] = c == 0u ? gc * sh[j * C] : fmaf_(gc, sh[j * C + c], ge[k][j]);
        }
      }
      if (WANT_SH) { // (every lane of the workgroup is here: the walk and the channel count are uniform)
#pragma unroll
        for (uint32_t j = 0; j < 9u; ++j) {
          const float v = light_wave_sum(tl[j]);
          if (lane == 0u) s_part[wave][j * C + c] = v;
        }
      }
    }
    // ---- 3. the normal's gradient through the polynomials and the normalisation
    if (gn_out && t.inside && (own != 0u || fused)) {
      float4 gn[3] = {zero4, zero4, zero4};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(lit & (1u << k))) continue;
        const float x = px[k].N[0], y = px[k].N[1], z = px[k].N[2];
        float gp[9];
#pragma unroll
        for (int j = 1; j < 9; ++j) gp[j] = ge[k][j] * (rad ? sh_yc(j) : sh_h(j));
        const float gN[3] = {fmaf_(2.0f * x, gp[8], fmaf_(gp[7], z, fmaf_(gp[4], y, gp[3]))),
                             fmaf_(-2.0f * y, gp[8], fmaf_(gp[5], z, fmaf_(gp[4], x, gp[1]))),
                             fmaf_(6.0f * z, gp[6], fmaf_(gp[7], x, fmaf_(gp[5], y, gp[2])))};
        const float d = l_dot(gN, px[k].N);
#pragma unroll
        for (int i = 0; i < 3; ++i) quad_at(gn[i], k) = (gN[i] - px[k].N[i] * d) * px[k].inl;
      }
      quad_store_owned(gn_out, t, gn, fused, own);
    }
    // ---- 4. the tile's K partial sums
    if (WANT_SH) {
      __syncthreads();
      if (tid < K) a.work[((size_t)f * tpf + ti) * K + tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
      __syncthreads(); // s_part is the next tile's too
    }
  });
}

// ================================================================================================================
// k_interp_deriv — SCREEN-SPACE DERIVATIVES OF CALLER ATTRIBUTES (srz_frameset_interpolate_deriv, include/srz.h): interpolation is
// affine in the sample point with owners held fixed (k_pos_grad's ∇α, ∇β), so channel ch of the owner changes per one-pixel step by
// (a − c) ∇α + (b − c) ∇β: a constant of the triangle.  k_interp's walk, loads and stores (no LDS, no barrier), plus load_pos9 of
// the owner as k_pos_grad has it, once per run of one owner within the quad; planes 2 ch (d/dx) and 2 ch + 1 (d/dy).  The class bit
// plays no part.  The floor is the memory system: 4 bytes of id per pixel; 36 + 12 n_ch of gather per owned pixel; 8 n_ch written.
// ================================================================================================================
struct DerivTri {
  float gax, gay, gbx, gby; // ∇α, ∇β
};
__device__ __forceinline__ DerivTri deriv_tri(const SRZ_CAS float *p) {
  float P[9]; // ax ay z0 bx by z1 cx cy z2
  load_pos9(p, P);
  const float area = (P[3] - P[0]) * (P[7] - P[1]) - (P[4] - P[1]) * (P[6] - P[0]);
  const float r = 1.0f / area; // (the IEEE division)
  return {(P[4] - P[7]) * r, (P[6] - P[3]) * r, (P[7] - P[1]) * r, (P[0] - P[6]) * r};
}
__global__ __launch_bounds__(256) void k_interp_deriv(InterpDerivArgs a) {
  const uint32_t C = a.n_ch;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool fused = t.fused(a.flags_or);
    // ---- 1. owner indices + 1 (the class bit dropped)
    uint32_t id[4];
    const uint32_t own = quad_ids<~S_CLASS_BIT>(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id);
    if (own == 0u && !fused) return;
    // ---- 2. ∇α, ∇β of each owner, gathered once per run of one owner
    const SRZ_CAS float *tpos = as_const(a.tri_pos) + (size_t)t.fd->tri_off * a.pos_stride;
    DerivTri T[4] = {};
    {
      uint32_t prev = 0u;
      DerivTri cur = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (id[k] == 0u) continue;
        if (id[k] != prev) cur = deriv_tri(tpos + (size_t)(id[k] - 1u) * a.pos_stride), prev = id[k];
        T[k] = cur;
      }
    }
    const SRZ_CAS float *at = as_const(a.attr) + (size_t)t.f * a.attr_frame_stride;
    // ---- 3. the channels, ATTR_CHUNK at a time
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 qx[ATTR_CHUNK], qy[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) qx[i] = qy[i] = make_float4(0.f, 0.f, 0.f, 0.f); // nobody: zeros
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (id[k] == 0u) continue;
        const SRZ_CAS float *p = at + (size_t)(id[k] - 1u) * (3u * C) + c0;
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
          if (i < nc) {
            const float cc = p[2u * C + i], da = p[i] - cc, db = p[C + i] - cc;
            quad_at(qx[i], k) = fmaf_(da, T[k].gax, db * T[k].gbx);
            quad_at(qy[i], k) = fmaf_(da, T[k].gay, db * T[k].gby);
          }
      }
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
        if (i >= nc) break;
        quad_store_owned(t.out + (size_t)(2u * (c0 + i)) * t.rc.plane, t, {qx[i], qy[i]}, fused, own);
      }
    }
  });
}

// ================================================================================================================
// k_persp / k_persp_grad / k_interp_deriv_persp — PERSPECTIVE-CORRECT BARYCENTRICS (srz_frameset_perspective, _perspective_grad,
// _interpolate_deriv_persp; include/srz.h states the rule).  A visibility buffer's α, β are linear in screen space; with q_k the
// reciprocal clip w of the owner's corners, α' = α q0 / s, β' = β q1 / s, s = α q0 + β q1 + γ q2 are the weights of the point of
// the triangle that projects onto the pixel.  k_persp writes them into a buffer of the visibility buffer's own layout, so that
// k_interp, k_interp_grad, k_gbuffer and k_shade_vis run on it unchanged; z and the ids are copied.
//   k_persp               k_interp's shape: pass_walk<false>, no LDS, no barrier; quad_ids, the four planes' quads, three dwords of q
//                         gathered per run of one owner within the quad; EVERY pixel of the tile is written (the words of a pixel
//                         nobody owns are copied), so a partial quad is stored pixel by pixel whoever owns it.  Plain stores:
//                         k_interp reads the buffer next.  Floor: 16 bytes read and 16 written per pixel, 12 gathered per owned pixel.
//   k_persp_grad          k_pos_grad's four stages at three values per owner (g0 α, g1 β, g2 γ into gq): the quad's run sums, the
//                         segmented DPP row scan, the tile's open-addressed owner table in LDS, the listed flush with
//                         global_atomic_add_f32; an owner without a slot adds straight to memory.  pp_scan_step, pp_emit and the
//                         flush are COPIES of pg_scan_step, pg_emit and k_pos_grad's step 4 (themselves copies of ig_scan_step /
//                         ig_emit), for the reason given there; a fix goes into all three.  A pixel that is not valid takes no
//                         part in the sums: its key is 0, like a pixel nobody owns.  galpha, gbeta from registers, no atomics.
//                         Without gq there is no table and no barrier.
//   k_interp_deriv_persp  k_interp_deriv's shape plus the α, β quads and the q gather; the channels in chunks of ATTR_CHUNK.
// ================================================================================================================
struct PerspPx {
  float ap, bp, s; // α', β' (α, β themselves where the rule does not apply) and the denominator
  bool valid;
};
// (a positive normal float: x >= 2^-126 && x < inf; a NaN fails)
__device__ __forceinline__ bool persp_ok(float x) { return x >= 0x1p-126f && x < __builtin_inff(); }
__device__ __forceinline__ PerspPx persp_px(float al, float be, float ga, float q0, float q1, float q2) {
  const float n0 = al * q0, n1 = be * q1, n2 = ga * q2, s = (n0 + n1) + n2;
  const bool valid = persp_ok(q0) && persp_ok(q1) && persp_ok(q2) && persp_ok(s);
  return {valid ? n0 / s : al, valid ? n1 / s : be, s, valid}; // (the IEEE divisions)
}
__global__ __launch_bounds__(256) void k_persp(PerspArgs a) {
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const TileRect &rc = t.rc;
    const float *gv = a.vis + (size_t)t.f * a.vis_stride + t.poff; // plane 0
    // ---- 1. owner ids, and the words of all four planes (the id quad is the one quad_ids loaded)
    uint32_t id[4];
    const uint32_t own = quad_ids(t, gv, id);
    float4 v[4];
    v[0] = v[1] = v[2] = v[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    quad_load(gv, rc.plane, v, t.whole, t.x4, rc.tx1);
    // ---- 2. α', β' of the owned pixels, q gathered once per run of one owner
    if (own != 0u) {
      const SRZ_CAS float *qf = as_const(a.q) + (size_t)t.f * a.q_frame_stride;
      uint32_t prev = 0u;
      float q0 = 0.f, q1 = 0.f, q2 = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (id[k] == 0u) continue;
        const uint32_t key = id[k] & ~S_CLASS_BIT;
        if (key != prev) {
          const SRZ_CAS float *p = qf + (size_t)(key - 1u) * 3u;
          q0 = p[0], q1 = p[1], q2 = p[2], prev = key;
        }
        const float al = quad_at(v[2], k), be = quad_at(v[3], k);
        const float ga = (id[k] & S_CLASS_BIT) ? 1.0f - al - be : 1.0f - (al + be); // (cover_s / cover_v)
        const PerspPx r = persp_px(al, be, ga, q0, q1, q2);
        quad_at(v[2], k) = r.ap, quad_at(v[3], k) = r.bp;
      }
    }
    // ---- 3. all four planes, every pixel of the tile
    float *go = t.out;
    if (t.whole) {
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<float4 *>(go + i * rc.plane) = v[i];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (t.x4 + k <= rc.tx1)
#pragma unroll
          for (int i = 0; i < 4; ++i) go[i * rc.plane + k] = quad_at(v[i], k);
    }
  });
}

constexpr uint32_t PP_VALS = 3, PP_SLOTS_PER_WAVE = 64 / PP_VALS;
struct PerspTable {
  uint32_t key[IG_SLOTS];  // triangle index + 1; 0: free
  uint32_t used[IG_SLOTS]; // the slots taken, in arrival order
  uint32_t n_used[2];      // [tile parity]
  float val[IG_SLOTS * PP_VALS]; // [slot][corner]
};
template <int CTRL> __device__ __forceinline__ void pp_scan_step(float (&acc)[PP_VALS], uint32_t &stop) { // (pg_scan_step)
  const uint32_t up_stop = dpp_u32<CTRL>(stop);
#pragma unroll
  for (uint32_t e = 0; e < PP_VALS; ++e) {
    const float up = u2f(dpp_u32<CTRL>(f2u(acc[e])));
    if (!stop) acc[e] += up;
  }
  stop |= up_stop;
}
__device__ __forceinline__ void pp_emit(PerspTable &tb, uint32_t par, uint32_t key, const float (&acc)[PP_VALS], float *gq) { // (pg_emit)
  uint32_t h = (key * 0x9e3779b1u) >> (32u - IG_SLOT_BITS);
  bool found = false;
  for (uint32_t p = 0; p < IG_PROBES && !found; ++p) {
    const uint32_t old = atomicCAS(&tb.key[h], 0u, key);
    if (old == 0u) tb.used[atomicAdd(&tb.n_used[par], 1u)] = h; // (each slot is taken once: n_used <= IG_SLOTS)
    found = old == 0u || old == key;
    if (!found) h = (h + 1u) & (IG_SLOTS - 1u);
  }
  if (found) {
#pragma unroll
    for (uint32_t e = 0; e < PP_VALS; ++e) atomicAdd(&tb.val[h * PP_VALS + e], acc[e]);
  } else {
    float *g = gq + (size_t)(key - 1u) * PP_VALS;
#pragma unroll
    for (uint32_t e = 0; e < PP_VALS; ++e) global_add(g + e, acc[e]);
  }
}
// one owned pixel: galpha, gbeta (ga, gb themselves where the rule does not apply); a valid pixel with ACC: its three terms onto acc
template <bool ACC>
__device__ __forceinline__ bool pp_pixel(float al, float be, float ga, float q0, float q1, float q2, float gA, float gB, float &gx, float &gy,
                                         float (&acc)[PP_VALS]) {
  const PerspPx r = persp_px(al, be, ga, q0, q1, q2);
  gx = gA, gy = gB;
  if (r.valid) {
    const float tt = fmaf_(gA, r.ap, gB * r.bp), rs = 1.0f / r.s; // (the IEEE division)
    const float g0 = (gA - tt) * rs, g1 = (gB - tt) * rs, g2 = (-tt) * rs;
    const float m = g2 * q2;
    gx = fmaf_(g0, q0, -m), gy = fmaf_(g1, q1, -m);
    if (ACC) acc[0] += g0 * al, acc[1] += g1 * be, acc[2] += g2 * ga;
  }
  return r.valid;
}
__global__ __launch_bounds__(256) void k_persp_grad(PerspArgs a) {
  __shared__ PerspTable tb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool want_q = a.gq != nullptr, want_bary = a.out != nullptr; // (kernel arguments: every branch on them is wave-uniform)
  if (want_q) {
    for (uint32_t i = tid; i < IG_SLOTS; i += 256) tb.key[i] = 0u;
    for (uint32_t i = tid; i < IG_SLOTS * PP_VALS; i += 256) tb.val[i] = 0.0f;
    if (tid < 2) tb.n_used[tid] = 0u;
    __syncthreads();
  }
  uint32_t par = 0u; // the tile's parity in this workgroup's walk (the same in every thread: nobody skips a tile)
  pass_walk<true>(a, [&](const PassTile &t) { // (a thread outside the frame owns nothing, and still meets the barriers)
    const TileRect &rc = t.rc;
    const float *gv = a.vis + (size_t)t.f * a.vis_stride + t.poff; // plane 0 (z: never read)
    const float *gg = a.gbary_p + (size_t)t.f * a.frame_stride + t.poff;
    // ---- 1. owner ids
    uint32_t id[4], first = 0u;
    const uint32_t own = quad_ids(t, gv, id);
    bool one_owner = true; // every owned pixel of the quad has the same triangle (either class)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (id[k] == 0u) continue;
      const uint32_t key = id[k] & ~S_CLASS_BIT;
      one_owner = one_owner && (first == 0u || first == key);
      first = first == 0u ? key : first;
    }
    // ---- 2. α, β of a quad with an owner, each owner's γ by its class, and the gradient quads; words of nobody's pixels are
    //         loaded with their quad at most, never used
    float4 al, be, ga;
    quad_bary(t, gv, own, id, al, be, ga);
    float4 qa = make_float4(0.f, 0.f, 0.f, 0.f), qb = qa;
    if (own != 0u) {
      if (t.whole) {
        qa = *reinterpret_cast<const float4 *>(gg), qb = *reinterpret_cast<const float4 *>(gg + rc.plane);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (own & (1u << k)) quad_at(qa, k) = gg[k], quad_at(qb, k) = gg[rc.plane + k];
      }
    }
    // ---- 3. the pixels: galpha, gbeta into ox, oy; the three terms of a valid pixel onto the open run's sums
    float4 ox = make_float4(0.f, 0.f, 0.f, 0.f), oy = ox; // nobody: zeros
    float acc[PP_VALS] = {0.0f, 0.0f, 0.0f};
    uint32_t cur = 0u; // the open run's key: a pixel that is not valid opens none
    const SRZ_CAS float *qf = as_const(a.q) + (size_t)t.f * a.q_frame_stride;
    float *gqf = a.gq + (size_t)t.f * a.q_frame_stride;
    if (own != 0u && one_owner) { // one owner: one gather, the quad is one run
      const SRZ_CAS float *p = qf + (size_t)(first - 1u) * 3u;
      const float q0 = p[0], q1 = p[1], q2 = p[2];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (id[k] == 0u) continue;
        float gx, gy;
        const bool valid = want_q ? pp_pixel<true>(quad_at(al, k), quad_at(be, k), quad_at(ga, k), q0, q1, q2, quad_at(qa, k), quad_at(qb, k), gx, gy, acc)
                                  : pp_pixel<false>(quad_at(al, k), quad_at(be, k), quad_at(ga, k), q0, q1, q2, quad_at(qa, k), quad_at(qb, k), gx, gy, acc);
        quad_at(ox, k) = gx, quad_at(oy, k) = gy;
        if (valid) cur = first;
      }
    } else if (own != 0u) { // several owners (an edge crosses the quad): pixel after pixel, a run that ends goes into the table
      uint32_t prev = 0u; // the owner whose q is held
      float q0 = 0.f, q1 = 0.f, q2 = 0.f, run[PP_VALS] = {0.0f, 0.0f, 0.0f};
#pragma nounroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t idk = k == 0 ? id[0] : k == 1 ? id[1] : k == 2 ? id[2] : id[3];
        if (idk == 0u) continue;
        const uint32_t key = idk & ~S_CLASS_BIT;
        if (key != prev) {
          const SRZ_CAS float *p = qf + (size_t)(key - 1u) * 3u;
          q0 = p[0], q1 = p[1], q2 = p[2], prev = key;
        }
        run[0] = run[1] = run[2] = 0.0f;
        float gx, gy;
        const bool valid = want_q ? pp_pixel<true>(quad_pick(al, k), quad_pick(be, k), quad_pick(ga, k), q0, q1, q2, quad_pick(qa, k), quad_pick(qb, k), gx, gy, run)
                                  : pp_pixel<false>(quad_pick(al, k), quad_pick(be, k), quad_pick(ga, k), q0, q1, q2, quad_pick(qa, k), quad_pick(qb, k), gx, gy, run);
        quad_put(ox, k, gx), quad_put(oy, k, gy);
        if (want_q && valid) {
          if (cur != 0u && key != cur) {
            pp_emit(tb, par, cur, acc, gqf);
            acc[0] = acc[1] = acc[2] = 0.0f;
          }
          cur = key;
          acc[0] += run[0], acc[1] += run[1], acc[2] += run[2];
        }
      }
    }
    if (want_q) {
      // the key a quad of one owner takes into the row's scan; 0: the quad emits its runs itself, or has none
      const uint32_t skey = own != 0u && one_owner ? cur : 0u;
      const bool scan = __builtin_amdgcn_ballot_w64(skey != 0u) != 0ull; // (wave-uniform)
      const uint32_t pos = (uint32_t)lane & 7u;
      // (every lane executes both shifts: a lane that skipped one behind a short-circuit would be missing as its neighbour's source)
      const uint32_t key_left = dpp_u32<DPP_ROW_SHR1>(skey), key_right = dpp_u32<DPP_ROW_SHL1>(skey);
      const bool seg_head = (pos == 0u) | (key_left != skey) | (skey == 0u); // (a quad without a key takes no carry)
      const bool seg_last = (pos == 7u) | (key_right != skey);
      if (scan) { // inclusive segmented scan over the 8 quads of the tile row (Hillis-Steele: a lane past a head takes no carry)
        uint32_t stop = seg_head ? 1u : 0u; // (position p < d has stop set before the step of distance d: position 0 is a head)
        pp_scan_step<DPP_ROW_SHR1>(acc, stop);
        pp_scan_step<DPP_ROW_SHR2>(acc, stop);
        pp_scan_step<DPP_ROW_SHR4>(acc, stop);
      }
      // the last quad of a row's run holds the run's sum; a quad of several owners (a head: the scan left it alone) its last run
      const uint32_t ekey = skey != 0u ? (seg_last ? skey : 0u) : cur;
      if (ekey != 0u) pp_emit(tb, par, ekey, acc, gqf);
      // ---- 4. the table into memory, and emptied: PP_SLOTS_PER_WAVE slots per wave and pass, a slot's three floats on three
      //         consecutive lanes; the slot's first lane reads and frees the key, the others get it from that lane
      __syncthreads();
      const uint32_t n_used = tb.n_used[par];
      if (tid == 0) tb.n_used[par ^ 1u] = 0u; // (last read before the previous tile's second barrier, next added to behind this tile's)
      const uint32_t sl = (uint32_t)lane / PP_VALS, e = (uint32_t)lane - sl * PP_VALS;
      for (uint32_t base = (uint32_t)wave * PP_SLOTS_PER_WAVE; base < n_used; base += 4u * PP_SLOTS_PER_WAVE) { // (wave-uniform)
        const bool on = sl < PP_SLOTS_PER_WAVE && base + sl < n_used;
        uint32_t s = 0u, key = 0u;
        if (on) s = tb.used[base + sl];
        if (on && e == 0u) key = tb.key[s], tb.key[s] = 0u;
        key = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(sl * PP_VALS) << 2, (int)key); // (every lane executes it)
        if (on) {
          const float v = tb.val[s * PP_VALS + e];
          tb.val[s * PP_VALS + e] = 0.0f;
          global_add(gqf + (size_t)(key - 1u) * PP_VALS + e, v);
        }
      }
      __syncthreads();
      par ^= 1u;
    }
    // ---- 5. galpha, gbeta: whole quads (fused clear, or four owners), else the owned pixels only
    const bool fused = t.fused(a.flags_or);
    if (want_bary && t.inside && (own != 0u || fused)) quad_store_owned(t.out, t, {ox, oy}, fused, own);
  });
}

__global__ __launch_bounds__(256) void k_interp_deriv_persp(PerspDerivArgs a) {
  const uint32_t C = a.n_ch;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool fused = t.fused(a.flags_or);
    const float *gv = a.vis + (size_t)t.f * a.vis_stride + t.poff; // plane 0 (z: never read)
    // ---- 1. owner ids (the class bit kept: γ and the interpolated value follow it)
    uint32_t id[4];
    const uint32_t own = quad_ids(t, gv, id);
    if (own == 0u && !fused) return;
    // ---- 2. α, β, γ of the owned pixels; ∇α, ∇β and q of each owner, gathered once per run of one owner; then α', β', γ', s
    float4 al, be, ga;
    quad_bary(t, gv, own, id, al, be, ga);
    const SRZ_CAS float *tpos = as_const(a.tri_pos) + (size_t)t.fd->tri_off * a.pos_stride;
    const SRZ_CAS float *qf = as_const(a.q) + (size_t)t.f * a.q_frame_stride;
    DerivTri T[4] = {};
    float4 Q0 = make_float4(0.f, 0.f, 0.f, 0.f), Q1 = Q0, Q2 = Q0, S = Q0;
    uint32_t valid = 0u;
    {
      uint32_t prev = 0u;
      DerivTri cur = {0.f, 0.f, 0.f, 0.f};
      float q0 = 0.f, q1 = 0.f, q2 = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (id[k] == 0u) continue;
        const uint32_t key = id[k] & ~S_CLASS_BIT;
        if (key != prev) {
          cur = deriv_tri(tpos + (size_t)(key - 1u) * a.pos_stride);
          const SRZ_CAS float *p = qf + (size_t)(key - 1u) * 3u;
          q0 = p[0], q1 = p[1], q2 = p[2], prev = key;
        }
        T[k] = cur;
        const PerspPx r = persp_px(quad_at(al, k), quad_at(be, k), quad_at(ga, k), q0, q1, q2);
        if (r.valid) {
          valid |= 1u << k;
          quad_at(al, k) = r.ap, quad_at(be, k) = r.bp;
          quad_at(ga, k) = (id[k] & S_CLASS_BIT) ? 1.0f - r.ap - r.bp : 1.0f - (r.ap + r.bp); // (cover_s / cover_v)
          quad_at(Q0, k) = q0, quad_at(Q1, k) = q1, quad_at(Q2, k) = q2, quad_at(S, k) = r.s;
        }
      }
    }
    const SRZ_CAS float *at = as_const(a.attr) + (size_t)t.f * a.attr_frame_stride;
    // ---- 3. the channels, ATTR_CHUNK at a time
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 qx[ATTR_CHUNK], qy[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) qx[i] = qy[i] = make_float4(0.f, 0.f, 0.f, 0.f); // nobody: zeros
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (id[k] == 0u) continue;
        const SRZ_CAS float *p = at + (size_t)((id[k] & ~S_CLASS_BIT) - 1u) * (3u * C) + c0;
        const bool isS = (id[k] & S_CLASS_BIT) != 0u;
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
          if (i < nc) {
            const float ca = p[i], cb = p[C + i], cc = p[2u * C + i];
            if (valid & (1u << k)) {
              const float u = interp_ch(isS, quad_at(al, k), quad_at(be, k), quad_at(ga, k), ca, cb, cc);
              const float e0 = (ca - u) * quad_at(Q0, k), e1 = (cb - u) * quad_at(Q1, k), e2 = (cc - u) * quad_at(Q2, k);
              quad_at(qx[i], k) = fmaf_(e0 - e2, T[k].gax, (e1 - e2) * T[k].gbx) / quad_at(S, k); // (the IEEE divisions)
              quad_at(qy[i], k) = fmaf_(e0 - e2, T[k].gay, (e1 - e2) * T[k].gby) / quad_at(S, k);
            } else { // (k_interp_deriv's words)
              const float da = ca - cc, db = cb - cc;
              quad_at(qx[i], k) = fmaf_(da, T[k].gax, db * T[k].gbx);
              quad_at(qy[i], k) = fmaf_(da, T[k].gay, db * T[k].gby);
            }
          }
      }
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
        if (i >= nc) break;
        quad_store_owned(t.out + (size_t)(2u * (c0 + i)) * t.rc.plane, t, {qx[i], qy[i]}, fused, own);
      }
    }
  });
}

// ================================================================================================================
// k_tex_mip — THE TRILINEAR LOOKUP OVER A MIP PYRAMID (srz_frameset_texture_mip, include/srz.h states the rule): k_tex's walk and
// shape (no LDS, no barrier, 4 pixels of a row per thread, quad_store), plus the four derivative planes of a quad with a sampled
// pixel.  Per sampled pixel the level l0 and the fraction f come from mip_lod — compares, one sqrt, frexp: no transcendental — and
// the taps of level l0 and, ONLY where f != 0, of level l0 + 1 from tex_tap with that level's extents; a magnified pixel (f == 0 at
// level 0) costs what it costs in k_tex.  A level's extents are shifts of the texture's, its place in the pyramid a short sum over
// the levels before it (mip_texels_before): nothing is indexed by a per-lane level, nothing lives in scratch.
// l0 <= n_levels - 1 by the clamp in mip_lod; every texel index follows tex_axis's clamp within its level: no uv or derivative
// leaves the texture or the pyramid.
// ================================================================================================================
struct MipLod {
  uint32_t l0;
  float f;
};
__device__ __forceinline__ MipLod mip_lod(float ux, float uy, float vx, float vy, float Wf, float Hf, uint32_t L) {
  MipLod r = {L - 1u, 0.0f}; // not finite, or a footprint beyond the coarsest level
  const bool fin = tex_finite(ux) && tex_finite(uy) && tex_finite(vx) && tex_finite(vy);
  const float ax = ux * Wf, ay = vx * Hf, bx = uy * Wf, by = vy * Hf;
  const float rx = fmaf_(ax, ax, ay * ay), ry = fmaf_(bx, bx, by * by), r2 = rx > ry ? rx : ry;
  if (fin && r2 < __builtin_inff()) {
    const float rho = __builtin_sqrtf(r2); // (the IEEE square root)
    if (!(rho > 1.0f)) {
      r.l0 = 0u; // magnified, or no footprint
    } else {
      int e;
      const float m = __builtin_frexpf(rho, &e); // rho = m 2^e, 0.5 <= m < 1, 1 <= e <= 128
      const uint32_t l = (uint32_t)(e - 1);
      if (l < L - 1u) r.l0 = l, r.f = fmaf_(2.0f, m, -1.0f);
    }
  }
  return r;
}
// what k_tex_mip and k_tex_mip_grad do alike in front of their loops: the ids, the owners, u and v of a quad with an owner, the
// derivatives of a quad with a sampled pixel and the level of each -> `own` and `smp`, one bit per pixel (tex_quad, with levels)
__device__ __forceinline__ void mip_quad(const TexMipArgs &a, const SRZ_CAS FrameDesc *fd, const TileRect &rc, uint32_t f, size_t poff,
                                         bool inside, bool whole, int x4, float4 (&uv)[2], MipLod (&lod)[4], uint32_t &own, uint32_t &smp) {
  const float *gv = a.vis + (size_t)f * a.vis_stride + poff; // plane 0 (z: never read)
  uint32_t id[4] = {0u, 0u, 0u, 0u};
  if (inside) {
    if (whole) {
      const uint4 q = *reinterpret_cast<const uint4 *>(gv + rc.plane);
      id[0] = q.x, id[1] = q.y, id[2] = q.z, id[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x4 + k <= rc.tx1) id[k] = f2u(gv[rc.plane + k]);
    }
  }
  const uint32_t n_tris = fd->n_tris;
  own = 0u, smp = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    lod[k] = {0u, 0.0f};
    if ((id[k] & ~S_CLASS_BIT) - 1u < n_tris) own |= 1u << k; // (0 and the bare class bit wrap to 0xffffffff)
  }
  uv[0] = uv[1] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (own == 0u) return;
  quad_load(a.uv + (size_t)f * a.uv_stride + poff, rc.plane, uv, whole, x4, rc.tx1);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if ((own & (1u << k)) && tex_finite(quad_at(uv[0], k)) && tex_finite(quad_at(uv[1], k))) smp |= 1u << k;
  if (a.n_levels <= 1u || smp == 0u) return;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 d[4] = {zero, zero, zero, zero}; // (words of pixels that are not sampled: loaded with their quad at most, never used)
  quad_load(a.uvd + (size_t)f * a.vis_stride + poff, rc.plane, d, whole, x4, rc.tx1);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (smp & (1u << k))
      lod[k] = mip_lod(quad_at(d[0], k), quad_at(d[1], k), quad_at(d[2], k), quad_at(d[3], k), (float)a.tex_w, (float)a.tex_h, a.n_levels);
}
// level l of frame f: level 0 is the texture itself, the others lie in the pyramid behind the levels before them
template <class P>
__device__ __forceinline__ P *mip_level(P *tex, P *mip, uint32_t tex_w, uint32_t tex_h, uint32_t C, uint32_t tex_frames, uint32_t f, uint32_t l) {
  const size_t ft = tex_frames == 1u ? 0u : f, texels = (size_t)mip_extent(tex_w, l) * mip_extent(tex_h, l);
  return l == 0u ? tex + ft * texels * C : mip + ((size_t)mip_texels_before(tex_w, tex_h, l) * tex_frames + ft * texels) * C;
}
__device__ __forceinline__ float tex_bilinear(const SRZ_CAS float *t, const TexTap &p, uint32_t C, uint32_t ch) {
  const float t00 = t[(size_t)p.i00 * C + ch], t01 = t[(size_t)p.i01 * C + ch], t10 = t[(size_t)p.i10 * C + ch], t11 = t[(size_t)p.i11 * C + ch];
  const float top = fmaf_(p.tx, t01 - t00, t00), bot = fmaf_(p.tx, t11 - t10, t10);
  return fmaf_(p.ty, bot - top, top);
}
__global__ __launch_bounds__(256) void k_tex_mip(TexMipArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ly = wave * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
  const uint32_t tpf = a.n_local_bands * a.tiles_x, n_items = a.n_frames * tpf;
  const uint32_t C = a.n_ch;
  const bool wrap = a.mode == SRZ_TEX_WRAP;
  // workgroup b walks the frames f ≡ b mod 8 tile by tile (fewer than 8 frames: every 8th tile): an inline copy of pass_walk
  const uint32_t sub = blockIdx.x & 7u, step = gridDim.x >> 3;
  for (uint32_t j = blockIdx.x >> 3;; j += step) {
    uint32_t f, t;
    if (a.n_frames >= 8u) {
      f = sub + 8u * (j / tpf), t = j % tpf;
      if (f >= a.n_frames) break;
    } else {
      const uint32_t i = j * 8u + sub;
      if (i >= n_items) break;
      f = i / tpf, t = i % tpf;
    }
    const SRZ_CAS FrameDesc *fd = as_const(a.frames) + f;
    const uint32_t lb = t / a.tiles_x, tx = t % a.tiles_x;
    const TileRect rc = tile_rect(a, fd, f, lb, tx);
    const int W = fd->width;
    const int y = rc.ty0 + ly, x4 = rc.tx0 + lx4;
    if (!(y <= rc.ty1 && x4 <= rc.tx1)) continue; // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool whole = (W & 3) == 0 && x4 + 3 <= rc.tx1;
    const bool fused = ((fd->flags | a.flags_or) & SRZ_FUSED_CLEAR) != 0;
    const size_t poff = (size_t)lb * BAND * (size_t)W + (size_t)ly * (size_t)W + (size_t)x4;
    float *go = rc.out0 + (size_t)ly * (size_t)W + (size_t)x4;
    // ---- 1. owners, u and v, the levels
    float4 uv[2];
    MipLod lod[4];
    uint32_t own, smp;
    mip_quad(a, fd, rc, f, poff, true, whole, x4, uv, lod, own, smp);
    if (own == 0u && !fused) continue;
    // ---- 2. the taps of level l0 and, where f != 0, of level l0 + 1
    TexTap t0[4] = {}, t1[4] = {};
    const SRZ_CAS float *p0[4], *p1[4];
    uint32_t two = 0u; // the pixels that blend two levels
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      p0[k] = p1[k] = as_const(a.tex);
      if (!(smp & (1u << k))) continue;
      const uint32_t l = lod[k].l0;
      t0[k] = tex_tap(quad_at(uv[0], k), quad_at(uv[1], k), mip_extent(a.tex_w, l), mip_extent(a.tex_h, l), wrap);
      p0[k] = mip_level(as_const(a.tex), as_const(a.mip), a.tex_w, a.tex_h, C, a.tex_frames, f, l);
      if (lod[k].f != 0.0f) { // (l + 1 <= n_levels - 1: mip_lod gives f == 0 at the coarsest level)
        two |= 1u << k;
        t1[k] = tex_tap(quad_at(uv[0], k), quad_at(uv[1], k), mip_extent(a.tex_w, l + 1u), mip_extent(a.tex_h, l + 1u), wrap);
        p1[k] = mip_level(as_const(a.tex), as_const(a.mip), a.tex_w, a.tex_h, C, a.tex_frames, f, l + 1u);
      }
    }
    const bool quads = fused || own == 15u; // whole quads (fused clear, or four owners), else the owned pixels only
    // ---- 3. the channels, ATTR_CHUNK at a time
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 q[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) q[i] = make_float4(0.f, 0.f, 0.f, 0.f); // nobody, and an owner that is not sampled: zeros
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(smp & (1u << k))) continue;
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
          if (i < nc) {
            float c = tex_bilinear(p0[k], t0[k], C, c0 + i);
            if (two & (1u << k)) c = fmaf_(lod[k].f, tex_bilinear(p1[k], t1[k], C, c0 + i) - c, c);
            quad_at(q[i], k) = c;
          }
      }
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
        if (i >= nc) break;
        float *p = go + (size_t)(c0 + i) * rc.plane;
        if (quads) {
          quad_store(p, rc.plane, {q[i]}, whole, x4, rc.tx1);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (own & (1u << k)) p[k] = quad_at(q[i], k);
        }
      }
    }
  }
}

// ================================================================================================================
// k_tex_mip_grad — THE BACKWARD OF k_tex_mip (srz_frameset_texture_mip_grad), λ held fixed.  k_tex_grad's walk and barriers; two
// phases per tile, each with its own channel loop:
//   A. guv (from registers, deterministic): the bilinear pass's fma chains at level l0 and, where f != 0, at level l0 + 1, blended
//      by f as the forward blends the samples;
//   B. the texel adds, ONE LEVEL AT A TIME: the tile's pixels name the levels they touch in a word of LDS; for each of them the
//      tile's table phase runs as k_tex_grad has it — the slots of the level's taps (TexelTable keyed on the texel index WITHIN the
//      level), per chunk the LDS adds of (w_rc * lw) * gout, the dense flush into that level's gradient, the keys released.  The
//      table's capacity thus counts the distinct texels of ONE level, which a minified tile's footprint keeps near its pixel
//      count; the slot numbers of one level are live at a time (k_tex_grad's 16 registers, not 32).
// A pixel takes part in level l with lw = 1 - f when l == l0 and with lw = f when l == l0 + 1 and f != 0; its tap of the level is
// formed again from u and v (some thirty operations) rather than kept across the phases.
// Every thread of the workgroup reaches every barrier: the levels of a tile are read from LDS by all, a thread outside the frame
// samples nothing.  The level word rotates over three words by the tile's count, the next one zeroed in front of the barrier: one
// barrier per tile in front of the levels' own.
// ================================================================================================================
__global__ __launch_bounds__(256) void k_tex_mip_grad(TexMipArgs a) {
  __shared__ TexelTable<TexMipArgs, ATTR_CHUNK> tb;
  __shared__ uint32_t levels[3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ly = wave * 8 + (lane >> 3), lx4 = (lane & 7) * 4;
  const uint32_t tpf = a.n_local_bands * a.tiles_x, n_items = a.n_frames * tpf;
  const uint32_t C = a.n_ch;
  const bool want_tex = a.gtex != nullptr, want_uv = a.out != nullptr, wrap = a.mode == SRZ_TEX_WRAP;
  if (want_tex) {
    tb.init(tid);
    if (tid < 3) levels[tid] = 0u;
    __syncthreads();
  }
  uint32_t turn = 0u; // the tile's count in this workgroup's walk mod 3 (the same in every thread: nobody skips a tile)
  // workgroup b walks the frames f ≡ b mod 8 tile by tile (fewer than 8 frames: every 8th tile): an inline copy of pass_walk
  const uint32_t sub = blockIdx.x & 7u, step = gridDim.x >> 3;
  for (uint32_t j = blockIdx.x >> 3;; j += step) {
    uint32_t f, t;
    if (a.n_frames >= 8u) {
      f = sub + 8u * (j / tpf), t = j % tpf;
      if (f >= a.n_frames) break;
    } else {
      const uint32_t i = j * 8u + sub;
      if (i >= n_items) break;
      f = i / tpf, t = i % tpf;
    }
    const SRZ_CAS FrameDesc *fd = as_const(a.frames) + f;
    const uint32_t lb = t / a.tiles_x, tx = t % a.tiles_x;
    const TileRect rc = tile_rect(a, fd, f, lb, tx);
    const int W = fd->width;
    const int y = rc.ty0 + ly, x4 = rc.tx0 + lx4;
    const bool inside = y <= rc.ty1 && x4 <= rc.tx1; // (a thread outside the frame samples nothing, and still meets the barriers)
    const bool whole = (W & 3) == 0 && x4 + 3 <= rc.tx1;
    const bool fused = ((fd->flags | a.flags_or) & SRZ_FUSED_CLEAR) != 0;
    const size_t poff = (size_t)lb * BAND * (size_t)W + (size_t)ly * (size_t)W + (size_t)x4;
    const float *gg = a.gout + (size_t)f * a.gout_stride + poff;
    // ---- 1. owners, u and v, the levels
    float4 uv[2];
    MipLod lod[4];
    uint32_t own, smp;
    mip_quad(a, fd, rc, f, poff, inside, whole, x4, uv, lod, own, smp);
    // ---- A. du, dv
    if (want_uv && inside && (own != 0u || fused)) {
      TexTap t0[4] = {}, t1[4] = {};
      const SRZ_CAS float *p0[4], *p1[4];
      uint32_t two = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        p0[k] = p1[k] = as_const(a.tex);
        if (!(smp & (1u << k))) continue;
        const uint32_t l = lod[k].l0;
        t0[k] = tex_tap(quad_at(uv[0], k), quad_at(uv[1], k), mip_extent(a.tex_w, l), mip_extent(a.tex_h, l), wrap);
        p0[k] = mip_level(as_const(a.tex), as_const(a.mip), a.tex_w, a.tex_h, C, a.tex_frames, f, l);
        if (lod[k].f != 0.0f) {
          two |= 1u << k;
          t1[k] = tex_tap(quad_at(uv[0], k), quad_at(uv[1], k), mip_extent(a.tex_w, l + 1u), mip_extent(a.tex_h, l + 1u), wrap);
          p1[k] = mip_level(as_const(a.tex), as_const(a.mip), a.tex_w, a.tex_h, C, a.tex_frames, f, l + 1u);
        }
      }
      float au0[4] = {0.f, 0.f, 0.f, 0.f}, av0[4] = {0.f, 0.f, 0.f, 0.f}, au1[4] = {0.f, 0.f, 0.f, 0.f}, av1[4] = {0.f, 0.f, 0.f, 0.f};
      for (uint32_t c0 = 0; c0 < C && smp != 0u; c0 += ATTR_CHUNK) {
        const uint32_t nc = min(ATTR_CHUNK, C - c0);
        float4 g[ATTR_CHUNK];
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
          if (i >= nc) break;
          gout_quad(gg + (size_t)(c0 + i) * rc.plane, whole, smp, g[i]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!(smp & (1u << k))) continue;
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) {
              const float gi = quad_at(g[i], k);
              {
                const SRZ_CAS float *q = p0[k] + c0 + i;
                bilerp_chain(q + (size_t)t0[k].i00 * C, q + (size_t)t0[k].i01 * C, q + (size_t)t0[k].i10 * C, q + (size_t)t0[k].i11 * C, t0[k].tx,
                             t0[k].ty, gi, au0[k], av0[k]);
              }
              if (two & (1u << k)) {
                const SRZ_CAS float *q = p1[k] + c0 + i;
                bilerp_chain(q + (size_t)t1[k].i00 * C, q + (size_t)t1[k].i01 * C, q + (size_t)t1[k].i10 * C, q + (size_t)t1[k].i11 * C, t1[k].tx,
                             t1[k].ty, gi, au1[k], av1[k]);
              }
            }
        }
      }
      // whole quads (fused clear, or four owners), else the owned pixels only; an owner that is not sampled: (0, 0)
      float4 du = make_float4(0.f, 0.f, 0.f, 0.f), dv = du;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (smp & (1u << k)) {
          const uint32_t l = lod[k].l0;
          float u0 = t0[k].in_x ? au0[k] * (float)mip_extent(a.tex_w, l) : 0.0f, v0 = t0[k].in_y ? av0[k] * (float)mip_extent(a.tex_h, l) : 0.0f;
          if (two & (1u << k)) {
            const float u1 = t1[k].in_x ? au1[k] * (float)mip_extent(a.tex_w, l + 1u) : 0.0f;
            const float v1 = t1[k].in_y ? av1[k] * (float)mip_extent(a.tex_h, l + 1u) : 0.0f;
            u0 = fmaf_(lod[k].f, u1 - u0, u0), v0 = fmaf_(lod[k].f, v1 - v0, v0);
          }
          quad_at(du, k) = u0, quad_at(dv, k) = v0;
        }
      float *go = rc.out0 + (size_t)ly * (size_t)W + (size_t)x4;
      if (fused || own == 15u) {
        quad_store(go, rc.plane, {du, dv}, whole, x4, rc.tx1);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (own & (1u << k)) go[k] = quad_at(du, k), go[rc.plane + k] = quad_at(dv, k);
      }
    }
    if (!want_tex) continue;
    // ---- B. the texel adds: the levels this tile touches, then the table phase of each
    {
      uint32_t mine = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (smp & (1u << k)) mine |= (lod[k].f != 0.0f ? 3u : 1u) << lod[k].l0; // (l0 + 1 <= n_levels - 1 <= 14 where f != 0)
      if (mine != 0u) atomicOr(&levels[turn], mine);
      if (tid == 0) levels[turn == 2u ? 0u : turn + 1u] = 0u; // (last read two tiles ago, in front of the previous tile's barrier)
    }
    __syncthreads();
    uint32_t todo = __builtin_amdgcn_readfirstlane(levels[turn]);
    turn = turn == 2u ? 0u : turn + 1u;
    for (; todo != 0u; todo &= todo - 1u) {
      const uint32_t l = (uint32_t)__builtin_ctz(todo), wl = mip_extent(a.tex_w, l), hl = mip_extent(a.tex_h, l);
      float *gdst = mip_level(a.gtex, a.gmip, a.tex_w, a.tex_h, C, a.tex_frames, f, l);
      // ---- B1. the pixels of this level, their taps and level weights, the slots of their corners
      TexTap tap[4] = {};
      float lw[4] = {0.f, 0.f, 0.f, 0.f};
      uint32_t part = 0u;
      uint32_t slot[4][4] = {};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(smp & (1u << k))) continue;
        const bool lower = lod[k].l0 == l, upper = lod[k].l0 + 1u == l && lod[k].f != 0.0f;
        if (!lower && !upper) continue;
        part |= 1u << k;
        lw[k] = lower ? 1.0f - lod[k].f : lod[k].f;
        tap[k] = tex_tap(quad_at(uv[0], k), quad_at(uv[1], k), wl, hl, wrap);
        slot[k][0] = tb.slot(tap[k].i00), slot[k][1] = tb.slot(tap[k].i01), slot[k][2] = tb.slot(tap[k].i10), slot[k][3] = tb.slot(tap[k].i11);
      }
      const auto at = [=](uint32_t idx) { return gdst + (size_t)idx * C; };
      uint32_t n_used = 0u;
      // ---- B2. the channels, ATTR_CHUNK at a time
      for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
        const uint32_t nc = min(ATTR_CHUNK, C - c0);
        float4 g[ATTR_CHUNK];
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (part != 0u) {
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
            if (i >= nc) break;
            gout_quad(gg + (size_t)(c0 + i) * rc.plane, whole, part, g[i]);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (part & (1u << k)) {
            const CornerW w = corner_weights(tap[k].tx, tap[k].ty, lw[k]);
#pragma unroll
            for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
              if (i < nc) corner_adds(tb, slot[k], tap[k], w, quad_at(g[i], k), i, gdst, C, c0 + i);
          }
        n_used = tb.flush(tid, c0, nc, at); // ---- B3. the table's values of this chunk into memory (k_tex_grad's step 4)
      }
      tb.release(tid, n_used); // the level's keys go
    }
  }
}

// ================================================================================================================
// k_cube_mip — A CUBE MAP'S MIP PYRAMID LOOKED UP BY DIRECTION AND LEVEL (srz_frameset_texture_cube_mip, include/srz.h states the
// rule): k_cube's walk and shape (pass_walk, no LDS, no barrier, quad_ids, quad_store_owned) with k_tex_mip's blend of two levels.
// The level is the caller's plane lam, clamped into [0, n_levels - 1] (cube_lod).  cube_face runs once per pixel — the face, its
// seams, s and t do not depend on the level —, cube_corners once per level read, with that level's face size: every level is a cube
// of its own, so a corner that leaves its face resolves within its level.  Level l of a frame lies at cube_level_ptr: the cube is
// 6 * tex_frames textures of n x n to the pyramid's layout.  A pixel with f == 0 reads one level and costs what it costs in k_cube;
// the wave skips the second level's gathers when none of its lanes blends.
// l0 <= n_levels - 1 and l0 + 1 <= n_levels - 1 where f != 0 by cube_lod's clamps; every texel index follows cube_axis's clamp within
// its level: no direction and no lam leaves the cube or the pyramid.
// ================================================================================================================
struct CubeCorners {
  uint32_t i00, i01, i10, i11;
  float tx, ty;
};
// the level and the fraction of a caller's lam (MipLod: k_tex_mip's pair)
__device__ __forceinline__ MipLod cube_lod(float lam, uint32_t L) {
  MipLod r = {0u, 0.0f};
  if (!(lam > 0.0f)) return r; // NaN, negative, +-0
  if (lam >= (float)(L - 1u)) {
    r.l0 = L - 1u; // (+inf too)
    return r;
  }
  const float lf = __builtin_floorf(lam);
  r.l0 = min((uint32_t)(int)lf, L - 1u), r.f = lam - lf; // (the clamp never changes a value: 0 < lam < L - 1)
  return r;
}
__device__ __forceinline__ CubeCorners cube_corners_of(const CubeFace &c, uint32_t N) {
  CubeCorners p;
  cube_corners(c.major, c.s, c.t, N, p.i00, p.i01, p.i10, p.i11, p.tx, p.ty);
  return p;
}
// level l of frame f's cube: level 0 is the cube itself, the others lie in the pyramid behind the levels before them
template <class P> __device__ __forceinline__ P *cube_level_ptr(P *tex, P *mip, uint32_t n, uint32_t C, uint32_t tex_frames, uint32_t f, uint32_t l) {
  const size_t ft = tex_frames == 1u ? 0u : f, texels = 6u * (size_t)mip_extent(n, l) * mip_extent(n, l);
  return l == 0u ? tex + ft * texels * C : mip + ((size_t)mip_texels_before(n, n, l) * 6u * tex_frames + ft * texels) * C;
}
// what k_cube_mip and k_cube_mip_grad do alike in front of their loops: the owners, the directions of a quad with an owner, the
// faces of the sampled pixels and their levels -> `own`, `smp` and `rhd`, one bit per pixel; rhd: a sampled pixel with
// 0 <= lam < n_levels - 1, where the level has a right-hand derivative (level l0 + 1 exists)
__device__ __forceinline__ void cube_mip_quad(const CubeMipArgs &a, const PassTile &t, CubeFace (&cf)[4], MipLod (&lod)[4], uint32_t &own,
                                              uint32_t &smp, uint32_t &rhd) {
  uint32_t id[4];
  own = quad_ids(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id), smp = 0u, rhd = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) lod[k] = {0u, 0.0f};
  if (own == 0u) return;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 d[3] = {zero4, zero4, zero4};
  quad_load(a.dir + (size_t)t.f * a.dir_stride + t.poff, t.rc.plane, d, t.whole, t.x4, t.rc.tx1);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!(own & (1u << k))) continue;
    if (cube_face(quad_at(d[0], k), quad_at(d[1], k), quad_at(d[2], k), cf[k].s, cf[k].t, cf[k].inv, cf[k].major)) smp |= 1u << k;
  }
  if (a.n_levels <= 1u || smp == 0u) return;
  float4 lq[1] = {zero4}; // (words of pixels that are not sampled: loaded with their quad at most, never used)
  quad_load(a.lam + (size_t)t.f * a.lam_stride + t.poff, t.rc.plane, lq, t.whole, t.x4, t.rc.tx1);
  const float top = (float)(a.n_levels - 1u);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (smp & (1u << k)) {
      const float lam = quad_at(lq[0], k);
      lod[k] = cube_lod(lam, a.n_levels);
      if (lam >= 0.0f && lam < top) rhd |= 1u << k;
    }
}
__device__ __forceinline__ float cube_bilinear(const SRZ_CAS float *t, const CubeCorners &p, uint32_t C, uint32_t ch) {
  const float t00 = t[(size_t)p.i00 * C + ch], t01 = t[(size_t)p.i01 * C + ch], t10 = t[(size_t)p.i10 * C + ch], t11 = t[(size_t)p.i11 * C + ch];
  const float top = fmaf_(p.tx, t01 - t00, t00), bot = fmaf_(p.tx, t11 - t10, t10);
  return fmaf_(p.ty, bot - top, top);
}
__global__ __launch_bounds__(256) void k_cube_mip(CubeMipArgs a) {
  const uint32_t C = a.n_ch;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const TileRect &rc = t.rc;
    const bool fused = t.fused(a.flags_or);
    // ---- 1. owners, directions, the faces, the levels
    CubeFace cf[4] = {};
    MipLod lod[4];
    uint32_t own, smp, rhd;
    cube_mip_quad(a, t, cf, lod, own, smp, rhd);
    if (own == 0u && !fused) return;
    // ---- 2. the corners of level l0 and, where f != 0, of level l0 + 1
    CubeCorners lo[4] = {}, hi[4] = {};
    const SRZ_CAS float *p0[4], *p1[4];
    uint32_t two = 0u; // the pixels that blend two levels
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      p0[k] = p1[k] = as_const(a.tex);
      if (!(smp & (1u << k))) continue;
      const uint32_t l = lod[k].l0;
      lo[k] = cube_corners_of(cf[k], mip_extent(a.n, l));
      p0[k] = cube_level_ptr(as_const(a.tex), as_const(a.mip), a.n, C, a.tex_frames, t.f, l);
      if (lod[k].f != 0.0f) { // (l + 1 <= n_levels - 1: cube_lod gives f == 0 at the coarsest level)
        two |= 1u << k;
        hi[k] = cube_corners_of(cf[k], mip_extent(a.n, l + 1u));
        p1[k] = cube_level_ptr(as_const(a.tex), as_const(a.mip), a.n, C, a.tex_frames, t.f, l + 1u);
      }
    }
    const bool wave_two = __builtin_amdgcn_ballot_w64(two != 0u) != 0ull; // (wave-uniform: no lane blends -> no second gather)
    // ---- 3. the channels, ATTR_CHUNK at a time (k_cube's loop)
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 q[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) q[i] = make_float4(0.f, 0.f, 0.f, 0.f); // nobody, and an owner that is not sampled: zeros
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(smp & (1u << k))) continue;
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
          if (i < nc) quad_at(q[i], k) = cube_bilinear(p0[k], lo[k], C, c0 + i);
      }
      if (wave_two) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!(two & (1u << k))) continue;
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) {
              const float c = quad_at(q[i], k);
              quad_at(q[i], k) = fmaf_(lod[k].f, cube_bilinear(p1[k], hi[k], C, c0 + i) - c, c);
            }
        }
      }
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
        if (i >= nc) break;
        quad_store_owned(t.out + (size_t)(c0 + i) * rc.plane, t, {q[i]}, fused, own);
      }
    }
  });
}

// ================================================================================================================
// k_cube_mip_grad — THE BACKWARD OF k_cube_mip (srz_frameset_texture_cube_mip_grad).  k_cube_grad's walk and barriers
// (pass_walk<true>: every thread of the workgroup reaches every barrier, one outside the frame samples nothing); two phases per
// tile, each with its own channel loop:
//   A. gdir and glam, from registers, deterministic: k_cube_grad's au, av chains at level l0 and at level l0 + 1, each taken through
//      cube_gdir with its own level's face size and blended by f as the forward blends the samples; glam is the fma chain of gout
//      over c_(l0+1) - c_l0, which reads level l0 + 1 wherever 0 <= lam < n_levels - 1 — at f == 0 too (the right-hand derivative);
//   B. the texel adds, BOTH LEVELS IN ONE TABLE: TexelTable keyed on the texel's offset in the frame's concatenated pyramid
//      (cube_pyr_before(l) + its index in level l, below 2^31), the slots found once in front of the channel loop, per chunk the
//      LDS adds of (w_rc * lw) * gout, the dense flush — cube_pyr_texel finds a key's level and its place in gtex or gmip again —,
//      the keys released.  A tile where no pixel is sampled skips the phase after one barrier: the tile's threads say so in a word
//      of LDS that rotates over three words by the tile's count (k_tex_mip_grad's level word), the next one zeroed in front of the
//      barrier.  A corner without a slot adds straight to memory.
// The corners of both levels stay in registers across the phases; the slot numbers are live in B only.
// ================================================================================================================
// the texels of one frame's levels 0 .. l - 1
__device__ __forceinline__ uint32_t cube_pyr_before(uint32_t n, uint32_t l) {
  uint32_t s = 0u;
  for (uint32_t k = 0; k < l; ++k) s += 6u * mip_extent(n, k) * mip_extent(n, k);
  return s;
}
// texel `off` of frame f's concatenated pyramid in the gradient buffers: level 0 in gtex, the others in gmip
__device__ __forceinline__ float *cube_pyr_texel(const CubeMipArgs &a, uint32_t f, uint32_t off) {
  uint32_t l = 0u, sz = 6u * a.n * a.n;
  while (l + 1u < a.n_levels && off >= sz) off -= sz, ++l, sz = 6u * mip_extent(a.n, l) * mip_extent(a.n, l);
  return cube_level_ptr(a.gtex, a.gmip, a.n, a.n_ch, a.tex_frames, f, l) + (size_t)off * a.n_ch;
}
__global__ __launch_bounds__(256) void k_cube_mip_grad(CubeMipArgs a) {
  __shared__ TexelTable<CubeMipArgs, ATTR_CHUNK> tb;
  __shared__ uint32_t busy[3];
  const uint32_t tid = threadIdx.x;
  const uint32_t C = a.n_ch;
  const bool want_tex = a.gtex != nullptr, want_dir = a.out != nullptr, want_lam = a.glam != nullptr;
  if (want_tex) {
    tb.init(tid);
    if (tid < 3) busy[tid] = 0u;
    __syncthreads();
  }
  uint32_t turn = 0u; // the tile's count in this workgroup's walk mod 3 (the same in every thread: nobody skips a tile)
  pass_walk<true>(a, [&](const PassTile &t) { // (a thread outside the frame owns nothing, and still meets the barriers)
    const TileRect &rc = t.rc;
    const bool fused = t.fused(a.flags_or);
    const float *gg = a.gout + (size_t)t.f * a.gout_stride + t.poff;
    // ---- 1. owners, directions, the faces, the levels; the corners of level l0 and, where it is read, of level l0 + 1
    CubeFace cf[4] = {};
    MipLod lod[4];
    uint32_t own, smp, rhd;
    cube_mip_quad(a, t, cf, lod, own, smp, rhd);
    if (!want_lam) rhd = 0u;
    CubeCorners lo[4] = {}, hi[4] = {};
    uint32_t two = 0u, up = 0u; // the pixels that blend two levels; those whose level l0 + 1 is read (the blend, or glam)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(smp & (1u << k))) continue;
      const uint32_t l = lod[k].l0;
      lo[k] = cube_corners_of(cf[k], mip_extent(a.n, l));
      if (lod[k].f != 0.0f) two |= 1u << k;
      if (((two | rhd) >> k) & 1u) { // (l + 1 <= n_levels - 1: f != 0, or 0 <= lam < n_levels - 1)
        up |= 1u << k;
        hi[k] = cube_corners_of(cf[k], mip_extent(a.n, l + 1u));
      }
    }
    // ---- A. gdir and glam
    if ((want_dir || want_lam) && t.inside && (own != 0u || fused)) {
      const SRZ_CAS float *p0[4], *p1[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        p0[k] = p1[k] = as_const(a.tex);
        if (!(smp & (1u << k))) continue;
        p0[k] = cube_level_ptr(as_const(a.tex), as_const(a.mip), a.n, C, a.tex_frames, t.f, lod[k].l0);
        if (up & (1u << k)) p1[k] = cube_level_ptr(as_const(a.tex), as_const(a.mip), a.n, C, a.tex_frames, t.f, lod[k].l0 + 1u);
      }
      float au0[4] = {0.f, 0.f, 0.f, 0.f}, av0[4] = {0.f, 0.f, 0.f, 0.f}, au1[4] = {0.f, 0.f, 0.f, 0.f}, av1[4] = {0.f, 0.f, 0.f, 0.f};
      float gl[4] = {0.f, 0.f, 0.f, 0.f};
      for (uint32_t c0 = 0; c0 < C && smp != 0u; c0 += ATTR_CHUNK) {
        const uint32_t nc = min(ATTR_CHUNK, C - c0);
        float4 g[ATTR_CHUNK];
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
          if (i >= nc) break;
          gout_quad(gg + (size_t)(c0 + i) * rc.plane, t.whole, smp, g[i]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!(smp & (1u << k))) continue;
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) {
              const float gi = quad_at(g[i], k);
              const SRZ_CAS float *q = p0[k] + c0 + i;
              const float c_lo = bilerp_chain(q + (size_t)lo[k].i00 * C, q + (size_t)lo[k].i01 * C, q + (size_t)lo[k].i10 * C, q + (size_t)lo[k].i11 * C,
                                              lo[k].tx, lo[k].ty, gi, au0[k], av0[k]);
              if (up & (1u << k)) {
                const SRZ_CAS float *r = p1[k] + c0 + i;
                const float c_hi = bilerp_chain(r + (size_t)hi[k].i00 * C, r + (size_t)hi[k].i01 * C, r + (size_t)hi[k].i10 * C, r + (size_t)hi[k].i11 * C,
                                                hi[k].tx, hi[k].ty, gi, au1[k], av1[k]);
                if (rhd & (1u << k)) gl[k] = fmaf_(gi, c_hi - c_lo, gl[k]);
              }
            }
        }
      }
      // whole quads (fused clear, or four owners), else the owned pixels only; an owner that is not sampled: zeros
      const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (want_dir) {
        float4 gd[3] = {zero4, zero4, zero4};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (smp & (1u << k)) {
            const uint32_t l = lod[k].l0;
            float g0[3];
            cube_gdir(cf[k], au0[k], av0[k], 0.5f * (float)mip_extent(a.n, l), g0);
            if (two & (1u << k)) {
              float g1[3];
              cube_gdir(cf[k], au1[k], av1[k], 0.5f * (float)mip_extent(a.n, l + 1u), g1);
#pragma unroll
              for (int c = 0; c < 3; ++c) g0[c] = fmaf_(lod[k].f, g1[c] - g0[c], g0[c]);
            }
            quad_at(gd[0], k) = g0[0], quad_at(gd[1], k) = g0[1], quad_at(gd[2], k) = g0[2];
          }
        quad_store_owned(t.out, t, gd, fused, own);
      }
      if (want_lam) {
        float4 gq[1] = {zero4};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (rhd & (1u << k)) quad_at(gq[0], k) = gl[k];
        quad_store_owned(a.glam + (size_t)t.f * a.lam_stride + t.poff, t, gq, fused, own);
      }
    }
    if (!want_tex) return;
    // ---- B. the texel adds; a tile with nothing to add leaves after the barrier
    if (smp != 0u) atomicOr(&busy[turn], 1u);
    if (tid == 0) busy[turn == 2u ? 0u : turn + 1u] = 0u; // (last read two tiles ago, in front of the previous tile's barrier)
    __syncthreads();
    const bool any = __builtin_amdgcn_readfirstlane(busy[turn]) != 0u;
    turn = turn == 2u ? 0u : turn + 1u;
    if (!any) return;
    // ---- B1. the slots of the sampled pixels' corners at both levels (two corners on one texel: one slot, both add)
    uint32_t slot[4][8] = {};
    float *q0[4], *q1[4]; // the pixel's two levels in the gradient buffers: where a corner without a slot adds
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      q0[k] = q1[k] = a.gtex;
      if (!(smp & (1u << k))) continue;
      const uint32_t l = lod[k].l0, off0 = cube_pyr_before(a.n, l);
      q0[k] = cube_level_ptr(a.gtex, a.gmip, a.n, C, a.tex_frames, t.f, l);
      slot[k][0] = tb.slot(off0 + lo[k].i00), slot[k][1] = tb.slot(off0 + lo[k].i01);
      slot[k][2] = tb.slot(off0 + lo[k].i10), slot[k][3] = tb.slot(off0 + lo[k].i11);
      if (two & (1u << k)) {
        const uint32_t off1 = off0 + 6u * mip_extent(a.n, l) * mip_extent(a.n, l);
        q1[k] = cube_level_ptr(a.gtex, a.gmip, a.n, C, a.tex_frames, t.f, l + 1u);
        slot[k][4] = tb.slot(off1 + hi[k].i00), slot[k][5] = tb.slot(off1 + hi[k].i01);
        slot[k][6] = tb.slot(off1 + hi[k].i10), slot[k][7] = tb.slot(off1 + hi[k].i11);
      }
    }
    uint32_t n_used = 0u;
    // ---- B2. the channels, ATTR_CHUNK at a time
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 g[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (smp != 0u) {
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
          if (i >= nc) break;
          gout_quad(gg + (size_t)(c0 + i) * rc.plane, t.whole, smp, g[i]);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(smp & (1u << k))) continue;
        {
          const CornerW w = corner_weights(lo[k].tx, lo[k].ty, 1.0f - lod[k].f);
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) corner_adds(tb, slot[k], lo[k], w, quad_at(g[i], k), i, q0[k], C, c0 + i);
        }
        if (two & (1u << k)) {
          const CornerW w = corner_weights(hi[k].tx, hi[k].ty, lod[k].f);
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) corner_adds(tb, slot[k] + 4, hi[k], w, quad_at(g[i], k), i, q1[k], C, c0 + i);
        }
      }
      // ---- B3. the table's values of this chunk into memory (k_tex_grad's step 4), each key to its level again
      n_used = tb.flush(tid, c0, nc, [&a, f = t.f](uint32_t off) { return cube_pyr_texel(a, f, off); });
    }
    tb.release(tid, n_used);
  });
}

// ================================================================================================================
// k_cube_level — THE LEVEL OF A CUBE LOOKUP FROM ITS SCREEN-SPACE FOOTPRINT (srz_frameset_cube_level, include/srz.h states the rule):
// pointwise, no LDS, no barrier, k_cube's walk.  Per sampled pixel the direction's face, s, t and 1 / ma (cube_face), the derivative
// of s and t per one-pixel step in x and in y from the six derivative planes interpolate_deriv wrote for the direction — the
// quotient rule on sc / ma, tc / ma with the face held fixed —, scaled to texels of level 0 (n / 2 texels per unit of s), then
// k_tex_mip's level rule word for word (mip_lod) and lam = (float)l0 + f.
// ================================================================================================================
__global__ __launch_bounds__(256) void k_cube_level(CubeMipArgs a) {
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool fused = t.fused(a.flags_or);
    uint32_t id[4];
    const uint32_t own = quad_ids(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id);
    if (own == 0u && !fused) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 lq[1] = {zero4}; // nobody, and an owner that is not sampled: 0
    if (own != 0u) {
      float4 d[3] = {zero4, zero4, zero4}, dd[6] = {zero4, zero4, zero4, zero4, zero4, zero4};
      quad_load(a.dir + (size_t)t.f * a.dir_stride + t.poff, t.rc.plane, d, t.whole, t.x4, t.rc.tx1);
      quad_load(a.dird + (size_t)t.f * (2u * a.dir_stride) + t.poff, t.rc.plane, dd, t.whole, t.x4, t.rc.tx1);
      const float half_n = 0.5f * (float)a.n;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(own & (1u << k))) continue;
        CubeFace c;
        if (!cube_face(quad_at(d[0], k), quad_at(d[1], k), quad_at(d[2], k), c.s, c.t, c.inv, c.major)) continue;
        const uint32_t m = c.major & 3u;
        const bool pos = (c.major & 4u) != 0u;
        float ds[2], dt[2]; // d s, d t per step in x, in y
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float vx = quad_at(dd[0 + e], k), vy = quad_at(dd[2 + e], k), vz = quad_at(dd[4 + e], k);
          // the components su, sv and the major axis name, with sc's, tc's and ma's sign flips (cube_face)
          const float dsc = m == 0u ? (pos ? -vz : vz) : m == 1u ? vx : (pos ? vx : -vx);
          const float dtc = m == 1u ? (pos ? vz : -vz) : -vy;
          const float dmc = m == 0u ? vx : m == 1u ? vy : vz, dma = pos ? dmc : -dmc;
          ds[e] = (dsc - c.s * dma) * c.inv, dt[e] = (dtc - c.t * dma) * c.inv;
        }
        const MipLod r = mip_lod(ds[0], ds[1], dt[0], dt[1], half_n, half_n, a.n_levels);
        quad_at(lq[0], k) = (float)r.l0 + r.f;
      }
    }
    quad_store_owned(t.out, t, lq, fused, own);
  });
}

// ================================================================================================================
// k_shadow — A CALLER'S DEPTH MAP COMPARED AND FILTERED OVER A VISIBILITY BUFFER (srz_frameset_shadow, include/srz.h states the rule):
// percentage-closer filtering of a float map [map frame][row][column] at the coordinate planes sx, sy, sd interpolate wrote for a
// three-channel attribute: the four texels around (sx, sy) are each compared with sd — the hard test, or with width > 0 a linear ramp
// — and the four results are blended bilinearly.  k_cube's shape on the passes' helpers: pass_walk, quad_ids, the three coordinate
// words only for a quad with an owner (quad_load), quad_store_owned; 4 pixels of a row per thread; no LDS, no barrier.  bias, width
// and the map's extents are kernel arguments (wave-uniform), hard or soft ONE wave-uniform branch per corner.  The four taps of a
// pixel are two row-adjacent pairs, each pair TWO 4-BYTE LOADS: one unaligned 8-byte load would need both texels of the pair inside
// the map, and at x0 = -1 and x1 = map_w only one of them is — the pair would need the very per-texel branch it was to save.
// Every float -> int conversion follows the float clamp to [-1, map_w] (and [-1, map_h]); a corner is read (and, in the backward,
// added to) only behind the unsigned compare of its own coordinates with the map's extents: no value of the planes leaves the map.
// shadow_px (a sampled pixel's fractions, corner values and moving corners) is the rule's text; k_shadow and k_shadow_grad both go
// through it, so the backward differentiates the very words the forward computed.
// ================================================================================================================
struct ShadowPx {
  float v[4];      // the corners' values v00, v01, v10, v11 (corner r * 2 + c is texel (y0 + r, x0 + c)); outside the map: 1
  float tx, ty;
  int base;        // y0 * map_w + x0 with x0 in [-1, map_w], y0 in [-1, map_h]: corner (r, c) is texel base + r * map_w + c, IF inside
  uint32_t moving; // bit r * 2 + c: the corner lies inside the map and on the ramp (0 < r < 1): its texel and sd move the sample
  bool in_x, in_y; // the coordinate lies strictly inside (-1, map_w) / (-1, map_h) (else its derivative is 0)
};
// one axis of the rule: coordinate s in texel units over n texels (centres on the integers) -> the first texel coordinate, in
// [-1, n], the fraction, and whether s moves the sample
__device__ __forceinline__ void shadow_axis(float s, uint32_t n, int &i0, float &t, bool &in) {
  const float nf = (float)n;
  in = s > -1.0f && s < nf;
  const float fx = __builtin_fminf(__builtin_fmaxf(s, -1.0f), nf);
  const float f0 = __builtin_floorf(fx);
  t = fx - f0;
  i0 = (int)f0;
}
// the pixel at (sx, sy, sd) of map `map`; false: not sampled (a coordinate not finite)
__device__ __forceinline__ bool shadow_px(const ShadowArgs &a, const SRZ_CAS float *map, float sx, float sy, float sd, ShadowPx &p) {
  if (!tex_finite(sx) || !tex_finite(sy) || !tex_finite(sd)) return false;
  const int W = (int)a.map_w, H = (int)a.map_h;
  int x0, y0;
  shadow_axis(sx, a.map_w, x0, p.tx, p.in_x);
  shadow_axis(sy, a.map_h, y0, p.ty, p.in_y);
  p.base = y0 * W + x0;
  p.moving = 0u;
  const bool soft = a.width > 0.0f;
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float v = 1.0f;
      if ((unsigned)(x0 + c) < (unsigned)W && (unsigned)(y0 + r) < (unsigned)H) {
        const float e = (map[p.base + r * W + c] + a.bias) - sd;
        if (soft) {
          const float q = e / a.width + 0.5f;
          v = __builtin_fminf(__builtin_fmaxf(q, 0.0f), 1.0f); // (NaN -> 0)
          if (q > 0.0f && q < 1.0f) p.moving |= 1u << (r * 2 + c);
        } else {
          v = e >= 0.0f ? 1.0f : 0.0f;
        }
      }
      p.v[r * 2 + c] = v;
    }
  return true;
}
// what k_shadow and k_shadow_grad do alike: the owners, the coordinates of a quad with an owner, the sampled pixels -> `own` and
// `smp`, one bit per pixel
__device__ __forceinline__ void shadow_quad(const ShadowArgs &a, const PassTile &t, ShadowPx (&px)[4], uint32_t &own, uint32_t &smp) {
  uint32_t id[4];
  own = quad_ids(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id), smp = 0u;
  if (own == 0u) return;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 s[3] = {zero4, zero4, zero4};
  quad_load(a.sc + (size_t)t.f * a.sc_stride + t.poff, t.rc.plane, s, t.whole, t.x4, t.rc.tx1);
  const SRZ_CAS float *map = as_const(a.map) + (size_t)t.f * a.map_frame_stride;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!(own & (1u << k))) continue;
    if (shadow_px(a, map, quad_at(s[0], k), quad_at(s[1], k), quad_at(s[2], k), px[k])) smp |= 1u << k;
  }
}
__global__ __launch_bounds__(256) void k_shadow(ShadowArgs a) {
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const bool fused = t.fused(a.flags_or);
    ShadowPx px[4];
    uint32_t own, smp;
    shadow_quad(a, t, px, own, smp);
    if (own == 0u && !fused) return;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f); // nobody: zeros (stored with the fused clear only)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(own & (1u << k))) continue;
      float r = 1.0f; // an owner that is not sampled: no occluder known, lit
      if (smp & (1u << k)) {
        const ShadowPx &p = px[k];
        const float top = fmaf_(p.tx, p.v[1] - p.v[0], p.v[0]), bot = fmaf_(p.tx, p.v[3] - p.v[2], p.v[2]);
        r = fmaf_(p.ty, bot - top, top);
      }
      quad_at(o, k) = r;
    }
    quad_store_owned(t.out, t, {o}, fused, own);
  });
}

// ================================================================================================================
// k_shadow_grad — THE BACKWARD OF k_shadow (srz_frameset_shadow_grad): gout -> the gradient planes of sx, sy, sd (gsc: per pixel,
// from registers, deterministic) and, WANT_MAP, the map's gradient: per MOVING corner one add (w[corner] * gout) / width into gmap.
// The planes-only build has no LDS, no shuffle and no barrier (k_light_grad<false>'s precedent): a call that does not ask for gmap
// pays for no table.  The WANT_MAP build is k_tex_grad's structure at one channel on the passes' helpers (pass_walk<true>: every
// thread of the workgroup reaches every barrier, one outside the frame samples nothing): the tile's open-addressed table of distinct
// texels in LDS (TexelTable with ONE value per slot, 24 KB, not ATTR_CHUNK — 48 KB would halve the workgroups a CU holds — keyed
// on y * map_w + x), the slots of the moving corners found first, LDS float adds, the dense flush with global_atomic_add_f32, a
// corner without a slot adding straight to memory.  A tile without a moving corner (every tile of a hard call; the lit and the
// fully shadowed tiles of a soft one) skips the table behind one __syncthreads_or, as k_light_grad does.
// ================================================================================================================
template <bool WANT_MAP> __device__ __forceinline__ void shadow_grad_body(const ShadowArgs &a, TexelTable<ShadowArgs, 1u> *tb) {
  const uint32_t tid = threadIdx.x;
  const bool want_sc = a.out != nullptr;
  if (WANT_MAP) { // (its own text, one loop: with TexelTable::init the kernel has 7 601 instructions, so 7 575)
    for (uint32_t i = tid; i < TG_SLOTS; i += 256) tb->key[i] = 0u, tb->val[i] = 0.0f;
    if (tid == 0) tb->n_used = 0u;
    __syncthreads();
  }
  pass_walk<WANT_MAP>(a, [&](const PassTile &t) { // (WANT_MAP: a thread outside the frame owns nothing, and still meets the barriers)
    const bool fused = t.fused(a.flags_or);
    // ---- 1. owners, coordinates, the sampled pixels; gout of a quad with a sampled pixel
    ShadowPx px[4];
    uint32_t own, smp;
    shadow_quad(a, t, px, own, smp);
    if (!WANT_MAP && own == 0u && !fused) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 g[1] = {zero4};
    if (smp != 0u) quad_load(a.gout + (size_t)t.f * a.gout_stride + t.poff, t.rc.plane, g, t.whole, t.x4, t.rc.tx1);
    // ---- 2. per sampled pixel: gsx, gsy from the corner values, the moving corners' terms d_rc and gsd = -(their sum)
    float4 gs[3] = {zero4, zero4, zero4};
    float d[4][4];
    uint32_t mov = 0u; // the thread's moving corners, bit k * 4 + corner
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[k][0] = d[k][1] = d[k][2] = d[k][3] = 0.0f;
      if (!(smp & (1u << k))) continue;
      const ShadowPx &p = px[k];
      const float gk = quad_at(g[0], k);
      const float top = fmaf_(p.tx, p.v[1] - p.v[0], p.v[0]), bot = fmaf_(p.tx, p.v[3] - p.v[2], p.v[2]);
      quad_at(gs[0], k) = p.in_x ? gk * fmaf_(p.ty, (p.v[3] - p.v[2]) - (p.v[1] - p.v[0]), p.v[1] - p.v[0]) : 0.0f;
      quad_at(gs[1], k) = p.in_y ? gk * (bot - top) : 0.0f;
      const float w[4] = {(1.0f - p.tx) * (1.0f - p.ty), p.tx * (1.0f - p.ty), (1.0f - p.tx) * p.ty, p.tx * p.ty};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (p.moving & (1u << c)) d[k][c] = (w[c] * gk) / a.width; // (moving: width > 0)
      quad_at(gs[2], k) = -(((d[k][0] + d[k][1]) + d[k][2]) + d[k][3]);
      mov |= p.moving << (4 * k);
    }
    if (want_sc && t.inside && (own != 0u || fused)) quad_store_owned(t.out, t, gs, fused, own);
    if (WANT_MAP) {
      // ---- 3. the tile's moving corners through the table into gmap; a tile without one is done
      if (!__syncthreads_or(mov != 0u)) return;
      float *gmap = a.gmap + (size_t)t.f * a.map_frame_stride;
      const int W = (int)a.map_w;
      uint32_t slot[4][4] = {};
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (mov & (1u << (4 * k + c))) slot[k][c] = tb->slot((uint32_t)(px[k].base + (c >> 1) * W + (c & 1)));
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (mov & (1u << (4 * k + c)))
            tb->add(slot[k][c], 0u, d[k][c], gmap, (uint32_t)(px[k].base + (c >> 1) * W + (c & 1)), 1u, 0u);
      // ---- 4. the table's values into memory, texel after texel, and the tile's keys go in the same loop (its own text: with
      // TexelTable::flush and release the kernel has 7 591 instructions, so 7 575, and measured 1.5 % slower, NOTEBOOK.md)
      __syncthreads();
      const uint32_t n_used = tb->n_used;
      for (uint32_t i = tid; i < n_used; i += 256) {
        const uint32_t s = tb->used[i];
        const float v = tb->val[s];
        global_add(gmap + (tb->key[s] - 1u), v);
        tb->val[s] = 0.0f, tb->key[s] = 0u;
      }
      __syncthreads();
      if (tid == 0) tb->n_used = 0u;
      __syncthreads();
    }
  });
}
template <bool WANT_MAP> __global__ __launch_bounds__(256) void k_shadow_grad(ShadowArgs a) {
  if constexpr (WANT_MAP) {
    __shared__ TexelTable<ShadowArgs, 1u> tb;
    shadow_grad_body<true>(a, &tb);
  } else {
    shadow_grad_body<false>(a, nullptr);
  }
}

// ================================================================================================================
// k_resolve8 — display()'s resolve (src/Render.cpp:61-62): cv::merge(planes 0,1,2) + convertTo(CV_8UC3) =
// saturate_cast<uchar>(cvRound(v)): round half to even, clamp to [0,255]; NaN → 0.  4 pixels per thread: three 16-byte
// plane reads → 12 output bytes (three dword stores).
// ================================================================================================================
__device__ __forceinline__ uint32_t to_u8(float v) {
  if (!(v == v)) return 0u;
  const float r = __builtin_rintf(v); // round half to even (default rounding mode)
  return r <= 0.0f ? 0u : (r >= 255.0f ? 255u : (uint32_t)r);
}
__global__ __launch_bounds__(256) void k_resolve8(const float *planes, uint8_t *out, uint32_t n_frames, uint32_t rows, uint32_t W,
                                                  uint64_t frame_stride) {
  const uint64_t quads_per_frame = (uint64_t)rows * W / 4; // W % 4 == 0 is required by the launcher
  const uint64_t total = quads_per_frame * n_frames;
  for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < total; q += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t f = q / quads_per_frame, i = (q - f * quads_per_frame) * 4;
    const float *p = planes + f * frame_stride + (uint64_t)rows * W; // plane 1 = c0 (plane 0 is z)
    const SRZ_CAS f32x4 *c0 = reinterpret_cast<const SRZ_CAS f32x4 *>(as_const(p + i));
    const SRZ_CAS f32x4 *c1 = reinterpret_cast<const SRZ_CAS f32x4 *>(as_const(p + (uint64_t)rows * W + i));
    const SRZ_CAS f32x4 *c2 = reinterpret_cast<const SRZ_CAS f32x4 *>(as_const(p + 2ull * rows * W + i));
    const f32x4 a = *c0, b = *c1, c = *c2;
    const uint32_t b0 = to_u8(a.x), g0 = to_u8(b.x), r0 = to_u8(c.x), b1 = to_u8(a.y), g1 = to_u8(b.y), r1 = to_u8(c.y);
    const uint32_t b2 = to_u8(a.z), g2 = to_u8(b.z), r2 = to_u8(c.z), b3 = to_u8(a.w), g3 = to_u8(b.w), r3 = to_u8(c.w);
    uint32_t *o = reinterpret_cast<uint32_t *>(out + (f * (uint64_t)rows * W + i) * 3);
    o[0] = b0 | (g0 << 8) | (r0 << 16) | (b1 << 24);
    o[1] = g1 | (r1 << 8) | (b2 << 16) | (g2 << 24);
    o[2] = r2 | (b3 << 8) | (g3 << 16) | (r3 << 24);
  }
}
// Frames whose plane size rows * W is not a multiple of 4 pixels (odd sizes: the planes behind the first are not 16-byte
// aligned and the 12-byte output groups would straddle frames): one pixel per thread, dword loads, byte stores — rare sizes,
// same result
__global__ __launch_bounds__(256) void k_resolve8_px(const float *planes, uint8_t *out, uint32_t n_frames, uint32_t rows, uint32_t W,
                                                     uint64_t frame_stride) {
  const uint64_t px_per_frame = (uint64_t)rows * W, total = px_per_frame * n_frames;
  for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < total; q += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t f = q / px_per_frame, i = q - f * px_per_frame;
    const SRZ_CAS float *p = as_const(planes + f * frame_stride + px_per_frame + i);
    uint8_t *o = out + q * 3;
    o[0] = (uint8_t)to_u8(p[0]), o[1] = (uint8_t)to_u8(p[px_per_frame]), o[2] = (uint8_t)to_u8(p[2 * px_per_frame]);
  }
}
void launch_resolve8(const float *planes, uint8_t *out, uint32_t n_frames, uint32_t rows, uint32_t W, uint64_t frame_stride,
                     hipStream_t s) {
  const uint64_t px = (uint64_t)n_frames * rows * W;
  if (!px) return;
  // the 4-pixel kernel walks a frame's plane as one flat run: it needs rows * W % 4 == 0 (then every plane and every frame starts
  // on a 16-byte boundary of a 16-byte aligned buffer, and every 12-byte output group on a 4-byte one) — not W % 4 == 0
  if ((((uint64_t)rows * W) & 3u) == 0 && ((uintptr_t)planes & 15u) == 0 && ((uintptr_t)out & 3u) == 0) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((px / 4 + 255) / 256, 8192);
    hipLaunchKernelGGL(k_resolve8, dim3(grid), dim3(256), 0, s, planes, out, n_frames, rows, W, frame_stride);
  } else {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((px + 255) / 256, 8192);
    hipLaunchKernelGGL(k_resolve8_px, dim3(grid), dim3(256), 0, s, planes, out, n_frames, rows, W, frame_stride);
  }
}

// ================================================================================================================
// k_deinterleave — the multi-GPU exchange's second half.  The all-gather leaves every rank's shard one after the other,
//   gathered[rank][frame][plane][local band][32 rows][row bytes]        (band b = band_of(local band, rank): srz_device.h),
// and this kernel restores the reference's row-major planes,
//   full[frame][plane][band][32 rows][row bytes],
// in one pass of 16-byte (or 4-byte) units: consecutive threads copy consecutive units of one destination row.
// ================================================================================================================
template <typename U>
__global__ __launch_bounds__(256) void k_deinterleave(const U *gathered, U *full, uint32_t world, uint32_t n_fp /* frames x planes */,
                                                      uint32_t bands_per_rank, uint32_t band_units_ /* units per 32-row band */) {
  const uint64_t band_units = band_units_, total = (uint64_t)n_fp * bands_per_rank * world * band_units;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t in_band = i % band_units, b = i / band_units; // b = (frame-plane, local band, rank) of the destination
    const uint64_t fp = b / ((uint64_t)world * bands_per_rank);
    const uint32_t bb = (uint32_t)(b % ((uint64_t)world * bands_per_rank)); // the band inside its frame-plane
    const uint32_t rank = (uint32_t)rank_of_band((int)bb, (int)world), lb = bb / world;
    full[i] = __builtin_nontemporal_load(gathered + (((uint64_t)rank * n_fp + fp) * bands_per_rank + lb) * band_units + in_band);
  }
}
void launch_deinterleave(const void *gathered, void *full, uint32_t world, uint32_t n_fp, uint32_t bands_per_rank, uint32_t row_bytes,
                         hipStream_t s) {
  // unit of the copy: what a BAND (32 rows) of row_bytes and both buffers are aligned to — 16, 4 or (8-bit images of a width that is
  // not a multiple of 4) 1 byte
  const uint32_t band_bytes = (uint32_t)BAND * row_bytes;
  const uintptr_t al = (uintptr_t)gathered | (uintptr_t)full;
  const uint32_t unit = ((band_bytes & 15u) == 0 && (al & 15u) == 0) ? 16u : ((band_bytes & 3u) == 0 && (al & 3u) == 0) ? 4u : 1u;
  const uint32_t band_units = band_bytes / unit; // (k_deinterleave's row_units x BAND: it only ever uses the product)
  const uint64_t total = (uint64_t)n_fp * bands_per_rank * world * band_units;
  if (!total) return;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((total + 255) / 256, 16384);
  if (unit == 16u)
    hipLaunchKernelGGL(k_deinterleave<u32x4>, dim3(grid), dim3(256), 0, s, (const u32x4 *)gathered, (u32x4 *)full, world, n_fp, bands_per_rank, band_units);
  else if (unit == 4u)
    hipLaunchKernelGGL(k_deinterleave<uint32_t>, dim3(grid), dim3(256), 0, s, (const uint32_t *)gathered, (uint32_t *)full, world, n_fp, bands_per_rank,
                       band_units);
  else
    hipLaunchKernelGGL(k_deinterleave<uint8_t>, dim3(grid), dim3(256), 0, s, (const uint8_t *)gathered, (uint8_t *)full, world, n_fp, bands_per_rank,
                       band_units);
}

// ================================================================================================================
// The tile-sparse exchange (srz_frameset_sparse_*; message format in include/srz.h).  A rank sends only the 32x32 tiles its
// render drew into; every other tile of its shard holds the clear values bit for bit, and the receivers write those themselves.
//   k_sparse_count  one wave per (frame, local band): touched tiles of the band
//   k_sparse_scan   one workgroup: exclusive scan of those counts = every band's first slot; the message header
//   k_sparse_pack   one workgroup per tile: its table entry (band's first slot + touched tiles left of it: a count, no atomics —
//                   two packs of one render give the same bytes) and, if touched, the tile's planes into its payload slot
//   k_sparse_unpack every peer's shard from its message: payload tiles copied, the others written with the clear values
// Units U (16, 4 or 1 bytes) never straddle a tile column or a row end: the launchers pick the largest one the row bytes and the
// buffers' alignment allow (16-B rows of float planes of any W % 4 == 0 width; 8-bit rows of W % 16 == 0).
// ================================================================================================================
// "touched" = k_clear's test for a tile it does NOT clear, copied: k_clear is tuned and stays as it is, and
// tests/test_sparse_exchange.py pins the two texts to each other.  A frame whose render was not a fused clear keeps the caller's
// old contents in the tiles no bbox reached: every tile of it counts as touched.
__device__ __forceinline__ bool sparse_touched(const SparseArgs &a, uint32_t f, uint32_t lb, uint32_t tx) {
  if (lb >= a.n_local_bands) return false; // (a padding band of this shard: no rows behind it)
  const SRZ_CAS FrameDesc *fd = as_const(a.frames) + f;
  if (!((fd->flags | a.flags_or) & SRZ_FUSED_CLEAR)) return true;
  const SRZ_CAS u32x2 *cnt = as_const(reinterpret_cast<const u32x2 *>(a.tile_info)) + ((size_t)f * a.n_local_bands + lb) * a.tiles_x;
  return cnt[tx].x != 0u;
}
template <typename U> __device__ __forceinline__ U sparse_clear(bool z) {
  const uint32_t v = z ? 0x7f800000u : 0u; // (z = +inf, colour 0; the 8-bit image's clear is 0, and it is the only plane of byte units)
  if constexpr (std::is_same<U, u32x4>::value) return U{v, v, v, v};
  else if constexpr (std::is_same<U, uint32_t>::value) return v;
  else return (U)0;
}
__global__ __launch_bounds__(256) void k_sparse_count(SparseArgs a) {
  const uint32_t lane = threadIdx.x & 63u, r = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (r >= a.n_frames * a.bands_per_rank) return; // (whole waves)
  const uint32_t f = r / a.bands_per_rank, lb = r % a.bands_per_rank;
  uint32_t n = 0;
  for (uint32_t x0 = 0; x0 < a.tiles_x; x0 += 64u)
    n += (uint32_t)__builtin_popcountll(__ballot(x0 + lane < a.tiles_x && sparse_touched(a, f, lb, x0 + lane)));
  if (lane == 0) a.row_cnt[r] = n;
}
__global__ __launch_bounds__(1024) void k_sparse_scan(SparseArgs a) {
  __shared__ uint32_t s_w[16];
  const uint32_t n_rows = a.n_frames * a.bands_per_rank, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  uint32_t carry = 0;
  for (uint32_t r0 = 0; r0 < n_rows; r0 += 1024u) {
    const uint32_t r = r0 + t, v = r < n_rows ? a.row_cnt[r] : 0u, incl = wave_scan_add(v);
    if (lane == 63u) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = carry, total = 0;
    for (uint32_t w = 0; w < 16u; ++w) before += w < wave ? s_w[w] : 0u, total += s_w[w];
    if (r < n_rows) a.row_cnt[r] = before + incl - v;
    carry += total;
    __syncthreads(); // (s_w is rewritten by the next chunk)
  }
  uint32_t *h = reinterpret_cast<uint32_t *>(a.msg);
  for (uint64_t w = 4u + (uint64_t)n_rows * a.tiles_x + t; w < a.payload_off / 4u; w += 1024u) h[w] = 0u; // (the table's padding: 0)
  if (t == 0) {
    const uint64_t tile_bytes = (uint64_t)a.planes * BAND * TILE * a.px_bytes;
    h[0] = carry, h[1] = n_rows * a.tiles_x;
    *reinterpret_cast<uint64_t *>(h + 2) = a.payload_off + (uint64_t)carry * tile_bytes;
  }
}
template <typename U>
__global__ __launch_bounds__(256) void k_sparse_pack(SparseArgs a) {
  const uint32_t i = blockIdx.x, tx = i % a.tiles_x, r = i / a.tiles_x;
  const uint32_t f = r / a.bands_per_rank, lb = r % a.bands_per_rank;
  uint32_t before = 0; // touched tiles left of this one in its band
  for (uint32_t x0 = 0; x0 < tx; x0 += 256u) before += (uint32_t)__syncthreads_count(x0 + threadIdx.x < tx && sparse_touched(a, f, lb, x0 + threadIdx.x));
  const bool mine = sparse_touched(a, f, lb, tx);
  const uint32_t slot = a.row_cnt[r] + before;
  if (threadIdx.x == 0) reinterpret_cast<uint32_t *>(a.msg + SPARSE_HEADER)[i] = mine ? slot : SPARSE_NONE;
  if (!mine) return;
  const uint32_t band = (uint32_t)band_of((int)lb, (int)a.rank, (int)a.world), rows = min((uint32_t)BAND, a.height - band * BAND);
  const uint32_t tru = TILE * a.px_bytes / (uint32_t)sizeof(U), row_units = a.row_bytes / (uint32_t)sizeof(U);
  const uint32_t x_units = tx * tru, cols = min(tru, row_units - x_units); // units of the tile's rows that are pixels of the frame
  const U *src = reinterpret_cast<const U *>(a.shard) + ((size_t)f * a.planes * a.local_rows + (size_t)lb * BAND) * row_units + x_units;
  const uint32_t per_plane = BAND * tru, n = a.planes * per_plane;
  U *dst = reinterpret_cast<U *>(a.msg + a.payload_off) + (size_t)slot * n;
  for (uint32_t k0 = threadIdx.x; k0 < n; k0 += 4u * 256u) { // [plane][32 rows][tile row]: coalesced stores, four loads in flight
    U v[4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
      const uint32_t k = k0 + j * 256u, pl = k / per_plane, rem = k - pl * per_plane, ly = rem / tru, u = rem - ly * tru;
      v[j] = (k < n && ly < rows && u < cols) ? src[((size_t)pl * a.local_rows + ly) * row_units + u] : sparse_clear<U>(false); // (edge padding: 0)
    }
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j)
      if (k0 + j * 256u < n) dst[k0 + j * 256u] = v[j];
  }
}
// One work item = one plane of one local band of one frame of one peer, written ROW-MAJOR like k_clear: a thread takes one unit
// column of the band and stores it in every row of the band (32 stores in flight), so runs of clear tiles and copied tiles alike
// become long contiguous bursts of the destination.  It writes only pixels: rows that exist, x < W.
template <typename U>
__global__ __launch_bounds__(256) void k_sparse_unpack(SparseArgs a, const uint8_t *recv, uint64_t stride, U *gathered) {
  const uint32_t P = a.planes, bpr = a.bands_per_rank, n_items = (a.world - 1u) * a.n_frames * bpr * P;
  const uint32_t n_bands = (a.height + BAND - 1) / BAND;
  const uint32_t tru = TILE * a.px_bytes / (uint32_t)sizeof(U), row_units = a.row_bytes / (uint32_t)sizeof(U), per_plane = BAND * tru;
  const uint64_t shard_units = (uint64_t)a.n_frames * P * a.local_rows * row_units;
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) { // it = ((q * n_frames + f) * bpr + lb) * P + pl
    const uint32_t pl = it % P, lb = (it / P) % bpr, f = (it / (P * bpr)) % a.n_frames, q = it / (P * bpr * a.n_frames);
    const uint32_t p = q + (q >= a.rank ? 1u : 0u); // (the peers: every rank but this one)
    const uint32_t band = (uint32_t)band_of((int)lb, (int)p, (int)a.world);
    if (band >= n_bands) continue;
    const uint32_t rows = min((uint32_t)BAND, a.height - band * BAND);
    const uint8_t *m = recv + (uint64_t)p * stride;
    const SRZ_CAS uint32_t *table = as_const(reinterpret_cast<const uint32_t *>(m + SPARSE_HEADER)) + ((size_t)f * bpr + lb) * a.tiles_x;
    const U *payload = reinterpret_cast<const U *>(m + a.payload_off) + (size_t)pl * per_plane;
    U *dst = gathered + p * shard_units + ((size_t)(f * P + pl) * a.local_rows + (size_t)lb * BAND) * row_units;
    const U clear = sparse_clear<U>(P == 4u && pl == 0u);
    for (uint32_t u = threadIdx.x; u < row_units; u += blockDim.x) {
      const uint32_t tx = u / tru, slot = table[tx];
      if (slot == SPARSE_NONE) {
        for (uint32_t ly = 0; ly < rows; ++ly) __builtin_nontemporal_store(clear, dst + (size_t)ly * row_units + u);
      } else {
        const U *src = payload + (size_t)slot * P * per_plane + (u - tx * tru);
        uint32_t ly = 0;
        for (; ly + 8u <= rows; ly += 8u) { // (eight loads in flight before the stores that depend on them)
          U v[8];
#pragma unroll
          for (uint32_t j = 0; j < 8u; ++j) v[j] = __builtin_nontemporal_load(src + (ly + j) * tru);
#pragma unroll
          for (uint32_t j = 0; j < 8u; ++j) __builtin_nontemporal_store(v[j], dst + (size_t)(ly + j) * row_units + u);
        }
        for (; ly < rows; ++ly) __builtin_nontemporal_store(__builtin_nontemporal_load(src + ly * tru), dst + (size_t)ly * row_units + u);
      }
    }
  }
}
namespace {
uint32_t sparse_unit(uint32_t row_bytes, uintptr_t al) {
  return ((row_bytes & 15u) == 0 && (al & 15u) == 0) ? 16u : ((row_bytes & 3u) == 0 && (al & 3u) == 0) ? 4u : 1u;
}
} // namespace
void launch_sparse_pack(const SparseArgs &a, hipStream_t s) {
  const uint32_t n_rows = a.n_frames * a.bands_per_rank, n_tab = n_rows * a.tiles_x;
  if (n_rows) hipLaunchKernelGGL(k_sparse_count, dim3((n_rows + 3) / 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_sparse_scan, dim3(1), dim3(1024), 0, s, a); // (also the header of an empty set)
  if (!n_tab) return;
  const uint32_t unit = sparse_unit(a.row_bytes, (uintptr_t)a.shard | (uintptr_t)a.msg);
  if (unit == 16u) hipLaunchKernelGGL(k_sparse_pack<u32x4>, dim3(n_tab), dim3(256), 0, s, a);
  else if (unit == 4u) hipLaunchKernelGGL(k_sparse_pack<uint32_t>, dim3(n_tab), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_sparse_pack<uint8_t>, dim3(n_tab), dim3(256), 0, s, a);
}
void launch_sparse_unpack(const SparseArgs &a, const void *recv, uint64_t msg_stride, void *gathered, hipStream_t s) {
  const uint32_t n_items = (a.world - 1u) * a.n_frames * a.bands_per_rank * a.planes;
  if (!n_items) return;
  const uint32_t grid = std::min(n_items, SPARSE_UNPACK_WGS);
  const uint32_t unit = sparse_unit(a.row_bytes, (uintptr_t)recv | (uintptr_t)gathered | (uintptr_t)msg_stride);
  const uint8_t *m = static_cast<const uint8_t *>(recv);
  if (unit == 16u) hipLaunchKernelGGL(k_sparse_unpack<u32x4>, dim3(grid), dim3(256), 0, s, a, m, msg_stride, static_cast<u32x4 *>(gathered));
  else if (unit == 4u) hipLaunchKernelGGL(k_sparse_unpack<uint32_t>, dim3(grid), dim3(256), 0, s, a, m, msg_stride, static_cast<uint32_t *>(gathered));
  else hipLaunchKernelGGL(k_sparse_unpack<uint8_t>, dim3(grid), dim3(256), 0, s, a, m, msg_stride, static_cast<uint8_t *>(gathered));
}

// Exhaustive check of the short exact sequences above against the IEEE expansions: all 2^32 bit patterns.
// out[0] = operands tested on the fast path, out[1..3] = mismatches of rcp_rn / sqrt_rn / rsqrt2_rn (must be 0).
__global__ void k_verify_fastmath(unsigned long long *out) {
  unsigned long long bad0 = 0, bad1 = 0, bad2 = 0, n = 0;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < (1ull << 32); i += (uint64_t)gridDim.x * blockDim.x) {
    const float x = __builtin_bit_cast(float, (uint32_t)i);
    const float a = rcp_rn(x), ra = 1.0f / x;
    bad0 += f2u_(a) != f2u_(ra);
    const float b = sqrt_rn(x), rb = __builtin_sqrtf(x);
    bad1 += f2u_(b) != f2u_(rb);
    const float c = rsqrt2_rn(x), rc = 1.0f / rb;
    bad2 += f2u_(c) != f2u_(rc);
    n += fast_range(x);
  }
  if (n) atomicAdd(&out[0], n);
  if (bad0) atomicAdd(&out[1], bad0);
  if (bad1) atomicAdd(&out[2], bad1);
  if (bad2) atomicAdd(&out[3], bad2);
}
void launch_verify_fastmath(unsigned long long *d_out, hipStream_t s) {
  hipLaunchKernelGGL(k_verify_fastmath, dim3(8192), dim3(256), 0, s, d_out);
}

// Companion check of div_by_rcp against the IEEE division: out[0] = pairs tested, out[1] = mismatches on pseudo-random
// (a, b) inside the documented ranges (uniform exponents, random mantissas, plus few-significant-bit operands whose
// quotients are exact or near-exact), out[2] = mismatches of texel / 255 over all 256 texels (must both be 0).
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull, z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull, z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__global__ void k_verify_fastdiv(unsigned long long *out, uint32_t per_thread) {
  unsigned long long bad = 0, bad255 = 0, n = 0;
  uint64_t st = mix64(blockIdx.x * (uint64_t)blockDim.x + threadIdx.x);
  for (uint32_t i = 0; i < per_thread; ++i) {
    st = mix64(st);
    uint32_t ua = (uint32_t)st, ub = (uint32_t)(st >> 32);
    const uint32_t ea = 67u + ((ua >> 23) & 0xffu) % 121u, eb = 87u + ((ub >> 23) & 0xffu) % 81u;
    if (i & 1u) ua &= ~0x7ff000u, ub &= ~0x7fff00u; // few significant bits
    ua = (ua & 0x807fffffu) | (ea << 23), ub = (ub & 0x007fffffu) | (eb << 23);
    const float a = __builtin_bit_cast(float, ua), b = __builtin_bit_cast(float, ub);
    bad += !(div_num_ok(a) && div_den_ok(b)) || f2u_(div_by_rcp(a, b, rcp_core(b))) != f2u_(a / b);
    ++n;
  }
  if (blockIdx.x == 0) {
    FastMath fm;
    const float t = (float)threadIdx.x;
    bad255 += f2u_(fm.div255(t)) != f2u_(t / 255.0f);
    float q0, q1, q2;
    fm.div3(0.0f, t, 1.0f, 255.0f, q0, q1, q2); // +0 numerator stays +0
    bad255 += f2u_(q0) != 0u || f2u_(q1) != f2u_(t / 255.0f) || fm.bad;
  }
  atomicAdd(&out[0], n);
  if (bad) atomicAdd(&out[1], bad);
  if (bad255) atomicAdd(&out[2], bad255);
}
void launch_verify_fastdiv(unsigned long long *d_out, hipStream_t s) {
  hipLaunchKernelGGL(k_verify_fastdiv, dim3(8192), dim3(256), 0, s, d_out, 2048u);
}

// Check of len2d_fast (two binary64 Heron steps from the binary32 root) against len2d_f64 (the compiler's correctly rounded binary64
// square root) on pseudo-random pairs: out[0] = pairs, out[1] = results that differ although the flag was clear (must be 0),
// out[2] = flagged pairs among the random ones (must stay rare), out[3] = among the Pythagorean ones, out[4] = among the
// few-significant-bit ones (exact roots and exact ties are common there).  A quarter of
// the pairs each: random mantissas with independent exponents 2^-30 .. 2^40; the same with exponents at most two apart (both
// squares matter); few significant bits (exact and near-exact roots); scaled Pythagorean pairs (m^2 - n^2, 2 m n) whose root
// m^2 + n^2 is an odd number of up to 25 bits — exactly ON a binary32 rounding boundary when it exceeds 2^24 (those must be flagged
// or equal: the reference's tie goes to even).
__global__ void k_verify_fastlen(unsigned long long *out, uint32_t per_thread) {
  unsigned long long bad = 0, flagged = 0, flagged_p = 0, flagged_f = 0, n = 0;
  uint64_t st = mix64(0x5eedull + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x);
  for (uint32_t i = 0; i < per_thread; ++i) {
    st = mix64(st);
    uint32_t ua = (uint32_t)st, ub = (uint32_t)(st >> 32);
    const uint32_t mode = i & 3u;
    float a, b;
    if (mode == 3u) {
      const uint32_t m = 2u + (ua >> 8) % 4094u;           // 2 .. 4095
      uint32_t k = 1u + (ub >> 8) % (m - 1u);              // 1 .. m - 1
      if (((m ^ k) & 1u) == 0u) k = k > 1u ? k - 1u : 2u;  // opposite parity (m = 2: k = 1)
      if (k >= m) k = m - 1u;
      const int e = (int)(ua & 31u) - 16;
      a = __builtin_ldexpf((float)(m * m - k * k), e), b = __builtin_ldexpf((float)(2u * m * k), e); // (both exact)
      if (ub & 1u) a = -a;
    } else {
      const uint32_t ea = 97u + ((ua >> 23) & 0xffu) % 71u;
      uint32_t eb = 97u + ((ub >> 23) & 0xffu) % 71u;
      if (mode == 1u) eb = ea + ((ub >> 23) & 3u) - 1u;
      if (mode == 2u) ua &= ~0x3fffu << ((ub >> 28) & 7u), ub &= ~0xfffu << ((ua >> 28) & 7u);
      a = u2f_((ua & 0x807fffffu) | (ea << 23)), b = u2f_((ub & 0x807fffffu) | (eb << 23));
    }
    bool amb = false;
    uint32_t sb;
    const float x = len2d_fast(a, b, amb, sb), y = len2d_f64(a, b);
    ++n, bad += (!amb && f2u_(x) != f2u_(y)) ? 1 : 0;
    if (amb) (mode == 3u ? flagged_p : mode == 2u ? flagged_f : flagged) += 1;
  }
  atomicAdd(&out[0], n);
  if (bad) atomicAdd(&out[1], bad);
  if (flagged) atomicAdd(&out[2], flagged);
  if (flagged_p) atomicAdd(&out[3], flagged_p);
  if (flagged_f) atomicAdd(&out[4], flagged_f);
}
void launch_verify_fastlen(unsigned long long *d_out4, hipStream_t s) {
  hipLaunchKernelGGL(k_verify_fastlen, dim3(8192), dim3(256), 0, s, d_out4, 2048u);
}

// Exhaustive check of pow_fast against pow_cr: every binary32 x in [2^-40, 1] (+ the operands above 1 the clamped cosines can
// reach by rounding) at exponent p.  out[0] = operands, out[1] = results that differ although pow_fast did NOT flag them (must
// be 0), out[2] = flagged operands whose result is a normal binary32 >= 2^-120 (ambiguous roundings: must stay rare), out[3] =
// flagged operands with smaller results (the band 2^-151 .. 2^-120 is flagged wholesale; cosines that small are rare).
__global__ void k_verify_fastpow(unsigned long long *out, float p) {
  unsigned long long bad = 0, flagged = 0, flagged_small = 0, n = 0;
  const uint32_t lo = 0x2b800000u /* 2^-40 */, hi = 0x3f800010u /* 1 + 16 ulp */;
  for (uint64_t i = lo + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i <= hi; i += (uint64_t)gridDim.x * blockDim.x) {
    const float x = __builtin_bit_cast(float, (uint32_t)i);
    bool amb = false;
    const float a = pow_fast(x, p, amb), b = pow_cr(x, p);
    ++n, bad += (!amb && f2u_(a) != f2u_(b)) ? 1 : 0;
    if (amb) (b >= 0x1p-120f ? flagged : flagged_small) += 1;
  }
  if (blockIdx.x == 0 && threadIdx.x < 4) { // the special operands: ±0 give +0 unflagged; negative, inf and NaN must be flagged
    const float sp[4] = {0.0f, -0.0f, -1.0f, __builtin_inff()};
    bool amb = false;
    const float a = pow_fast(sp[threadIdx.x], p, amb);
    bad += threadIdx.x < 2 ? (amb || f2u_(a) != 0u) : !amb;
  }
  atomicAdd(&out[0], n);
  if (bad) atomicAdd(&out[1], bad);
  if (flagged) atomicAdd(&out[2], flagged);
  if (flagged_small) atomicAdd(&out[3], flagged_small);
}
void launch_verify_fastpow(unsigned long long *d_out3, float p, hipStream_t s) {
  hipLaunchKernelGGL(k_verify_fastpow, dim3(8192), dim3(256), 0, s, d_out3, p);
}

// BGR u8 (row_stride bytes per row) → one dword per texel
__global__ void k_tex_convert(const uint8_t *bgr, int w, int h, int row_stride, uint32_t *out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w * h) return;
  int y = i / w, x = i - y * w;
  const uint8_t *p = bgr + (size_t)y * row_stride + (size_t)x * 3;
  out[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// ---- launchers ---------------------------------------------------------------------------------------------------
void launch_vertex(const DrawDesc *draws, uint32_t n_draws, uint32_t max_faces, srz_tri *tris, float *tri_pos, const FrameDesc *frames,
                   BBox *bbox_out, hipStream_t s) {
  if (n_draws == 0 || max_faces == 0) return;
  dim3 grid((max_faces + 255) / 256, n_draws);
  if (grid.x > 1024) grid.x = 1024;
  hipLaunchKernelGGL(k_vertex, grid, dim3(256), 0, s, draws, tris, tri_pos, frames, bbox_out);
}

void launch_positions(const FrameDesc *frames, uint32_t n_frames, const float *tri_pos, uint32_t pos_stride, float *out, uint32_t pos_tris,
                      hipStream_t s) {
  if (n_frames == 0 || pos_tris == 0) return;
  const size_t blocks = ((size_t)pos_tris * TRI_POS_F + 255) / 256;
  dim3 grid((uint32_t)(blocks > 1024 ? 1024 : blocks), n_frames);
  hipLaunchKernelGGL(k_positions, grid, dim3(256), 0, s, frames, tri_pos, pos_stride, out, pos_tris);
}

void launch_vertex_grad(const VertexGradArgs &a, hipStream_t s) {
  if (a.n_frames == 0 || a.n_verts == 0) return;
  hipLaunchKernelGGL(k_vertex_grad, dim3((a.n_verts + 255) / 256, a.n_frames), dim3(256), 0, s, a);
}

void launch_mesh_normals(const MeshNormalsArgs &a, hipStream_t s) {
  if (a.n_sets == 0 || a.n_verts == 0) return;
  hipLaunchKernelGGL(k_mesh_normals, dim3((a.n_verts + 255) / 256, a.n_sets), dim3(256), 0, s, a);
}

void launch_mesh_normals_grad(const MeshNormalsArgs &a, hipStream_t s) {
  if (a.n_sets == 0 || a.n_verts == 0) return;
  const dim3 grid((a.n_verts + 255) / 256, a.n_sets);
  hipLaunchKernelGGL(k_mesh_normals_grad<1>, grid, dim3(256), 0, s, a); // (stream order: every gS is stored before phase 2 reads one)
  hipLaunchKernelGGL(k_mesh_normals_grad<2>, grid, dim3(256), 0, s, a);
}

void launch_mesh_tangents(const MeshTangentsArgs &a, hipStream_t s) {
  if (a.n_sets == 0 || a.n_verts == 0) return;
  hipLaunchKernelGGL(k_mesh_tangents, dim3((a.n_verts + 255) / 256, a.n_sets), dim3(256), 0, s, a);
}

void launch_mesh_laplacian(const MeshLaplacianArgs &a, int kind, bool transpose, hipStream_t s) {
  if (a.n_verts == 0u) return;
  const dim3 grid((a.n_verts + 255) / 256, a.n_sets, (a.n_ch + LAP_CHUNK - 1) / LAP_CHUNK);
  if (kind == SRZ_LAP_COTAN) hipLaunchKernelGGL(k_mesh_laplacian<SRZ_LAP_COTAN>, grid, dim3(256), 0, s, a);
  else if (kind == SRZ_LAP_GRAPH) hipLaunchKernelGGL(k_mesh_laplacian<SRZ_LAP_GRAPH>, grid, dim3(256), 0, s, a);
  else if (transpose) hipLaunchKernelGGL(k_mesh_laplacian<LAP_UMBRELLA_T>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_mesh_laplacian<SRZ_LAP_UMBRELLA>, grid, dim3(256), 0, s, a);
}

void launch_mesh_edges(const MeshEdgesArgs &a, int kind, hipStream_t s) {
  if (a.n_faces == 0u) return;
  const dim3 grid((a.n_faces + 255) / 256, a.n_sets);
  if (kind == SRZ_EDGE_COUNT) hipLaunchKernelGGL(k_mesh_edges<SRZ_EDGE_COUNT>, grid, dim3(256), 0, s, a);
  else if (kind == SRZ_EDGE_LENGTH) hipLaunchKernelGGL(k_mesh_edges<SRZ_EDGE_LENGTH>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_mesh_edges<SRZ_EDGE_DIHEDRAL>, grid, dim3(256), 0, s, a);
}

void launch_mesh_edges_grad(const MeshEdgesArgs &a, int kind, hipStream_t s) {
  if (a.n_verts == 0u) return;
  const dim3 verts((a.n_verts + 255) / 256, a.n_sets), faces((a.n_faces + 255) / 256, a.n_sets);
  if (kind == SRZ_EDGE_LENGTH) {
    hipLaunchKernelGGL(k_mesh_edges_grad<0>, verts, dim3(256), 0, s, a);
    return;
  }
  // (a slot with no faces: every corner list is empty, phase 2 alone writes the zeros)
  if (a.n_faces != 0u) hipLaunchKernelGGL(k_mesh_edges_grad<1>, faces, dim3(256), 0, s, a); // (stream order, as launch_mesh_normals_grad)
  hipLaunchKernelGGL(k_mesh_edges_grad<2>, verts, dim3(256), 0, s, a);
}

void launch_mesh_tangents_grad(const MeshTangentsArgs &a, hipStream_t s) {
  if (a.n_sets == 0 || a.n_verts == 0) return;
  const dim3 grid((a.n_verts + 255) / 256, a.n_sets);
  hipLaunchKernelGGL(k_mesh_tangents_grad<1>, grid, dim3(256), 0, s, a); // (stream order, as launch_mesh_normals_grad)
  hipLaunchKernelGGL(k_mesh_tangents_grad<2>, grid, dim3(256), 0, s, a);
}

// (n_verts * n_ch <= 2^32 * 64: at most 2^30 blocks)
static dim3 corner_attr_grid(const CornerAttrArgs &a) { return dim3((uint32_t)(((uint64_t)a.n_verts * a.n_ch + 255) / 256), a.n_frames); }
void launch_corner_attr(const CornerAttrArgs &a, hipStream_t s) {
  if (a.n_frames == 0 || a.n_verts == 0) return;
  hipLaunchKernelGGL(k_corner_attr, corner_attr_grid(a), dim3(256), 0, s, a);
}

void launch_corner_attr_grad(const CornerAttrArgs &a, hipStream_t s) {
  if (a.n_frames == 0 || a.n_verts == 0) return;
  hipLaunchKernelGGL(k_corner_attr_grad, corner_attr_grid(a), dim3(256), 0, s, a);
}

void launch_chunks(const RenderArgs &a, int n_frames, uint32_t max_tris, hipStream_t s) {
  if (n_frames <= 0 || max_tris == 0) return;
  dim3 grid((max_tris + GROUP_TRIS - 1u) / GROUP_TRIS, n_frames); // one workgroup pass per group
  if (grid.x > 4096) grid.x = 4096;
  hipLaunchKernelGGL(k_chunks, grid, dim3(256), 0, s, a);
}

void launch_setup(const RenderArgs &a, int n_frames, uint32_t max_tris, bool stats, hipStream_t s) {
  if (n_frames <= 0 || max_tris == 0) return;
  dim3 grid((max_tris + GROUP_TRIS - 1u) / GROUP_TRIS, n_frames); // one workgroup pass per group
  if (grid.x > 4096) grid.x = 4096;
  BBox *bb = const_cast<BBox *>(a.bbox);
  if (stats)
    hipLaunchKernelGGL(k_setup<true>, grid, dim3(256), 0, s, a, bb);
  else
    hipLaunchKernelGGL(k_setup<false>, grid, dim3(256), 0, s, a, bb);
}

void launch_bin(const RenderArgs &a, int n_frames, uint32_t max_tris, hipStream_t s) {
  if (n_frames <= 0 || a.n_local_bands == 0) return;
  const uint32_t groups = ((uint32_t)n_frames + 7u) / 8u;
  // (measured: 4 waves best at 5.9 k triangles, 8 at 94 k; a job with fewer band workgroups than CUs is pure latency: 8)
  const int waves = (max_tris <= 32768u && (uint32_t)n_frames * a.n_local_bands > 256u) ? 4 : BIN_MAX_WAVES;
  const size_t lds = sizeof(uint32_t) * (3u * (size_t)a.tiles_x + 64u * waves + 4u + BIN_STAGE + 2u + 128u * waves * bin_keep((uint32_t)waves));
  hipLaunchKernelGGL(k_bin, dim3(groups * 8u * a.n_local_bands), dim3(64 * waves), lds, s, a);
}

// End of a measurement render (one thread; srz_device.h, ClearCtl): file the sample, move to the next grid or decide.
__global__ void k_clear_tune(ClearCtl *c, uint32_t *h_wgs) {
  const unsigned long long now = __builtin_amdgcn_s_memrealtime();
  if (c->done) return;
  if (c->pos > 0 && c->n[c->cur] < 4u) c->t[c->cur][c->n[c->cur]++] = (float)(now - c->last);
  c->last = now;
  if (++c->pos < (uint32_t)CLEAR_TUNE_BLOCK) return;
  c->pos = 0; // a block has ended
  int next = -1;
  if (c->phase == 0u) {
    // A larger grid that is already more than 5 % behind the best smaller one ends the first pass: the step is the clear, and the grids
    // beyond it would only be worse (config 2: 96 / 128 / 256 workgroups take 0.78 / 0.83 / 1.04 ms) — they are not tried.
    bool worse = false;
    if (c->cur > 0u) {
      float best = 3.0e38f;
      for (uint32_t i = 0; i < c->cur; ++i) best = fminf(best, 0.5f * (c->t[i][0] + c->t[i][1]));
      worse = 0.5f * (c->t[c->cur][0] + c->t[c->cur][1]) > 1.05f * best;
    }
    const int tried = (int)c->cur + 1;
    if (tried < CLEAR_CANDS && !worse) next = tried;
    else { // the first pass is over: who stays?
      // Dropped: a grid that was tried AFTER the best one and is still more than 5 % behind it.  (The first renders after idle, or into
      // buffers touched for the first time, run slower: the first pass favours the later grids, so an earlier one that looks worse
      // stays in, and the mirrored pass settles it.)
      float m[CLEAR_CANDS];
      int ib = 0;
      for (int i = 0; i < tried; ++i) {
        m[i] = 0.5f * (c->t[i][0] + c->t[i][1]);
        if (m[i] < m[ib]) ib = i;
      }
      for (int i = tried; i < CLEAR_CANDS; ++i) m[i] = 0.f;
      uint32_t alive = 0;
      for (int i = 0; i < tried; ++i)
        if (i <= ib || m[i] <= 1.05f * m[ib]) alive |= 1u << i;
      c->alive = alive, c->phase = 1u;
      for (int i = 0; i < CLEAR_CANDS; ++i) c->score[i] = (alive >> i & 1u) ? m[i] : 0.f;
      if (__popc(alive) > 1) next = 31 - __clz((int)alive); // (the mirrored pass starts with the grid in use)
    }
  } else {
    const uint32_t lower = c->alive & ((1u << c->cur) - 1u);
    if (lower) next = 31 - __clz((int)lower);
    else // the mirrored pass is over: medians of four
      for (int i = 0; i < CLEAR_CANDS; ++i)
        if (c->alive >> i & 1u) {
          float *t = c->t[i];
          for (int x = 1; x < 4; ++x)
            for (int y = x; y > 0 && t[y] < t[y - 1]; --y) { const float u = t[y]; t[y] = t[y - 1], t[y - 1] = u; }
          c->score[i] = 0.5f * (t[1] + t[2]);
        }
  }
  if (next >= 0) {
    c->cur = (uint32_t)next, c->wgs = CLEAR_CAND[next];
    return;
  }
  int arg = -1;
  for (int i = 0; i < CLEAR_CANDS; ++i)
    if ((c->alive >> i & 1u) && (arg < 0 || c->score[i] < c->score[arg])) arg = i;
  c->wgs = CLEAR_CAND[arg < 0 ? 0 : arg], c->done = 1u;
  __hip_atomic_store(h_wgs, c->wgs, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); // (mapped host memory: the host launches that grid from now on)
}

void launch_clear_tune(ClearCtl *ctl, uint32_t *h_wgs, hipStream_t s) { hipLaunchKernelGGL(k_clear_tune, dim3(1), dim3(1), 0, s, ctl, h_wgs); }

// End of a render that files no sample (srz_frameset_render_visibility) while the set measures: the next sample starts here, so that
// it times the next colour render alone
__global__ void k_clear_rebase(ClearCtl *c) {
  if (!c->done) c->last = __builtin_amdgcn_s_memrealtime();
}
void launch_clear_rebase(ClearCtl *ctl, hipStream_t s) { hipLaunchKernelGGL(k_clear_rebase, dim3(1), dim3(1), 0, s, ctl); }

void launch_clear(const RenderArgs &a, uint32_t max_tiles, hipStream_t s, uint32_t wgs) {
  if (max_tiles == 0) return;
  // Beside k_raster/k_shade the clear is THROTTLED by its grid size, so that the stores spread over the whole pipeline instead of starving
  // the rasteriser's loads and the shader's register file.  The best grid depends on what runs beside it (config 2: 96 workgroups, 0.738
  // of the roofline against 0.727 at 80 and 0.681 at 128; config 4: 0.406 at 96, 0.438 at 256), so it is measured per set (srz_device.h,
  // ClearCtl: while that goes on the grid is CLEAR_GRID_MAX and a.clear_wgs_dev says how many of it work).  Work items are planes of bands.
  const uint32_t n_items = a.n_frames * a.n_local_bands * 4u;
  const uint32_t cap = wgs ? wgs : 96u;
  // (round 6, same box: the clear's stores as nt / sc1 nt / sc0 sc1 nt / sc1 / plain give config 4 3.10 / 3.22 / 3.26 / 3.29 / 3.29 ms per
  // step and config 5 5.25 / 5.48 / 5.44 / 5.71 / 5.62: nt, as round 3 found on config 2)
  hipLaunchKernelGGL(k_clear, dim3(n_items < cap ? n_items : cap), dim3(256), 0, s, a);
}

// The grid of a kernel that strides over `items` tiles: at most `cap` workgroups, a multiple of 8 (workgroup b serves the frames f ≡ b mod 8)
static uint32_t tile_grid(uint32_t items, uint32_t cap = 16384u) { return (std::min(items, cap) + 7u) & ~7u; }

// One stream: a LARGE grid (a tile or two per workgroup: in-order hand-out, one-tile tail).  Renders interleaved on several streams
// (a.other_streams): a grid about as large as the machine's resident capacity, the workgroups striding through the lists — measured,
// 2 x 128 frames of 1024^2 on two streams: 16384 workgroups 1.10 ms per batch, 4096 1.08, 2560 1.07, 1280 1.065 (and on ONE stream
// 0.73 / 0.78 / — / 0.78 ms for k_shade alone).  A multiple of 8: workgroup b serves list b % 8.
static dim3 shade_grid(const RenderArgs &a, uint32_t max_tiles) { return dim3(tile_grid(max_tiles, a.other_streams ? 2048u : 16384u)); }

// One launch per FAST build kind of `kinds`, in ascending kind order: launch(FASTNL, BUMPY, APPROX) gets each as std::integral_constants.
// The tolerance mode (approx) has builds for kinds 0..3 only: classify_frames sends it no frame of another FAST kind.
template <int FASTNL, bool BUMPY, class L> static void launch_kind(uint32_t kinds, bool approx, L &launch) {
  if (!((kinds >> build_kind<FASTNL, BUMPY>()) & 1u)) return;
  if constexpr (FASTNL > 0 && !BUMPY)
    if (approx) return launch(std::integral_constant<int, FASTNL>{}, std::false_type{}, std::true_type{});
  launch(std::integral_constant<int, FASTNL>{}, std::bool_constant<BUMPY>{}, std::false_type{});
}
template <class L> static void launch_fast_kinds(uint32_t kinds, bool approx, L &&launch) {
  launch_kind<1, false>(kinds, approx, launch), launch_kind<2, false>(kinds, approx, launch);
  launch_kind<3, false>(kinds, approx, launch), launch_kind<4, false>(kinds, approx, launch);
  launch_kind<1, true>(kinds, approx, launch), launch_kind<2, true>(kinds, approx, launch);
  launch_kind<3, true>(kinds, approx, launch), launch_kind<4, true>(kinds, approx, launch);
  launch_kind<-1, false>(kinds, approx, launch), launch_kind<-2, false>(kinds, approx, launch);
  launch_kind<-3, false>(kinds, approx, launch), launch_kind<-4, false>(kinds, approx, launch);
}

void launch_shade(const RenderArgs &a, uint32_t max_tiles, bool stats, uint32_t kinds, bool any_generic, bool approx, hipStream_t s) {
  if (max_tiles == 0) return;
  const dim3 grid = shade_grid(a, max_tiles);
  if (stats) { // (counting runs shade every frame with the generic build: force_generic)
    hipLaunchKernelGGL((k_shade<true, 0>), grid, dim3(256), 0, s, a);
    return;
  }
  launch_fast_kinds(kinds, approx, [&](auto nl, auto bumpy, auto ap) {
    hipLaunchKernelGGL((k_shade<false, decltype(nl)::value, decltype(bumpy)::value, decltype(ap)::value>), grid, dim3(256), 0, s, a);
  });
  // the generic build also serves the tiles the FAST builds hand back: when no frame is generic that is normally
  // nothing, and a small grid does
  dim3 ggrid(any_generic ? grid.x : (grid.x < 128u ? grid.x : 128u));
  hipLaunchKernelGGL((k_shade<false, 0>), ggrid, dim3(256), 0, s, a);
}

void launch_visibility(const RenderArgs &a, uint32_t max_tiles, hipStream_t s) {
  if (max_tiles == 0) return;
  hipLaunchKernelGGL(k_visibility, shade_grid(a, max_tiles), dim3(256), 0, s, a);
}

void launch_shade_vis(const ShadeVisArgs &a, uint32_t kinds, bool any_generic, bool approx, hipStream_t s) {
  const uint32_t items = a.n_frames * a.n_local_bands * a.tiles_x;
  if (items == 0) return;
  const dim3 grid(tile_grid(items)), blk(256);
  launch_fast_kinds(kinds, approx, [&](auto nl, auto bumpy, auto ap) {
    hipLaunchKernelGGL((k_shade_vis<decltype(nl)::value, decltype(bumpy)::value, decltype(ap)::value>), grid, blk, 0, s, a);
  });
  // the generic build also serves the tiles the exact FAST builds hand back (redo_count: zeroed by the caller)
  if (any_generic || (kinds && !approx)) hipLaunchKernelGGL((k_shade_vis<0>), any_generic ? grid : dim3(std::min(grid.x, 128u)), blk, 0, s, a);
}

// the passes over a visibility buffer that are one kernel each: one workgroup of 256 per tile_grid() entry, nothing for an empty set
template <auto Kernel, class Args> static void launch_pass(const Args &a, hipStream_t s) {
  const uint32_t items = a.n_frames * a.n_local_bands * a.tiles_x;
  if (items != 0) hipLaunchKernelGGL(Kernel, dim3(tile_grid(items)), dim3(256), 0, s, a);
}
void launch_gbuffer(const GbufArgs &a, hipStream_t s) { launch_pass<k_gbuffer>(a, s); }
void launch_motion(const MotionArgs &a, hipStream_t s) { launch_pass<k_motion>(a, s); }
void launch_interp(const InterpArgs &a, hipStream_t s) { launch_pass<k_interp>(a, s); }
void launch_interp_grad(const InterpArgs &a, hipStream_t s) { launch_pass<k_interp_grad>(a, s); }
void launch_pos_grad(const PosGradArgs &a, hipStream_t s) { launch_pass<k_pos_grad>(a, s); }
void launch_antialias(const AntialiasArgs &a, hipStream_t s) { launch_pass<k_antialias>(a, s); }
void launch_antialias_grad(const AntialiasArgs &a, hipStream_t s) { launch_pass<k_antialias_grad>(a, s); }
void launch_tex(const TexArgs &a, hipStream_t s) { launch_pass<k_tex>(a, s); }
void launch_tex_grad(const TexArgs &a, hipStream_t s) { launch_pass<k_tex_grad>(a, s); }
void launch_cube(const CubeArgs &a, hipStream_t s) { launch_pass<k_cube>(a, s); }
void launch_cube_grad(const CubeArgs &a, hipStream_t s) { launch_pass<k_cube_grad>(a, s); }
void launch_light(const LightArgs &a, hipStream_t s) { launch_pass<k_light>(a, s); }
// with a.work: the tiles' partial sums, then k_light_fold over each frame's tiles — into gpar's rows, or (one parameter frame for
// every frame) into the rows behind the partials and from there, frame after frame, into gpar.  Not launch_pass for the fold: its
// grid is the rows it writes, not the set's tiles.  A shard without bands has no tiles and launches no k_light_grad; the folds run all
// the same — a sum of no partials is +0 — so every row of gpar is WRITTEN there too
void launch_light_grad(const LightArgs &a, float *gpar, hipStream_t s) {
  if (!gpar) return launch_pass<k_light_grad<false>>(a, s);
  const uint32_t tpf = a.n_local_bands * a.tiles_x, K = SRZ_LIGHT_PAR(a.n_lights);
  const bool shared = a.par_stride == 0u;
  launch_pass<k_light_grad<true>>(a, s);
  float *rows = shared ? a.work + (size_t)a.n_frames * tpf * K : gpar;
  if (a.n_frames != 0u) hipLaunchKernelGGL(k_light_fold, dim3(a.n_frames), dim3(64), 0, s, (const float *)a.work, rows, tpf, K);
  if (shared) hipLaunchKernelGGL(k_light_fold, dim3(1), dim3(64), 0, s, (const float *)rows, gpar, a.n_frames, K);
}
// (launch_light_grad's two steps over rows of 9, k_light_fold unchanged; ray_stride == 0: one ray block for every frame)
void launch_background(const BgArgs &a, hipStream_t s) { launch_pass<k_background>(a, s); }
void launch_background_grad(const BgArgs &a, float *gray, hipStream_t s) {
  if (!gray) return launch_pass<k_background_grad<false>>(a, s);
  const uint32_t tpf = a.n_local_bands * a.tiles_x, K = 9u;
  const bool shared = a.ray_stride == 0u;
  launch_pass<k_background_grad<true>>(a, s);
  float *rows = shared ? a.work + (size_t)a.n_frames * tpf * K : gray;
  if (a.n_frames != 0u) hipLaunchKernelGGL(k_light_fold, dim3(a.n_frames), dim3(64), 0, s, (const float *)a.work, rows, tpf, K);
  if (shared) hipLaunchKernelGGL(k_light_fold, dim3(1), dim3(64), 0, s, (const float *)rows, gray, a.n_frames, K);
}
void launch_microfacet(const MicrofacetArgs &a, hipStream_t s) { launch_pass<k_microfacet>(a, s); }
// (launch_light_grad's two steps, k_light_fold unchanged: K = SRZ_MICROFACET_PAR(n_lights) <= 54 of its 64 threads)
void launch_microfacet_grad(const MicrofacetArgs &a, float *gpar, hipStream_t s) {
  if (!gpar) return launch_pass<k_microfacet_grad<false>>(a, s);
  const uint32_t tpf = a.n_local_bands * a.tiles_x, K = SRZ_MICROFACET_PAR(a.n_lights);
  const bool shared = a.par_stride == 0u;
  launch_pass<k_microfacet_grad<true>>(a, s);
  float *rows = shared ? a.work + (size_t)a.n_frames * tpf * K : gpar;
  if (a.n_frames != 0u) hipLaunchKernelGGL(k_light_fold, dim3(a.n_frames), dim3(64), 0, s, (const float *)a.work, rows, tpf, K);
  if (shared) hipLaunchKernelGGL(k_light_fold, dim3(1), dim3(64), 0, s, (const float *)rows, gpar, a.n_frames, K);
}
void launch_reflect(const ReflectArgs &a, hipStream_t s) { launch_pass<k_reflect>(a, s); }
void launch_reflect_grad(const ReflectArgs &a, hipStream_t s) { launch_pass<k_reflect_grad>(a, s); }
void launch_brdf_table(float *tab, uint32_t n, uint32_t m, hipStream_t s) { hipLaunchKernelGGL(k_brdf_table, dim3(n * n), dim3(64), 0, s, tab, n, m); }
void launch_ibl(const IblArgs &a, hipStream_t s) { launch_pass<k_ibl>(a, s); }
// (with gtab: a grid of at most 1024 workgroups, so that each clears and flushes its LDS table once for several tiles)
void launch_ibl_grad(const IblArgs &a, hipStream_t s) {
  if (!a.gtab) return launch_pass<k_ibl_grad<false>>(a, s);
  const uint32_t items = a.n_frames * a.n_local_bands * a.tiles_x;
  if (items != 0) hipLaunchKernelGGL(k_ibl_grad<true>, dim3(tile_grid(items, 1024u)), dim3(256), 0, s, a);
}
void launch_normal_map(const NormalMapArgs &a, hipStream_t s) { launch_pass<k_normal_map>(a, s); }
void launch_normal_map_grad(const NormalMapArgs &a, hipStream_t s) { launch_pass<k_normal_map_grad>(a, s); }
void launch_shadow(const ShadowArgs &a, hipStream_t s) { launch_pass<k_shadow>(a, s); }
// (without gmap: the build that has no table)
void launch_shadow_grad(const ShadowArgs &a, hipStream_t s) {
  if (a.gmap) launch_pass<k_shadow_grad<true>>(a, s);
  else launch_pass<k_shadow_grad<false>>(a, s);
}
void launch_interp_deriv(const InterpDerivArgs &a, hipStream_t s) { launch_pass<k_interp_deriv>(a, s); }
void launch_persp(const PerspArgs &a, hipStream_t s) { launch_pass<k_persp>(a, s); }
void launch_persp_grad(const PerspArgs &a, hipStream_t s) { launch_pass<k_persp_grad>(a, s); }
void launch_interp_deriv_persp(const PerspDerivArgs &a, hipStream_t s) { launch_pass<k_interp_deriv_persp>(a, s); }
void launch_tex_mip(const TexMipArgs &a, hipStream_t s) { launch_pass<k_tex_mip>(a, s); }
void launch_tex_mip_grad(const TexMipArgs &a, hipStream_t s) { launch_pass<k_tex_mip_grad>(a, s); }
void launch_cube_mip(const CubeMipArgs &a, hipStream_t s) { launch_pass<k_cube_mip>(a, s); }
void launch_cube_mip_grad(const CubeMipArgs &a, hipStream_t s) { launch_pass<k_cube_mip_grad>(a, s); }
void launch_cube_level(const CubeMipArgs &a, hipStream_t s) { launch_pass<k_cube_level>(a, s); }
// a workgroup per row of the level written (build) or of level 0 (fold), at most MIP_GRID of them striding over the rows
constexpr uint32_t MIP_GRID = 8192;
void launch_mip_build(const float *src, float *dst, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h, uint32_t n_ch,
                      uint32_t tex_frames, hipStream_t s) {
  const uint32_t n_rows = tex_frames * dst_h;
  hipLaunchKernelGGL(k_mip_build, dim3(std::min(n_rows, MIP_GRID)), dim3(256), 0, s, src, dst, src_w, src_h, dst_w, dst_h, n_ch, n_rows);
}
void launch_mip_fold(const float *gmip, float *gtex, uint32_t tex_w, uint32_t tex_h, uint32_t n_ch, uint32_t tex_frames, uint32_t n_levels,
                     hipStream_t s) {
  hipLaunchKernelGGL(k_mip_fold, dim3(std::min(tex_frames * tex_h, MIP_GRID)), dim3(256), 0, s, gmip, gtex, tex_w, tex_h, n_ch, tex_frames, n_levels);
}
// the table, (backward) q, the pieces' walks, (a walk cut into rows) the rows' fold, the fold: five launches at the most, in stream order
template <bool BWD> static void launch_prefilter_impl(const PrefilterArgs &p, hipStream_t s) {
  const uint32_t n_own = BWD ? p.n_src : p.n_dst, n_walk = BWD ? p.n_dst : p.n_src;
  const uint32_t own_texels = (uint32_t)prefilter_texels(n_own), walk_texels = (uint32_t)prefilter_texels(n_walk);
  const float r = p.roughness < 0.0625f ? 0.0625f : p.roughness, al = r * r;
  PfWalk a{};
  a.tab = (const PfTexel *)p.work;
  char *after = (char *)p.work + prefilter_table_bytes(n_walk);
  a.val = p.src;
  hipLaunchKernelGGL(k_prefilter_table, dim3((walk_texels + 255u) / 256u), dim3(256), 0, s, (PfTexel *)p.work, n_walk);
  if (BWD) {
    const size_t n_q = (size_t)walk_texels * p.n_ch * p.frames;
    hipLaunchKernelGGL(k_prefilter_q, dim3((uint32_t)((n_q + 255u) / 256u)), dim3(256), 0, s, p.src, p.den, (float *)after, walk_texels, p.n_ch, p.frames);
    a.val = (const float *)after;
    after += prefilter_q_bytes(p.n_dst, p.n_ch, p.frames);
  }
  a.part = (float *)after;
  a.n_own = n_own, a.n_walk = n_walk, a.C = p.n_ch, a.CS = p.n_ch + (BWD ? 0u : 1u), a.frames = p.frames;
  a.chunks = prefilter_chunks(n_own, n_walk, p.n_ch, p.frames), a.kind = p.kind;
  a.a2m1 = al * al - 1.0f, a.cmin = p.cmin;
  const uint32_t fg = p.frames * prefilter_groups(p.n_ch);
  hipLaunchKernelGGL(k_prefilter<BWD>, dim3((own_texels + 255u) / 256u, a.chunks, std::min(fg, 65535u)), dim3(256), 0, s, a);
  const size_t n_fold = (size_t)own_texels * p.frames;
  if (a.chunks > 6u) { // rows into faces first, behind the rows' partial sums
    float *faces = a.part + (size_t)a.chunks * n_fold * a.CS;
    hipLaunchKernelGGL(k_prefilter_rows, dim3((uint32_t)((6u * n_fold * a.CS + 255u) / 256u)), dim3(256), 0, s, a, faces);
    a.part = faces, a.chunks = 6u;
  }
  hipLaunchKernelGGL(k_prefilter_fold<BWD>, dim3((uint32_t)((n_fold + 255u) / 256u)), dim3(256), 0, s, a, p.dst, p.den_out);
}
void launch_prefilter(const PrefilterArgs &a, hipStream_t s) { launch_prefilter_impl<false>(a, s); }
void launch_prefilter_grad(const PrefilterArgs &a, hipStream_t s) { launch_prefilter_impl<true>(a, s); }
// the rows' partials, k_light_fold twice (a face's rows, a frame's faces: K = 9 n_ch + 1 of its 64 threads), the division
constexpr uint32_t CUBE_SH_GRID = 65536;
void launch_cube_sh(const CubeShArgs &a, hipStream_t s) {
  const uint32_t K = cube_sh_slots(a.n_ch);
  const uint64_t rows = (uint64_t)a.frames * 6u * a.n;
  float *faces = a.work + (size_t)rows * K, *cube = faces + (size_t)a.frames * 6u * K;
  hipLaunchKernelGGL(k_cube_sh, dim3((uint32_t)std::min<uint64_t>((rows + 3u) / 4u, CUBE_SH_GRID)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_light_fold, dim3(a.frames * 6u), dim3(64), 0, s, (const float *)a.work, faces, a.n, K);
  hipLaunchKernelGGL(k_light_fold, dim3(a.frames), dim3(64), 0, s, (const float *)faces, cube, 6u, K);
  const uint32_t count = a.frames * 9u * a.n_ch;
  hipLaunchKernelGGL(k_cube_sh_finish, dim3((count + 255u) / 256u), dim3(256), 0, s, (const float *)cube, a.dst, a.den_out, a.n_ch, a.frames);
}
void launch_cube_sh_grad(const CubeShArgs &a, hipStream_t s) {
  const uint32_t count = a.frames * 9u * a.n_ch;
  const uint64_t blocks = (uint64_t)a.frames * ((6u * a.n * a.n + 255u) / 256u);
  hipLaunchKernelGGL(k_cube_sh_q, dim3((count + 255u) / 256u), dim3(256), 0, s, a.src, a.den, a.work, count);
  hipLaunchKernelGGL(k_cube_sh_grad, dim3((uint32_t)std::min<uint64_t>(blocks, 1u << 20)), dim3(256), 0, s, a);
}
void launch_sh(const ShArgs &a, hipStream_t s) { launch_pass<k_sh>(a, s); }
// (launch_light_grad's two steps over rows of 9 n_ch, k_light_fold unchanged; sh_stride == 0: one set of coefficients for every frame)
void launch_sh_grad(const ShArgs &a, float *gsh, hipStream_t s) {
  if (!gsh) return launch_pass<k_sh_grad<false>>(a, s);
  const uint32_t tpf = a.n_local_bands * a.tiles_x, K = 9u * a.n_ch;
  const bool shared = a.sh_stride == 0u;
  launch_pass<k_sh_grad<true>>(a, s);
  float *rows = shared ? a.work + (size_t)a.n_frames * tpf * K : gsh;
  if (a.n_frames != 0u) hipLaunchKernelGGL(k_light_fold, dim3(a.n_frames), dim3(64), 0, s, (const float *)a.work, rows, tpf, K);
  if (shared) hipLaunchKernelGGL(k_light_fold, dim3(1), dim3(64), 0, s, (const float *)rows, gsh, a.n_frames, K);
}

bool raster_four_waves(const RenderArgs &a) { return a.n_frames * a.n_local_bands * a.tiles_x <= 4096u; }

void launch_raster(const RenderArgs &a, int n_frames, bool stats, hipStream_t s) {
  if (n_frames <= 0 || a.n_local_bands == 0) return;
  const uint32_t groups = ((uint32_t)n_frames + 7u) / 8u;
  const uint32_t tiles = groups * 8u * a.n_local_bands * a.tiles_x;
  // batches: one wave per tile; a few frames: four waves per tile (the frame is as slow as its heaviest tile)
  if (!raster_four_waves(a))
    hipLaunchKernelGGL(k_raster<1>, dim3(tiles), dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL(k_raster<4>, dim3(tiles), dim3(256), 0, s, a);
  // the ordered rasteriser for whatever k_raster listed (normally nothing: its waves read a zero and leave)
  // (a large grid whenever the ordered rasteriser is known to get every touched tile: counting runs, SRZ_ORDERED_RASTER on the
  // render or on some frame — a.any_ordered, set by the host)
  const uint32_t slow_grid = (stats || a.force_ordered || a.any_ordered) ? (tiles < 4096u ? tiles : 4096u) : (tiles < 256u ? tiles : 256u);
  if (stats)
    hipLaunchKernelGGL(k_raster_slow<true>, dim3(slow_grid), dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL(k_raster_slow<false>, dim3(slow_grid), dim3(64), 0, s, a);
}

void launch_peel(const RenderArgs &a, const float *prev, int n_frames, hipStream_t s) {
  if (n_frames <= 0 || a.n_local_bands == 0) return;
  const uint32_t groups = ((uint32_t)n_frames + 7u) / 8u;
  hipLaunchKernelGGL(k_peel, dim3(groups * 8u * a.n_local_bands * a.tiles_x), dim3(64), 0, s, a, prev); // (k_raster<1>'s grid)
}

void launch_tex_convert(const uint8_t *d_bgr, int w, int h, int row_stride, uint32_t *d_bgrx, hipStream_t s) {
  int n = w * h;
  hipLaunchKernelGGL(k_tex_convert, dim3((n + 255) / 256), dim3(256), 0, s, d_bgr, w, h, row_stride, d_bgrx);
}

// ================================================================================================================
// k_composite, k_composite_grad — DEPTH LAYERS COMPOSITED FRONT TO BACK (srz_frameset_composite / _composite_grad, include/srz.h
// states the rule).  k_interp's shape on the passes' helpers: pass_walk, four pixels of a row per thread, quad_load, quad_store; no
// LDS, no barrier, no atomics.  A thread reads the id quads of ALL layers first (comp_cover: independent 16-byte loads, then the
// passes' owner test, four bits per layer), and loads a layer's alpha and colour quads only where the layer covers one of its pixels.
// The loops over the layers are unrolled by the build's maximum ML with the run-time count as a guard, so that the per-layer values (w_k in
// the forward; a_k, T_k and d_k in the backward) are registers and the layers' pointers scalar loads of the kernel arguments.  The
// channels go in register chunks of ATTR_CHUNK, as in k_interp.  EVERY pixel of the walk is written (quad_store, never
// quad_store_owned): a pixel no layer covers is bg (or +0) with T = 1, and +0 in the gradients of a layer that does not cover it.
// (At the end of the file, behind the launchers: no existing kernel moves.)
// ================================================================================================================
// the coverage of the thread's quad: bit 4 k + j = layer k covers pixel j
template <int ML> __device__ __forceinline__ uint32_t comp_cover(const CompositeArgs &a, const PassTile &t) {
  uint32_t idw[ML][4];
  const size_t off = (size_t)t.f * a.vis_stride + t.poff + t.rc.plane; // (plane 1: the ids)
#pragma unroll
  for (int k = 0; k < ML; ++k) {
    idw[k][0] = idw[k][1] = idw[k][2] = idw[k][3] = 0u;
    if ((uint32_t)k < a.n_layers) {
      if (t.whole) {
        const uint4 q = *reinterpret_cast<const uint4 *>(a.lvis[k] + off);
        idw[k][0] = q.x, idw[k][1] = q.y, idw[k][2] = q.z, idw[k][3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (t.x4 + j <= t.rc.tx1) idw[k][j] = f2u(a.lvis[k][off + j]);
      }
    }
  }
  const uint32_t n_tris = t.fd->n_tris;
  uint32_t cov = 0u;
#pragma unroll
  for (int k = 0; k < ML; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((idw[k][j] & ~S_CLASS_BIT) - 1u < n_tris) cov |= 1u << (4 * k + j); // (quad_ids' test: 0 and the bare class bit wrap)
  return cov;
}
// layer k's alpha quad: the plane's words, or the scalar in every pixel
__device__ __forceinline__ float4 comp_alpha(const CompositeArgs &a, const PassTile &t, int k) {
  float4 al[1] = {make_float4(a.opacity[k], a.opacity[k], a.opacity[k], a.opacity[k])};
  if (a.alpha[k]) quad_load(a.alpha[k] + (size_t)t.f * t.rc.plane + t.poff, t.rc.plane, al, t.whole, t.x4, t.rc.tx1);
  return al[0];
}
// planes c0 .. c0 + nc - 1 of the thread's quad in an n_ch-plane buffer
__device__ __forceinline__ void comp_chunk_load(const float *buf, const CompositeArgs &a, const PassTile &t, uint32_t c0, uint32_t nc,
                                                float4 (&v)[ATTR_CHUNK]) {
  const float *p = buf + (size_t)t.f * a.col_stride + t.poff + (size_t)c0 * t.rc.plane;
#pragma unroll
  for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
    float4 q[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
    if (i < nc) quad_load(p + (size_t)i * t.rc.plane, t.rc.plane, q, t.whole, t.x4, t.rc.tx1);
    v[i] = q[0];
  }
}
__device__ __forceinline__ void comp_chunk_store(float *buf, const CompositeArgs &a, const PassTile &t, uint32_t c0, uint32_t nc,
                                                 const float4 (&v)[ATTR_CHUNK]) {
  float *p = buf + (size_t)t.f * a.col_stride + t.poff + (size_t)c0 * t.rc.plane;
#pragma unroll
  for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
    if (i < nc) quad_store(p + (size_t)i * t.rc.plane, t.rc.plane, {v[i]}, t.whole, t.x4, t.rc.tx1);
}

template <int ML> __global__ __launch_bounds__(256) void k_composite(CompositeArgs a) {
  const uint32_t C = a.n_ch;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const TileRect &rc = t.rc;
    // ---- 1. every layer's ids, then w_k = a_k T_k of the covering layers and the final T
    const uint32_t cov = comp_cover<ML>(a, t);
    float4 T = make_float4(1.f, 1.f, 1.f, 1.f);
    float4 w[ML];
#pragma unroll
    for (int k = 0; k < ML; ++k) {
      w[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      const uint32_t m = (cov >> (4 * k)) & 15u;
      if (m == 0u) continue;
      const float4 al = comp_alpha(a, t, k);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (m & (1u << j)) {
          quad_at(w[k], j) = quad_at(al, j) * quad_at(T, j);
          quad_at(T, j) = quad_at(T, j) * (1.0f - quad_at(al, j));
        }
    }
    // ---- 2. the channels, ATTR_CHUNK at a time: acc = acc + col * w over the covering layers, then + bg * T
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 q[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < ML; ++k) {
        const uint32_t m = (cov >> (4 * k)) & 15u;
        if (m == 0u) continue;
        float4 col[ATTR_CHUNK];
        comp_chunk_load(a.col[k], a, t, c0, nc, col);
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (m & (1u << j)) quad_at(q[i], j) = quad_at(q[i], j) + quad_at(col[i], j) * quad_at(w[k], j);
      }
      if (a.bg) {
        float4 bg[ATTR_CHUNK];
        comp_chunk_load(a.bg, a, t, c0, nc, bg);
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) quad_at(q[i], j) = quad_at(q[i], j) + quad_at(bg[i], j) * quad_at(T, j);
      }
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
        if (i < nc) quad_store(t.out + (size_t)(c0 + i) * rc.plane, rc.plane, {q[i]}, t.whole, t.x4, rc.tx1);
    }
    if (a.through) quad_store(t.out + (size_t)C * rc.plane, rc.plane, {T}, t.whole, t.x4, rc.tx1);
  });
}

template <int ML> __global__ __launch_bounds__(256) void k_composite_grad(CompositeArgs a) {
  const uint32_t C = a.n_ch;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const TileRect &rc = t.rc;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // ---- 1. every layer's ids; a_k and T_k of the covering layers, recomputed as the forward computes them; the final T
    const uint32_t cov = comp_cover<ML>(a, t);
    float4 T = make_float4(1.f, 1.f, 1.f, 1.f);
    float4 al[ML], Tk[ML], d[ML];
#pragma unroll
    for (int k = 0; k < ML; ++k) {
      al[k] = Tk[k] = d[k] = zero4;
      const uint32_t m = (cov >> (4 * k)) & 15u;
      if (m == 0u) continue;
      al[k] = comp_alpha(a, t, k);
      Tk[k] = T;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (m & (1u << j)) quad_at(T, j) = quad_at(T, j) * (1.0f - quad_at(al[k], j));
    }
    const float *gout = a.gout + (size_t)t.f * a.frame_stride + t.poff;
    float4 S[1] = {zero4}; // gT, then + sum g_c bg_c
    if (a.through) quad_load(gout + (size_t)C * rc.plane, rc.plane, S, t.whole, t.x4, rc.tx1);
    // ---- 2. the channels, ATTR_CHUNK at a time: gbg and gcol leave, S's bg term and every d_k grow in channel order
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 g[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
        float4 q[1] = {zero4};
        if (i < nc) quad_load(gout + (size_t)(c0 + i) * rc.plane, rc.plane, q, t.whole, t.x4, rc.tx1);
        g[i] = q[0];
      }
      if (a.bg) {
        float4 bg[ATTR_CHUNK];
        comp_chunk_load(a.bg, a, t, c0, nc, bg);
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
          if (i < nc)
#pragma unroll
            for (int j = 0; j < 4; ++j) quad_at(S[0], j) = fmaf_(quad_at(g[i], j), quad_at(bg[i], j), quad_at(S[0], j));
      }
      if (a.gbg) {
        float4 o[ATTR_CHUNK];
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) quad_at(o[i], j) = quad_at(g[i], j) * quad_at(T, j);
        comp_chunk_store(a.gbg, a, t, c0, nc, o);
      }
#pragma unroll
      for (int k = 0; k < ML; ++k) {
        if ((uint32_t)k >= a.n_layers) continue;
        const uint32_t m = (cov >> (4 * k)) & 15u;
        if (m != 0u && a.want_d) {
          float4 col[ATTR_CHUNK];
          comp_chunk_load(a.col[k], a, t, c0, nc, col);
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc)
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (m & (1u << j)) quad_at(d[k], j) = fmaf_(quad_at(g[i], j), quad_at(col[i], j), quad_at(d[k], j));
        }
        if (a.gcol[k]) {
          float4 o[ATTR_CHUNK];
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              quad_at(o[i], j) = (m & (1u << j)) ? quad_at(g[i], j) * (quad_at(al[k], j) * quad_at(Tk[k], j)) : 0.f;
          comp_chunk_store(a.gcol[k], a, t, c0, nc, o);
        }
      }
    }
    // ---- 3. the alphas, from the last layer to the first: galpha = T_k (d - S), then S = a d + (1 - a) S
    if (!a.want_d) return;
#pragma unroll
    for (int k = ML - 1; k >= 0; --k) {
      if ((uint32_t)k >= a.n_layers) continue;
      const uint32_t m = (cov >> (4 * k)) & 15u;
      float4 ga[1] = {zero4};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (m & (1u << j)) {
          const float aj = quad_at(al[k], j), dj = quad_at(d[k], j), Sj = quad_at(S[0], j);
          quad_at(ga[0], j) = quad_at(Tk[k], j) * (dj - Sj);
          quad_at(S[0], j) = fmaf_(aj, dj, (1.0f - aj) * Sj);
        }
      if (a.galpha[k]) quad_store(a.galpha[k] + (size_t)t.f * rc.plane + t.poff, rc.plane, ga, t.whole, t.x4, rc.tx1);
    }
  });
}
// (two builds of each, for up to COMP_FEW layers and for up to SRZ_COMPOSITE_MAX: the per-layer registers of the unrolled loops are
// what the kernels cost, and the generic backward spilled to scratch when held to three waves a SIMD)
constexpr uint32_t COMP_FEW = 4;
void launch_composite(const CompositeArgs &a, hipStream_t s) {
  if (a.n_layers <= COMP_FEW) launch_pass<k_composite<(int)COMP_FEW>>(a, s);
  else launch_pass<k_composite<SRZ_COMPOSITE_MAX>>(a, s);
}
void launch_composite_grad(const CompositeArgs &a, hipStream_t s) {
  if (a.n_layers <= COMP_FEW) launch_pass<k_composite_grad<(int)COMP_FEW>>(a, s);
  else launch_pass<k_composite_grad<SRZ_COMPOSITE_MAX>>(a, s);
}


// ================================================================================================================
// k_tex_set, k_tex_set_grad — TEXTURE SETS (srz_frameset_texture_set / _texture_set_grad, include/srz.h states the rule): k_tex and
// k_tex_grad with the texture of each pixel picked by its owner's batch.  k_cube's and k_cube_grad's shape on the passes' helpers:
// pass_walk, quad_ids, quad_load, quad_store_owned; tex_tap and TexelTable are k_tex's and k_tex_grad's own, used as they are.
// The slot is a per-LANE value (a quad can straddle two meshes): one 2-byte gather of the owner's batch per owned pixel — not
// repeated for a pixel whose owner was looked up last — and one byte of the caller's map; a byte that names no slot leaves
// the pixel unsampled, so no byte of the map reaches an address.  The per-slot pointers and sizes are never indexed by the lane's
// slot (that would put the table into scratch): as in k_composite the loop over the slots is unrolled by SRZ_TEXSET_MAX with the
// run-time count as guard, a wave skips a slot none of its lanes has (ballot), and the slot's pointer and sizes are then scalar
// loads of the kernel arguments; what a sampled pixel keeps of its slot is its taps and the slot number, in registers.  The
// forward's channel loop is k_tex's slot after slot (the same unrolled loop and ballot: the texture stays a scalar base under the
// lanes' texel offsets — with a per-pixel pointer the build took 130 VGPRs and three waves a SIMD, this way 118 and k_tex's four);
// the backward's is k_tex_grad's with the texture's pointer at the frame per pixel (213 VGPRs, k_tex_grad's two waves).
// The gradient's table counts distinct (slot, texel) pairs of the tile: its key is slot << 28 | texel index — a texel index
// is below SRZ_TEX_MAX_SIZE^2 = 2^28, eight slots end at 2^31 —, so two slots that touch the same texel index are two entries.  A
// corner of a slot without gtex takes no entry and adds nothing.  The flush takes the slot out of the key and adds into THAT
// slot's gtex at its own frame stride (0: every frame folds into the one texture), and so does the straight-to-memory add of a
// corner that found no entry (ts_gtex: a chain of selects over the kernel arguments, no indexing).  Every thread of the workgroup
// reaches every barrier.
// (At the end of the file, behind the launchers: no existing kernel moves.)
// ================================================================================================================
constexpr uint32_t TS_IDX_BITS = 28;
static_assert((uint64_t)SRZ_TEX_MAX_SIZE * SRZ_TEX_MAX_SIZE <= (1ull << TS_IDX_BITS) && ((uint64_t)SRZ_TEXSET_MAX << TS_IDX_BITS) < 0xffffffffull,
              "a (slot, texel) pair + 1 fits the table's 32-bit key");
// what k_tex_set and k_tex_set_grad do alike in front of their channel loops: the owners, their batches' slots, u and v of a quad
// with an owner, and per sampled pixel (an owner with a slot whose u and v are both finite) its taps and the slot as the key's
// high bits -> `own` and `smp`.  keep(k, s): what else the caller keeps of slot s for pixel k, called where s is wave-uniform
template <class Keep>
__device__ __forceinline__ void texset_quad(const TexSetArgs &a, const PassTile &t, TexTap (&tap)[4], uint32_t (&hi)[4], uint32_t &own,
                                            uint32_t &smp, Keep keep) {
  uint32_t id[4];
  own = quad_ids<~S_CLASS_BIT>(t, a.vis + (size_t)t.f * a.vis_stride + t.poff, id), smp = 0u;
  if (own == 0u) return;
  float4 uv[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  quad_load(a.uv + (size_t)t.f * a.uv_stride + t.poff, t.rc.plane, uv, t.whole, t.x4, t.rc.tx1);
  const SRZ_CAS uint16_t *tri_batch = as_const(a.tri_batch) + t.fd->tri_off;
  const SRZ_CAS uint8_t *map = as_const(a.batch_slot);
  uint32_t bs[4], last_id = 0u, last_bs = SRZ_TEXSET_NONE; // (the owner looked up last, and its slot: no owner's id is 0)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    bs[k] = SRZ_TEXSET_NONE;
    if (!(own & (1u << k))) continue;
    if (id[k] != last_id) {
      const uint32_t b = tri_batch[id[k] - 1u]; // (id - 1 < the frame's triangle count: quad_ids)
      last_id = id[k], last_bs = b < a.n_batch_slot ? (uint32_t)map[b] : (uint32_t)SRZ_TEXSET_NONE;
    }
    bs[k] = last_bs;
    if (bs[k] < a.n_slots && tex_finite(quad_at(uv[0], k)) && tex_finite(quad_at(uv[1], k))) smp |= 1u << k;
  }
#pragma unroll
  for (uint32_t s = 0; s < SRZ_TEXSET_MAX; ++s) {
    if (s >= a.n_slots) continue;
    uint32_t m = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((smp & (1u << k)) && bs[k] == s) m |= 1u << k;
    if (__ballot(m != 0u) == 0ull) continue;
    const uint32_t tw = a.tex_w[s], th = a.tex_h[s];
    const bool wrap = ((a.wrap_mask >> s) & 1u) != 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (m & (1u << k)) {
        tap[k] = tex_tap(quad_at(uv[0], k), quad_at(uv[1], k), tw, th, wrap);
        hi[k] = s << TS_IDX_BITS;
        keep(k, s);
      }
  }
}
__global__ __launch_bounds__(256) void k_tex_set(TexSetArgs a) {
  const uint32_t C = a.n_ch;
  pass_walk<false>(a, [&](const PassTile &t) { // (no barrier in this kernel: a thread outside the frame just moves on)
    const TileRect &rc = t.rc;
    const bool fused = t.fused(a.flags_or);
    // ---- 1. owners, slots, u and v, the taps
    TexTap tap[4] = {};
    uint32_t hi[4] = {0u, 0u, 0u, 0u}, own, smp;
    texset_quad(a, t, tap, hi, own, smp, [](int, uint32_t) {});
    if (own == 0u && !fused) return;
    // ---- 2. the channels, ATTR_CHUNK at a time (k_tex's loop)
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 q[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) q[i] = make_float4(0.f, 0.f, 0.f, 0.f); // nobody, and an owner that is not sampled: zeros
      // (slot after slot, so that the texture is a scalar base under the lanes' texel offsets: a wave skips a slot it does not hold)
#pragma unroll
      for (uint32_t s = 0; s < SRZ_TEXSET_MAX; ++s) {
        if (s >= a.n_slots) continue;
        uint32_t m = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if ((smp & (1u << k)) && hi[k] == s << TS_IDX_BITS) m |= 1u << k;
        if (__ballot(m != 0u) == 0ull) continue;
        const SRZ_CAS float *slot_tex = as_const(a.tex[s]) + (size_t)t.f * a.tex_frame_stride[s];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!(m & (1u << k))) continue;
          const SRZ_CAS float *p00 = slot_tex + (size_t)tap[k].i00 * C + c0, *p01 = slot_tex + (size_t)tap[k].i01 * C + c0;
          const SRZ_CAS float *p10 = slot_tex + (size_t)tap[k].i10 * C + c0, *p11 = slot_tex + (size_t)tap[k].i11 * C + c0;
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) {
              const float t00 = p00[i], t01 = p01[i], t10 = p10[i], t11 = p11[i];
              const float top = fmaf_(tap[k].tx, t01 - t00, t00), bot = fmaf_(tap[k].tx, t11 - t10, t10);
              quad_at(q[i], k) = fmaf_(tap[k].ty, bot - top, top);
            }
        }
      }
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
        if (i >= nc) break;
        quad_store_owned(t.out + (size_t)(c0 + i) * rc.plane, t, {q[i]}, fused, own);
      }
    }
  });
}

// slot s's texel gradient at frame f (null: not asked for)
__device__ __forceinline__ float *ts_gtex(const TexSetArgs &a, uint32_t s, uint32_t f) {
  float *g = nullptr;
  uint64_t stride = 0u;
#pragma unroll
  for (uint32_t q = 0; q < SRZ_TEXSET_MAX; ++q)
    if (s == q) g = a.gtex[q], stride = a.tex_frame_stride[q];
  return g ? g + (size_t)f * stride : nullptr;
}
__global__ __launch_bounds__(256) void k_tex_set_grad(TexSetArgs a) {
  __shared__ TexelTable<TexSetArgs, ATTR_CHUNK> tb;
  const uint32_t tid = threadIdx.x;
  const uint32_t C = a.n_ch;
  const bool want_tex = a.want_tex != 0u, want_uv = a.out != nullptr;
  uint32_t asked = 0u; // bit s: slot s's gtex is asked for
#pragma unroll
  for (uint32_t q = 0; q < SRZ_TEXSET_MAX; ++q)
    if (a.gtex[q]) asked |= 1u << q;
  if (want_tex) {
    tb.init(tid);
    __syncthreads();
  }
  pass_walk<true>(a, [&](const PassTile &t) { // (a thread outside the frame owns nothing, and still meets the barriers)
    const TileRect &rc = t.rc;
    const bool fused = t.fused(a.flags_or);
    const float *gg = a.gout + (size_t)t.f * a.gout_stride + t.poff;
    // ---- 1. owners, slots, u and v, the taps
    TexTap tap[4] = {};
    const SRZ_CAS float *tex[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t hi[4] = {0u, 0u, 0u, 0u}, own, smp;
    texset_quad(a, t, tap, hi, own, smp, [&](int k, uint32_t s) { tex[k] = as_const(a.tex[s]) + (size_t)t.f * a.tex_frame_stride[s]; });
    // ---- 2. the table entries of the sampled pixels' corners, keyed by (slot, texel); none for a slot without gtex
    uint32_t slot[4][4] = {};
    uint32_t add = 0u; // the sampled pixels whose slot's gtex is asked for
    if (want_tex) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((smp & (1u << k)) && ((asked >> (hi[k] >> TS_IDX_BITS)) & 1u)) {
          add |= 1u << k;
          slot[k][0] = tb.slot(hi[k] | tap[k].i00), slot[k][1] = tb.slot(hi[k] | tap[k].i01);
          slot[k][2] = tb.slot(hi[k] | tap[k].i10), slot[k][3] = tb.slot(hi[k] | tap[k].i11);
        }
    }
    float au[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t n_used = 0u;
    // ---- 3. the channels, ATTR_CHUNK at a time
    for (uint32_t c0 = 0; c0 < C; c0 += ATTR_CHUNK) {
      const uint32_t nc = min(ATTR_CHUNK, C - c0);
      float4 g[ATTR_CHUNK];
#pragma unroll
      for (uint32_t i = 0; i < ATTR_CHUNK; ++i) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (smp != 0u) {
#pragma unroll
        for (uint32_t i = 0; i < ATTR_CHUNK; ++i) {
          if (i >= nc) break;
          gout_quad(gg + (size_t)(c0 + i) * rc.plane, t.whole, smp, g[i]);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(smp & (1u << k))) continue;
        if (want_uv) {
          const SRZ_CAS float *p00 = tex[k] + (size_t)tap[k].i00 * C + c0, *p01 = tex[k] + (size_t)tap[k].i01 * C + c0;
          const SRZ_CAS float *p10 = tex[k] + (size_t)tap[k].i10 * C + c0, *p11 = tex[k] + (size_t)tap[k].i11 * C + c0;
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) bilerp_chain(p00 + i, p01 + i, p10 + i, p11 + i, tap[k].tx, tap[k].ty, quad_at(g[i], k), au[k], av[k]);
        }
        if (add & (1u << k)) {
          const CornerW w = corner_weights(tap[k].tx, tap[k].ty);
#pragma unroll
          for (uint32_t i = 0; i < ATTR_CHUNK; ++i)
            if (i < nc) corner_adds(tb, slot[k], tap[k], w, quad_at(g[i], k), i, ts_gtex(a, hi[k] >> TS_IDX_BITS, t.f), C, c0 + i);
        }
      }
      // ---- 4. the table's values of this chunk into memory, each into its own slot's gtex (an entry's slot has one: step 2)
      if (want_tex)
        n_used = tb.flush(tid, c0, nc, [&a, f = t.f, C](uint32_t pair) {
          return ts_gtex(a, pair >> TS_IDX_BITS, f) + (size_t)(pair & ((1u << TS_IDX_BITS) - 1u)) * C;
        });
    }
    if (want_tex) tb.release(tid, n_used);
    // ---- 5. du, dv: whole quads (fused clear, or four owners), else the owned pixels only; an owner that is not sampled: (0, 0)
    if (want_uv && t.inside && (own != 0u || fused)) {
      float4 d[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (smp & (1u << k)) {
          uint32_t tw = 0u, th = 0u; // the extents of the pixel's slot
#pragma unroll
          for (uint32_t q = 0; q < SRZ_TEXSET_MAX; ++q)
            if ((hi[k] >> TS_IDX_BITS) == q) tw = a.tex_w[q], th = a.tex_h[q];
          quad_at(d[0], k) = tap[k].in_x ? au[k] * (float)tw : 0.0f;
          quad_at(d[1], k) = tap[k].in_y ? av[k] * (float)th : 0.0f;
        }
      quad_store_owned(t.out, t, d, fused, own);
    }
  });
}
void launch_tex_set(const TexSetArgs &a, hipStream_t s) { launch_pass<k_tex_set>(a, s); }
void launch_tex_set_grad(const TexSetArgs &a, hipStream_t s) { launch_pass<k_tex_set_grad>(a, s); }

} // namespace srz
