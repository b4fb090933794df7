// Device helpers of the quantiser shared by its kernels (ac_quant.hip, ac_pack.hip, ac_rate.hip, ac_clip_rate.hip) and the
// synthesis from codes (ac_fast_inv_dev.h): one definition, so that every path quantises and dequantises bit for bit alike.
// DESIGN.md section 8a has the definition.
#pragma once
#include <climits>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace ac {

constexpr float kQuantSqrt3 = 1.73205080756887729353f;   // fp32(sqrt 3)

// a product that is never contracted into a multiply-add (the library builds with -ffp-contract=fast)
__device__ __forceinline__ float qmul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// fp32(2^(-r/4)), r = 0 .. 3
__device__ __forceinline__ float quant_ic(int r) {
  return r == 0 ? 1.0f : r == 1 ? 0.84089641525371454303f : r == 2 ? 0.70710678118654752440f : 0.59460355750136053336f;
}
// step(s) = ldexp(c[s & 3], s >> 2) (arithmetic shift), c[r] = fp32(2^(r/4)), s in [-128, 127]: c[r] lies in [1, 2), so the
// product is c[r]'s mantissa under the exponent 127 + (s >> 2) -- assembled from bits, without branches (v_cndmask only)
__device__ __forceinline__ uint32_t quant_step_bits(int s) {
  const int r = s & 3;
  const uint32_t mant = (r & 2) ? ((r & 1) ? 0x5744fdu : 0x3504f3u) : ((r & 1) ? 0x1837f0u : 0u);
  return ((uint32_t)(127 + (s >> 2)) << 23) | mant;
}
__device__ __forceinline__ float quant_step(int s) { return __uint_as_float(quant_step_bits(s)); }
// inv(s) = ldexp(ic[s & 3], -(s >> 2))
__device__ __forceinline__ float quant_inv_step(int s) { return __builtin_ldexpf(quant_ic(s & 3), -(s >> 2)); }
// X^ = fp32(code * step(sf)); sf = -128 (a band with NaN / Inf) dequantises to NaN
__device__ __forceinline__ float dequant(int code, int sf) {
  const uint32_t st = sf == -128 ? 0x7fc00000u : quant_step_bits(sf);
  return qmul((float)code, __uint_as_float(st));
}

// code = clamp(rint(fp32(x * inv)), +-32767) for the inverse step r of the bin's band
__device__ __forceinline__ int qcode(float x, float r) {
  return (int)fminf(fmaxf(__builtin_rintf(qmul(x, r)), -32767.f), 32767.f);
}
// the code that is stored: 0 throughout a band with sf = -128, whose inverse step is kept as NaN
__device__ __forceinline__ short code_or_zero(float x, float r) { return __builtin_isnan(r) ? (short)0 : (short)qcode(x, r); }
// zz(q) = (q << 1) ^ (q >> 31): 0, -1, 1, -2, ... -> 0, 1, 2, 3, ...  For every int16 q this is the 16-bit form
// ((q << 1) ^ (q >> 15)) & 0xffff of section 8b: q >> 15 and q >> 31 agree on a sign-extended int16, and zz(q) <= 65535
__device__ __forceinline__ uint32_t zigzag(int q) { return (uint32_t)((q << 1) ^ (q >> 31)); }

// float -> int key whose signed order is the float order (the map is its own inverse); NaN / Inf are flagged apart
__device__ __forceinline__ int ordered_key(float v) {
  const int u = __float_as_int(v);
  return u >= 0 ? u : (u ^ 0x7fffffff);
}
__device__ __forceinline__ float key_value(int k) { return __int_as_float(k >= 0 ? k : (k ^ 0x7fffffff)); }
// what a bin adds to its band's smallest-threshold key: INT_MIN marks a band that holds a NaN / Inf in X or thr
__device__ __forceinline__ int thr_key(float x, float t) {
  return (__builtin_isfinite(x) && __builtin_isfinite(t)) ? ordered_key(t) : INT_MIN;
}

// the largest s in [-127, 127] with fp32(step(s) * sqrt 3) <= m, else -127: a log2 estimate corrected against the criterion
__device__ inline int scale_factor_of(float m) {
  auto ok = [m](int s) { return qmul(quant_step(s), kQuantSqrt3) <= m; };
  if (!(m > 0.f)) return -127;
  int s = (int)floorf(4.f * log2f(m / kQuantSqrt3));
  s = max(-127, min(127, s));
  while (s < 127 && ok(s + 1)) ++s;
  while (s > -127 && !ok(s)) --s;
  return s;
}

}  // namespace ac
