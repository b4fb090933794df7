// Device helpers shared by the rate-control kernels (ac_rate.hip, section 8c; ac_clip_rate.hip, section 8d): a band's packed
// cost at an offset from its three statistics, and the run-wise segmented reduction that gathers them -- one definition, so
// that the per-row and the per-clip search count a row's bits alike.
#pragma once
#include <climits>

#include "ac_quant_dev.h"

namespace ac {

constexpr int kRateMaxOffset = 254;

__device__ __forceinline__ int qcode(float x, float r) {
  return (int)fminf(fmaxf(__builtin_rintf(qmul(x, r)), -32767.f), 32767.f);
}
// zz(q) of section 8b for |q| <= 32767
__device__ __forceinline__ uint32_t zigzag(int q) { return (uint32_t)((q << 1) ^ (q >> 31)); }

// A band's statistics once its sf0 is known: meta = (length << 8) | (sf0 & 0xff); 0 for an empty band, -1 for sf0 = -128
// (both store nothing at any offset); kx, kn the ordered keys of the band's largest and smallest X
__device__ __forceinline__ int band_meta(int L, int kt) {
  return L == 0 ? 0 : kt == INT_MIN ? -1 : (L << 8) | (scale_factor_of(key_value(kt)) & 0xff);
}
__device__ __forceinline__ int band_bits(int meta, int kx, int kn, int k) {
  if (meta <= 0) return 0;
  const int s = max(-127, min(127, (int)(int8_t)(meta & 0xff) + k));
  const float r = quant_inv_step(s);
  const uint32_t z = max(zigzag(qcode(key_value(kx), r)), zigzag(qcode(key_value(kn), r)));
  const int w = z ? 32 - __builtin_clz(z) : 0;
  return w ? 8 + w * (meta >> 8) : 0;
}
// the scale factor a band with this meta word takes at offset k (section 8c rule 1)
__device__ __forceinline__ int band_sf(int meta, int k) {
  return meta == 0 ? 0 : meta < 0 ? -128 : max(-127, min(127, (int)(int8_t)(meta & 0xff) + k));
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// the segmented reduction of k_quantize over one pass of the block: runs of equal band index along the wave
struct BandRuns {
  int key;        // band of the lane's bin, -1 past the last bin
  bool head;      // the lane folds its run into the band's slot
  bool same[6];   // lane + 2^k lies in the same run
};

__device__ __forceinline__ BandRuns band_runs(const uint16_t* __restrict__ band, int i, int N, int lane) {
  BandRuns r;
  const bool valid = i < N;
  r.key = valid ? (int)band[i] : -1;
  const int prev = __shfl_up(r.key, 1);
  r.head = valid && (lane == 0 || prev != r.key);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    // (the shuffle outside the condition: under a divergent branch ds_bpermute would read 0 from the lanes it masks off)
    const int d = 1 << k, kd = __shfl_down(r.key, d);
    r.same[k] = (lane + d < 64) && kd == r.key;
  }
  return r;
}

__device__ __forceinline__ void fold(const BandRuns& r, bool valid, float x, float t, int* kt, int* kx, int* kn, int slot) {
  int vt = INT_MAX, vx = INT_MIN, vn = INT_MAX;
  if (valid) {
    vt = (__builtin_isfinite(x) && __builtin_isfinite(t)) ? ordered_key(t) : INT_MIN;
    vx = vn = ordered_key(x);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int d = 1 << k;
    const int wt = __shfl_down(vt, d), wx = __shfl_down(vx, d), wn = __shfl_down(vn, d);
    if (r.same[k]) {
      vt = min(vt, wt);
      vx = max(vx, wx);
      vn = min(vn, wn);
    }
  }
  if (r.head) {
    atomicMin(&kt[slot], vt);
    atomicMax(&kx[slot], vx);
    atomicMin(&kn[slot], vn);
  }
}

}  // namespace ac
