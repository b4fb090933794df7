// Device phases shared by the kernels that take one (clip, frame) row and group of channels per workgroup -- the quantiser
// (ac_quant.hip), the packer (ac_pack.hip) and rate control (ac_rate.hip, ac_clip_rate.hip through ac_rate_dev.h): the
// run-wise segmented reduction over a wave, the block-wide scan, the scale factor with its inverse step, and the scalar codes
// loop.  One definition each, so that every path reduces, scans and quantises alike.
#pragma once
#include "ac_quant_dev.h"

namespace ac {

// The segmented reduction over one pass of the block: each wave takes 64 consecutive bins, whose band indices are monotone
// along the wave, so a band is a run of lanes.  Every run is reduced with a log-step suffix reduction across the lanes and
// its first lane folds the result into the band's LDS slot -- lanes of one instruction never hit the same LDS address.
struct BandRuns {
  int key;        // band of the lane's bin, -1 past the last bin (the end of the wave's last run)
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

// op over the lane's run from the lane to the run's end: on a head lane, op over the whole run.  Every lane of the wave
// calls it (the shuffles stay outside the condition, as in band_runs).
template <class T, class Op>
__device__ __forceinline__ T run_reduce(const BandRuns& r, T v, Op op) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const T w = __shfl_down(v, 1 << k);
    if (r.same[k]) v = op(v, w);
  }
  return v;
}
struct MinOp {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return min(a, b); }
};
struct MaxOp {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return max(a, b); }
};

// exclusive scan of v over the block (every thread calls it, blockDim.x <= 1024); *total = the sum.  sc: 16 LDS slots,
// free again when it returns.  WAVES > 0: the block is known to have that many waves (the sum over them unrolls).
template <int WAVES = 0>
__device__ inline uint64_t block_scan(uint64_t v, uint64_t* total, uint64_t* sc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = WAVES > 0 ? WAVES : (blockDim.x + 63) >> 6;
  uint64_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) sc[wave] = x;
  __syncthreads();
  uint64_t before = 0, all = 0;
  for (int k = 0; k < waves; ++k) {
    const uint64_t s = sc[k];
    before += k < wave ? s : 0;
    all += s;
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

// a band's scale factor from its smallest key: 0 for an empty band, -128 for a band that holds a NaN / Inf (key INT_MIN), else
// the criterion's.  FLAT: the search runs for every lane and the special cases select afterwards, so that it is not nested
// under their lane masks (the fused encode's frame loop has no scalar registers for them); the value is the same
template <bool FLAT = false>
__device__ __forceinline__ int band_scale_factor(bool empty, int kmin) {
  if constexpr (FLAT) {
    const int s = scale_factor_of(key_value(kmin));
    return empty ? 0 : kmin == INT_MIN ? -128 : s;
  } else {
    if (empty) return 0;
    if (kmin == INT_MIN) return -128;
    return scale_factor_of(key_value(kmin));
  }
}

// a band's scale factor q into sf and its inverse step into the LDS slot the codes loop reads: NaN for sf = -128
__device__ __forceinline__ void store_sf(int q, int8_t* __restrict__ sf, float* inv) {
  *sf = (int8_t)q;
  *inv = q == -128 ? __builtin_nanf("") : quant_inv_step(q);
}

// the codes of a row's bins for the cg channels from c0 on, any N and group: inv [M][CG] as store_sf left it.  Bins in the
// outer loop, channels in the inner one (no division by C).
__device__ __forceinline__ void quantize_bins(const float* __restrict__ X, int16_t* __restrict__ codes, size_t rowN,
                                              const uint16_t* __restrict__ band, const float* inv, int N, int C, int c0,
                                              int cg, int CG) {
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const int j = band[i];
    for (int c = 0; c < cg; ++c) {
      const size_t e = rowN + (size_t)i * C + c0 + c;
      codes[e] = code_or_zero(X[e], inv[j * CG + c]);
    }
  }
}

}  // namespace ac
