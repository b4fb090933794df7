// Device helpers shared by the rate-control kernels (ac_rate.hip, section 8c; ac_clip_rate.hip, section 8d): a band's three
// statistics and the phase that gathers them (on the segmented reduction of ac_band_dev.h), a band's packed cost and scale
// factor at an offset, and a row's bits at an offset -- one definition, so that the per-row and the per-clip search count a
// row's bits alike.
#pragma once
#include "ac_band_dev.h"

namespace ac {

constexpr int kRateMaxOffset = 254;

// A band's statistics once its sf0 is known: meta = (length << 8) | (sf0 & 0xff); 0 for an empty band, -1 for sf0 = -128
// (both store nothing at any offset); kx, kn the ordered keys of the band's largest and smallest X.  FLAT as in
// band_scale_factor: the sf0 search runs for every lane and the special cases select afterwards; the value is the same
template <bool FLAT = false>
__device__ __forceinline__ int band_meta(int L, int kt) {
  if constexpr (FLAT) {
    const int s = scale_factor_of(key_value(kt));
    return L == 0 ? 0 : kt == INT_MIN ? -1 : (L << 8) | (s & 0xff);
  } else {
    return L == 0 ? 0 : kt == INT_MIN ? -1 : (L << 8) | (scale_factor_of(key_value(kt)) & 0xff);
  }
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

// bits_r(k) of a row from its bands' statistics: band j's meta, kx and kn at st[j * stride + {0, 1, 2} * plane] (the whole
// wave calls; lanes take the bands)
__device__ __forceinline__ int row_bits_at(const int* __restrict__ st, int stride, int plane, int M, int lane, int k) {
  int acc = 0;
  for (int j = lane; j < M; j += 64) {
    const int* b = st + j * stride;
    acc += band_bits(b[0], b[plane], b[2 * plane], k);
  }
  return 5 * M + wave_sum(acc);
}

// a bin's x and thr folded into its band's slot: the smallest thr key and the largest and smallest X key
__device__ __forceinline__ void fold(const BandRuns& r, bool valid, float x, float t, int* kt, int* kx, int* kn, int slot) {
  int vt = INT_MAX, vx = INT_MIN, vn = INT_MAX;
  if (valid) {
    vt = thr_key(x, t);
    vx = vn = ordered_key(x);
  }
  vt = run_reduce(r, vt, MinOp());
  vx = run_reduce(r, vx, MaxOp());
  vn = run_reduce(r, vn, MinOp());
  if (r.head) {
    atomicMin(&kt[slot], vt);
    atomicMax(&kx[slot], vx);
    atomicMin(&kn[slot], vn);
  }
}

__device__ __forceinline__ void band_stats_init(int* kt, int* kx, int* kn, int slots) {
  for (int s = threadIdx.x; s < slots; s += blockDim.x) {
    kt[s] = INT_MAX;
    kx[s] = INT_MIN;
    kn[s] = INT_MAX;
  }
  __syncthreads();
}

// The band statistics phase of a row's channels c0 .. c0 + cg - 1 into kt, kx, kn [M][CG] (LDS): any N; X and thr are read
// once and not kept.  CGT > 0: cg = CGT, a bin's loads of all its channels issued before the first fold.  Ends in a barrier.
template <int CGT>
__device__ __forceinline__ void band_stats(const float* __restrict__ X, const float* __restrict__ thr, size_t rowN,
                                           const uint16_t* __restrict__ band, int N, int M, int C, int c0, int cg, int CG,
                                           int* kt, int* kx, int* kn) {
  band_stats_init(kt, kx, kn, M * CG);
  const int lane = threadIdx.x & 63;
  for (int base = 0; base < N; base += blockDim.x) {
    const int i = base + (int)threadIdx.x;
    const bool valid = i < N;
    const BandRuns r = band_runs(band, i, N, lane);
    if constexpr (CGT > 0) {
      float x[CGT], t[CGT];
#pragma unroll
      for (int c = 0; c < CGT; ++c) {
        x[c] = t[c] = 0.f;
        if (valid) {
          const size_t e = rowN + (size_t)i * C + c0 + c;
          x[c] = X[e];
          t[c] = thr[e];
        }
      }
#pragma unroll
      for (int c = 0; c < CGT; ++c) fold(r, valid, x[c], t[c], kt, kx, kn, r.key * CG + c);
    } else {
      for (int c = 0; c < cg; ++c) {
        float x = 0.f, t = 0.f;
        if (valid) {
          const size_t e = rowN + (size_t)i * C + c0 + c;
          x = X[e];
          t = thr[e];
        }
        fold(r, valid, x, t, kt, kx, kn, r.key * CG + c);
      }
    }
  }
  __syncthreads();
}

}  // namespace ac
