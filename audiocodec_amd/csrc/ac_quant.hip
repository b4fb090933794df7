// Perceptual quantiser (no counterpart in the reference, whose add_noise -- psychoacoustic.py:150-167 --
// models its noise): per (clip, frame, channel) and scale-factor band j one step 2^(sf/4) with step * sqrt(3) <= the band's
// smallest masking threshold, so the uniform quantiser's noise (RMS step / sqrt 12) stays at or below add_noise's thr / 6.
//
//   k_quantize    X, thr [B,F,N,C] float32 -> codes int16 [B,F,N,C], sf int8 [B,F,M,C]
//   k_dequantize  codes, sf -> X^ = fp32(code * step(sf)) (the fallback of ac_decode_quantized; the independent path the
//                 fused synthesis from codes, k_inv_fast_q in ac_fast_inv.hip, is tested against)
//
// One workgroup per (clip, frame) row and group of channels.  The band minimum is a segmented reduction over contiguous
// bins: each wave takes 64 consecutive bins, reduces every run of equal band index with a log-step suffix minimum across
// the lanes (keys monotone along the wave), and the first lane of each run folds it into the band's LDS slot with one
// ds_min -- so lanes of one instruction never hit the same LDS address.
#include <climits>

#include "ac_internal.h"
#include "ac_quant_dev.h"

namespace ac {
namespace {

constexpr int kQuantThreads = 256;
constexpr int kQuantLdsBytes = 32768;   // 8 bytes per (band, channel) slot of a workgroup: key + inverse step

// grid (B*F rows, channel groups); block: a multiple of 64 threads; CG channels per group (a group's slots fit the LDS)
__global__ __launch_bounds__(kQuantThreads) void k_quantize(const float* __restrict__ X, const float* __restrict__ thr,
                                                           int16_t* __restrict__ codes, int8_t* __restrict__ sf,
                                                           const int32_t* __restrict__ off, const uint16_t* __restrict__ band,
                                                           int N, int M, int C, int CG) {
  extern __shared__ int qlds[];
  const int slots = M * CG;
  int* kmin = qlds;                                             // [M][CG] smallest key of the band
  float* inv = reinterpret_cast<float*>(qlds + slots);          // [M][CG] 2^(-sf/4), NaN for sf = -128
  const int c0 = blockIdx.y * CG, cg = min(CG, C - c0);
  const size_t row = (size_t)blockIdx.x;
  const size_t rowN = row * (size_t)N * C;
  for (int s = threadIdx.x; s < slots; s += blockDim.x) kmin[s] = INT_MAX;
  __syncthreads();

  const int lane = threadIdx.x & 63;
  for (int base = 0; base < N; base += blockDim.x) {
    const int i = base + (int)threadIdx.x;
    const bool valid = i < N;
    const int key = valid ? (int)band[i] : -1;   // (-1: past the last bin, the end of the wave's last run)
    const int prev = __shfl_up(key, 1);
    const bool head = valid && (lane == 0 || prev != key);
    bool same[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      // (the shuffle outside the condition: under a divergent branch ds_bpermute would read 0 from the lanes it masks off)
      const int d = 1 << k, kd = __shfl_down(key, d);
      same[k] = (lane + d < 64) && kd == key;
    }
    for (int c = 0; c < cg; ++c) {
      int v = INT_MAX;
      if (valid) {
        const size_t e = rowN + (size_t)i * C + c0 + c;
        const float x = X[e], t = thr[e];
        v = (__builtin_isfinite(x) && __builtin_isfinite(t)) ? ordered_key(t) : INT_MIN;
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int w = __shfl_down(v, 1 << k);
        if (same[k]) v = min(v, w);
      }
      if (head) atomicMin(&kmin[key * CG + c], v);
    }
  }
  __syncthreads();

  int8_t* sfrow = sf + row * (size_t)M * C + c0;
  for (int s = threadIdx.x; s < M * cg; s += blockDim.x) {
    const int j = s / cg, c = s - j * cg;
    int q;
    if (off[j] == off[j + 1]) q = 0;                 // empty band
    else if (kmin[j * CG + c] == INT_MIN) q = -128;  // NaN / Inf in the band
    else q = scale_factor_of(key_value(kmin[j * CG + c]));
    sfrow[(size_t)j * C + c] = (int8_t)q;
    inv[j * CG + c] = q == -128 ? __builtin_nanf("") : quant_inv_step(q);
  }
  __syncthreads();

  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const int j = band[i];
    for (int c = 0; c < cg; ++c) {
      const size_t e = rowN + (size_t)i * C + c0 + c;
      const float r = inv[j * CG + c];
      short q = 0;
      if (!__builtin_isnan(r)) q = (short)(int)fminf(fmaxf(__builtin_rintf(qmul(X[e], r)), -32767.f), 32767.f);
      codes[e] = q;
    }
  }
}

// grid: B*F rows; every element of a row: X^ = fp32(code * step(sf of its band)).  Bins in the outer loop, channels in
// the inner one (no division by C), as in k_quantize.
__global__ __launch_bounds__(kQuantThreads) void k_dequantize(const int16_t* __restrict__ codes, const int8_t* __restrict__ sf,
                                                             float* __restrict__ X, const uint16_t* __restrict__ band,
                                                             int N, int M, int C) {
  const size_t row = (size_t)blockIdx.x;
  const size_t rowN = row * (size_t)N * C;
  const int8_t* sfrow = sf + row * (size_t)M * C;
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const int8_t* sfb = sfrow + (size_t)band[i] * C;
    const size_t e = rowN + (size_t)i * C;
    for (int c = 0; c < C; ++c) X[e + c] = dequant(codes[e + c], sfb[c]);
  }
}

}  // namespace

int launch_quantize(const ac_psy_plan* p, const float* X, const float* thr, int16_t* codes, int8_t* sf, int B, int F, int C,
                    hipStream_t s) {
  const long long rows = (long long)B * F;
  if (rows == 0 || C == 0) return AC_OK;
  if (rows > 2147483647ll) {
    set_error("problem too large for one launch (%lld rows)", rows);
    return AC_EINVAL;
  }
  const int M = p->M, N = p->N;
  const int CG = std::max(1, std::min(C, kQuantLdsBytes / (8 * M)));
  const int groups = (C + CG - 1) / CG;
  const int threads = std::min(kQuantThreads, (N + 63) / 64 * 64);
  hipLaunchKernelGGL(k_quantize, dim3((unsigned)rows, (unsigned)groups), dim3(threads), (size_t)8 * M * CG, s, X, thr, codes, sf,
                     p->d_qoff, p->d_qband, N, M, C, CG);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

int launch_dequantize(const ac_psy_plan* p, const int16_t* codes, const int8_t* sf, float* X, int B, int F, int C,
                      hipStream_t s) {
  const long long rows = (long long)B * F;
  if (rows == 0 || C == 0) return AC_OK;
  if (rows > 2147483647ll) {
    set_error("problem too large for one launch (%lld rows)", rows);
    return AC_EINVAL;
  }
  const int threads = std::min(kQuantThreads, (p->N + 63) / 64 * 64);
  hipLaunchKernelGGL(k_dequantize, dim3((unsigned)rows), dim3(threads), 0, s, codes, sf, X, p->d_qband, p->N, p->M, C);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
