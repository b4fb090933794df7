// Perceptual quantiser (no counterpart in the reference, whose add_noise -- psychoacoustic.py:150-167 --
// models its noise): per (clip, frame, channel) and scale-factor band j one step 2^(sf/4) with step * sqrt(3) <= the band's
// smallest masking threshold, so the uniform quantiser's noise (RMS step / sqrt 12) stays at or below add_noise's thr / 6.
//
//   k_quantize    X, thr [B,F,N,C] float32 -> codes int16 [B,F,N,C], sf int8 [B,F,M,C]
//   k_dequantize  codes, sf -> X^ = fp32(code * step(sf)) (the fallback of ac_decode_quantized; the independent path the
//                 fused synthesis from codes, k_inv_fast_q in ac_fast_inv.hip, is tested against)
//
// One workgroup per (clip, frame) row and group of channels.  The band minimum is the run-wise segmented reduction of
// ac_band_dev.h (band_runs, run_reduce) with one ds_min per run.  The phases the packer and rate control share with this
// kernel live there too (store_sf, quantize_bins), the arithmetic in ac_quant_dev.h, the launch geometry in row_launch
// (ac_internal.h).
#include "ac_band_dev.h"
#include "ac_internal.h"

namespace ac {
namespace {

constexpr int kQuantThreads = kRowThreads;
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
    const BandRuns r = band_runs(band, i, N, lane);
    for (int c = 0; c < cg; ++c) {
      int v = INT_MAX;
      if (valid) {
        const size_t e = rowN + (size_t)i * C + c0 + c;
        v = thr_key(X[e], thr[e]);
      }
      v = run_reduce(r, v, MinOp());
      if (r.head) atomicMin(&kmin[r.key * CG + c], v);
    }
  }
  __syncthreads();

  int8_t* sfrow = sf + row * (size_t)M * C + c0;
  for (int s = threadIdx.x; s < M * cg; s += blockDim.x) {
    const int j = s / cg, c = s - j * cg;
    const int q = band_scale_factor(off[j] == off[j + 1], kmin[j * CG + c]);
    store_sf(q, &sfrow[(size_t)j * C + c], &inv[j * CG + c]);
  }
  __syncthreads();

  quantize_bins(X, codes, rowN, band, inv, N, C, c0, cg, CG);
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
  if ((long long)B * F == 0 || C == 0) return AC_OK;
  RowLaunch l;
  if (int st = row_launch(p, B, F, C, lds_group(C, kQuantLdsBytes, 8 * p->M), &l)) return st;
  hipLaunchKernelGGL(k_quantize, l.grid(), dim3(l.threads), (size_t)8 * p->M * l.CG, s, X, thr, codes, sf, p->d_qoff,
                     p->d_qband, p->N, p->M, C, l.CG);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

int launch_dequantize(const ac_psy_plan* p, const int16_t* codes, const int8_t* sf, float* X, int B, int F, int C,
                      hipStream_t s) {
  if ((long long)B * F == 0 || C == 0) return AC_OK;
  RowLaunch l;
  if (int st = row_launch(p, B, F, C, C, &l)) return st;
  hipLaunchKernelGGL(k_dequantize, dim3((unsigned)l.rows), dim3(l.threads), 0, s, codes, sf, X, p->d_qband, p->N, p->M, C);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
