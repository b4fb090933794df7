// Requantiser: rate control of section 8c on a row that is already quantised.  The row's stored scale
// factors stand where sf0 stood and X^ = fp32(code * step(sf)) where X stood, so neither a spectrum nor a threshold is read.
//
//   k_requantize_budget  codes int16 [B,F,N,C], sf int8 [B,F,M,C], budget -> codes, sf, offset int16 [B,F,C],
//                        row bits int32 [B,F,C] (either of the last two may be null)
//
// One workgroup per (clip, frame) row and group of channels, in k_quantize_budget's three phases (ac_rate.hip):
//   1. per (band, channel) the largest and the smallest code: integer ds_max / ds_min on the run-wise segmented reduction
//      of ac_band_dev.h.  fp32(q * step) is monotone in q, so the band's largest and smallest X^ are those of the two codes;
//   2. every band's meta word from the stored scale factor (band_meta's encoding, no scale_factor_of) and the keys of the
//      two X^; then per channel one wave bisects [kmin, 254] with row_bits_at, and band_sf / store_sf write the new scale
//      factors -- the search of k_quantize_budget, word for word;
//   3. every bin: code_or_zero(dequant(q, stored sf), inverse step of the new sf).  The codes are read again (2 bytes a bin).
// The input need not be canonical: codes under sf = -128 count as 0 and an all-zero band counts as sf 0, which is how
// ac_unpack would return the row after ac_pack.  Input and output tensors must not overlap.
#include "ac_internal.h"
#include "ac_rate_dev.h"

namespace ac {
namespace {

constexpr int kRequantThreads = kRowThreads;
constexpr int kRequantLdsBytes = 32768;   // a group's slots: 12 bytes per (band, channel)

// the stored scale factor a meta word was made from (-128 for a band marked non-representable)
__device__ __forceinline__ int meta_sf(int meta) { return meta < 0 ? -128 : (int)(int8_t)(meta & 0xff); }

// grid (B*F rows, channel groups); block: a multiple of 64 threads
__global__ __launch_bounds__(kRequantThreads) void k_requantize_budget(
    const int16_t* __restrict__ codes_in, const int8_t* __restrict__ sf_in, int budget, const int32_t* __restrict__ row_budget,
    int kmin, int16_t* __restrict__ codes, int8_t* __restrict__ sf, int16_t* __restrict__ offset,
    int32_t* __restrict__ row_bits, const int32_t* __restrict__ off, const uint16_t* __restrict__ band, int N, int M, int C,
    int CG) {
  extern __shared__ int qlds[];
  const int slots = M * CG;
  int* kt = qlds;              // [M][CG] the band's meta (band_bits)
  int* kx = qlds + slots;      // [M][CG] largest code, then the key of its X^; from the search's end the inverse step
  int* kn = qlds + 2 * slots;  // [M][CG] smallest code, then the key of its X^
  const int c0 = blockIdx.y * CG, cg = min(CG, C - c0);
  const size_t row = (size_t)blockIdx.x;
  const size_t rowN = row * (size_t)N * C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;

  // ---- phase 1: band extremes of the codes
  for (int s = threadIdx.x; s < slots; s += blockDim.x) {
    kx[s] = INT_MIN;
    kn[s] = INT_MAX;
  }
  __syncthreads();
  for (int base = 0; base < N; base += blockDim.x) {
    const int i = base + (int)threadIdx.x;
    const bool valid = i < N;
    const BandRuns r = band_runs(band, i, N, lane);
    for (int c = 0; c < cg; ++c) {
      int vx = INT_MIN, vn = INT_MAX;
      if (valid) vx = vn = (int)codes_in[rowN + (size_t)i * C + c0 + c];
      vx = run_reduce(r, vx, MaxOp());
      vn = run_reduce(r, vn, MinOp());
      if (r.head) {
        atomicMax(&kx[r.key * CG + c], vx);
        atomicMin(&kn[r.key * CG + c], vn);
      }
    }
  }
  __syncthreads();

  // ---- phase 2: the meta word and the keys of every band, then one wave per channel searches the offset
  const int8_t* sfrow_in = sf_in + row * (size_t)M * C + c0;
  int8_t* sfrow = sf + row * (size_t)M * C + c0;
  for (int s = threadIdx.x; s < M * cg; s += blockDim.x) {
    const int j = s / cg, c = s - j * cg, e = j * CG + c;
    const int L = off[j + 1] - off[j];
    int sv = sfrow_in[(size_t)j * C + c];
    const int qx = kx[e], qn = kn[e];
    if (sv != -128 && qx == 0 && qn == 0) sv = 0;   // an all-zero band stores no scale factor
    kt[e] = L == 0 ? 0 : sv == -128 ? -1 : (L << 8) | (sv & 0xff);
    kx[e] = L == 0 ? 0 : ordered_key(dequant(qx, sv));
    kn[e] = L == 0 ? 0 : ordered_key(dequant(qn, sv));
  }
  __syncthreads();
  for (int c = wave; c < cg; c += nw) {
    const size_t rc = row * C + c0 + c;
    const int R = row_budget ? row_budget[rc] : budget;
    // a row's bits are non-increasing in k: the smallest k with row_bits_at(k) <= R, or the top of the range where none is
    int lo = kmin, hi = kRateMaxOffset;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (row_bits_at(kt + c, CG, slots, M, lane, mid) <= R) hi = mid;
      else lo = mid + 1;
    }
    const int bits = row_bits_at(kt + c, CG, slots, M, lane, lo);
    if (lane == 0) {
      if (offset) offset[rc] = (int16_t)lo;
      if (row_bits) row_bits[rc] = bits;
    }
    for (int j = lane; j < M; j += 64) {
      const int s = j * CG + c;
      store_sf(band_sf(kt[s], lo), &sfrow[(size_t)j * C + c], reinterpret_cast<float*>(kx) + s);
    }
  }
  __syncthreads();

  // ---- phase 3: the codes at the row's offset
  const float* inv = reinterpret_cast<const float*>(kx);
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const int j = band[i];
    for (int c = 0; c < cg; ++c) {
      const size_t e = rowN + (size_t)i * C + c0 + c;
      codes[e] = code_or_zero(dequant((int)codes_in[e], meta_sf(kt[j * CG + c])), inv[j * CG + c]);
    }
  }
}

}  // namespace

int launch_requantize_budget(const ac_psy_plan* p, const int16_t* codes_in, const int8_t* sf_in, int budget,
                             const int32_t* row_budget, int kmin, int16_t* codes, int8_t* sf, int16_t* offset,
                             int32_t* row_bits, int B, int F, int C, hipStream_t s) {
  if ((long long)B * F == 0 || C == 0) return AC_OK;
  const int M = p->M, N = p->N;
  RowLaunch l;
  if (int st = row_launch(p, B, F, C, lds_group(C, kRequantLdsBytes, 12 * M), &l)) return st;
  hipLaunchKernelGGL(k_requantize_budget, l.grid(), dim3(l.threads), (size_t)12 * M * l.CG, s, codes_in, sf_in, budget,
                     row_budget, kmin, codes, sf, offset, row_bits, p->d_qoff, p->d_qband, N, M, C, l.CG);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
