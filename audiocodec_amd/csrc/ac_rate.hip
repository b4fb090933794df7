// Rate control: the quantiser of section 8a with every scale factor of a (clip, frame, channel) row
// raised by one offset k, the smallest k in [kmin, 254] whose packed row (section 8b) fits the row's bit budget.
//
//   k_quantize_budget  X, thr [B,F,N,C] float32, budget -> codes int16 [B,F,N,C], sf int8 [B,F,M,C], offset int16 [B,F,C],
//                      row bits int32 [B,F,C]
//
// One workgroup per (clip, frame) row and group of channels, as k_quantize, in three phases:
//   1. per (band, channel) the smallest thr key and the largest and smallest X key: k_quantize's run-wise segmented
//      reduction, three ds_min / ds_max per run;
//   2. every band's sf0 (one pass over the slots, as k_quantize), then per channel one wave bisects [kmin, 254].  The
//      widest zigzag code of a band at an offset follows from its largest and smallest X alone (q is monotone in X for a
//      fixed step), so an evaluation of the row's length reads three LDS words per band and never touches the bins;
//   3. every bin quantised with the step of its band at the row's offset.  Where a group's bins fit IT passes of the
//      block and CGT channels (N <= 1024, one or two channels), X stays in registers from phase 1; otherwise it is re-read.
#include "ac_internal.h"
#include "ac_rate_dev.h"

namespace ac {
namespace {

constexpr int kRateThreads = 256;
constexpr int kRateLdsBytes = 32768;   // a group's slots: 12 bytes per (band, channel)

// grid (B*F rows, channel groups); block: a multiple of 64 threads.  IT > 0: N <= IT * blockDim and every group holds CGT
// channels (X kept in registers); IT = 0: any N and group, X re-read in phase 3.
template <int IT, int CGT>
__global__ __launch_bounds__(kRateThreads) void k_quantize_budget(
    const float* __restrict__ X, const float* __restrict__ thr, int budget, const int32_t* __restrict__ row_budget,
    int kmin, int16_t* __restrict__ codes, int8_t* __restrict__ sf, int16_t* __restrict__ offset,
    int32_t* __restrict__ row_bits, const int32_t* __restrict__ off, const uint16_t* __restrict__ band, int N, int M, int C,
    int CG) {
  extern __shared__ int rlds[];
  const int slots = M * CG;
  int* kt = rlds;              // [M][CG] smallest thr key; from phase 2 the band's meta (band_bits)
  int* kx = rlds + slots;      // [M][CG] largest X key; from phase 2 the inverse step, NaN for sf = -128
  int* kn = rlds + 2 * slots;  // [M][CG] smallest X key
  const int c0 = blockIdx.y * CG, cg = CGT > 0 ? CGT : min(CG, C - c0);
  const size_t row = (size_t)blockIdx.x;
  const size_t rowN = row * (size_t)N * C;
  for (int s = threadIdx.x; s < slots; s += blockDim.x) {
    kt[s] = INT_MAX;
    kx[s] = INT_MIN;
    kn[s] = INT_MAX;
  }
  __syncthreads();

  // ---- phase 1: band extremes
  const int lane = threadIdx.x & 63;
  float xr[IT > 0 ? IT * CGT : 1];
  int jr[IT > 0 ? IT : 1];
  if constexpr (IT > 0) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = it * (int)blockDim.x + (int)threadIdx.x;
      const bool valid = i < N;
      const BandRuns r = band_runs(band, i, N, lane);
      jr[it] = r.key;
#pragma unroll
      for (int c = 0; c < CGT; ++c) {
        float x = 0.f, t = 0.f;
        if (valid) {
          const size_t e = rowN + (size_t)i * C + c0 + c;
          x = X[e];
          t = thr[e];
        }
        xr[it * CGT + c] = x;
        fold(r, valid, x, t, kt, kx, kn, r.key * CG + c);
      }
    }
  } else {
    for (int base = 0; base < N; base += blockDim.x) {
      const int i = base + (int)threadIdx.x;
      const bool valid = i < N;
      const BandRuns r = band_runs(band, i, N, lane);
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

  // ---- phase 2: sf0 of every band (in its own pass: inside the search loop it made the kernel spill SGPRs), then one wave
  // per channel (lanes take the bands; every slot a wave touches is its channel's)
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int8_t* sfrow = sf + row * (size_t)M * C + c0;
  for (int s = threadIdx.x; s < M * cg; s += blockDim.x) {
    const int j = s / cg, c = s - j * cg, L = off[j + 1] - off[j], t = kt[j * CG + c];
    kt[j * CG + c] = L == 0 ? 0 : t == INT_MIN ? -1 : (L << 8) | (scale_factor_of(key_value(t)) & 0xff);
  }
  __syncthreads();
  for (int c = wave; c < cg; c += nw) {
    auto bits_at = [&](int k) {
      int acc = 0;
      for (int j = lane; j < M; j += 64) acc += band_bits(kt[j * CG + c], kx[j * CG + c], kn[j * CG + c], k);
      return 5 * M + wave_sum(acc);
    };
    const size_t rc = row * C + c0 + c;
    const int R = row_budget ? row_budget[rc] : budget;
    // bits_at is non-increasing in k: the smallest k with bits_at(k) <= R, or the top of the range where none is
    int lo = kmin, hi = kRateMaxOffset;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (bits_at(mid) <= R) hi = mid;
      else lo = mid + 1;
    }
    const int bits = bits_at(lo);
    if (lane == 0) {
      offset[rc] = (int16_t)lo;
      if (row_bits) row_bits[rc] = bits;
    }
    for (int j = lane; j < M; j += 64) {
      const int s = j * CG + c, meta = kt[s];
      const int q = meta == 0 ? 0 : meta < 0 ? -128 : max(-127, min(127, (int)(int8_t)(meta & 0xff) + lo));
      sfrow[(size_t)j * C + c] = (int8_t)q;
      reinterpret_cast<float*>(kx)[s] = q == -128 ? __builtin_nanf("") : quant_inv_step(q);
    }
  }
  __syncthreads();

  // ---- phase 3: the codes at the row's offset
  const float* inv = reinterpret_cast<const float*>(kx);
  if constexpr (IT > 0) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = it * (int)blockDim.x + (int)threadIdx.x;
      if (i < N) {
#pragma unroll
        for (int c = 0; c < CGT; ++c) {
          const float r = inv[jr[it] * CG + c];
          codes[rowN + (size_t)i * C + c0 + c] = __builtin_isnan(r) ? (short)0 : (short)qcode(xr[it * CGT + c], r);
        }
      }
    }
  } else {
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
      const int j = band[i];
      for (int c = 0; c < cg; ++c) {
        const size_t e = rowN + (size_t)i * C + c0 + c;
        const float r = inv[j * CG + c];
        codes[e] = __builtin_isnan(r) ? (short)0 : (short)qcode(X[e], r);
      }
    }
  }
}

}  // namespace

int launch_quantize_budget(const ac_psy_plan* p, const float* X, const float* thr, int budget, const int32_t* row_budget,
                           int kmin, int16_t* codes, int8_t* sf, int16_t* offset, int32_t* row_bits, int B, int F, int C,
                           hipStream_t s) {
  const long long rows = (long long)B * F;
  if (rows == 0 || C == 0) return AC_OK;
  if (rows > 2147483647ll) {
    set_error("problem too large for one launch (%lld rows)", rows);
    return AC_EINVAL;
  }
  const int M = p->M, N = p->N;
  const int CG = std::max(1, std::min(C, kRateLdsBytes / (12 * M)));
  const int groups = (C + CG - 1) / CG;
  const int threads = std::min(kRateThreads, (N + 63) / 64 * 64);
  const int passes = (N + threads - 1) / threads;
  const size_t lds = (size_t)12 * M * CG;
  const dim3 grid((unsigned)rows, (unsigned)groups);
  // X in registers where a group is the whole of one or two channels and the row fits four passes of the block
  const int it = passes == 1 ? 1 : passes == 2 ? 2 : passes <= 4 ? 4 : 0;
  const int cgt = (CG == C && C <= 2) ? C : 0;
#define AC_RATE_LAUNCH(IT_, CGT_)                                                                                         \
  hipLaunchKernelGGL((k_quantize_budget<IT_, CGT_>), grid, dim3(threads), lds, s, X, thr, budget, row_budget, kmin, codes, \
                     sf, offset, row_bits, p->d_qoff, p->d_qband, N, M, C, CG)
  if (it == 0 || cgt == 0) AC_RATE_LAUNCH(0, 0);
  else if (cgt == 1) {
    if (it == 1) AC_RATE_LAUNCH(1, 1);
    else if (it == 2) AC_RATE_LAUNCH(2, 1);
    else AC_RATE_LAUNCH(4, 1);
  } else {
    if (it == 1) AC_RATE_LAUNCH(1, 2);
    else if (it == 2) AC_RATE_LAUNCH(2, 2);
    else AC_RATE_LAUNCH(4, 2);
  }
#undef AC_RATE_LAUNCH
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
