// Rate control: the quantiser of section 8a with every scale factor of a (clip, frame, channel) row
// raised by one offset k, the smallest k in [kmin, 254] whose packed row (section 8b) fits the row's bit budget.
//
//   k_quantize_budget  X, thr [B,F,N,C] float32, budget -> codes int16 [B,F,N,C], sf int8 [B,F,M,C], offset int16 [B,F,C],
//                      row bits int32 [B,F,C] (either of the last two may be null: ac_quantize on a plan with a row budget)
//
// One workgroup per (clip, frame) row and group of channels, as k_quantize, in three phases:
//   1. per (band, channel) the smallest thr key and the largest and smallest X key: band_stats (ac_rate_dev.h, shared with
//      k_clip_stats) on the run-wise segmented reduction of ac_band_dev.h, three ds_min / ds_max per run;
//   2. every band's sf0 (band_meta, one pass over the slots), then per channel one wave bisects [kmin, 254].  The widest
//      zigzag code of a band at an offset follows from its largest and smallest X alone (q is monotone in X for a fixed
//      step), so an evaluation of the row's length (row_bits_at) reads three LDS words per band and never touches the bins;
//   3. every bin quantised with the step of its band at the row's offset (band_sf, store_sf, quantize_bins).  Where a
//      group's bins fit IT passes of the block and CGT channels (N <= 1024, one or two channels), X stays in registers
//      from phase 1 -- the one form with a statistics loop and a codes loop of its own, over the same band_runs / fold and
//      code_or_zero; otherwise it is re-read.
#include "ac_internal.h"
#include "ac_rate_dev.h"

namespace ac {
namespace {

constexpr int kRateThreads = kRowThreads;
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

  // ---- phase 1: band extremes
  float xr[IT > 0 ? IT * CGT : 1];
  int jr[IT > 0 ? IT : 1];
  if constexpr (IT > 0) {
    band_stats_init(kt, kx, kn, slots);
    const int lane = threadIdx.x & 63;
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
    __syncthreads();
  } else {
    band_stats<0>(X, thr, rowN, band, N, M, C, c0, cg, CG, kt, kx, kn);
  }

  // ---- phase 2: sf0 of every band (in its own pass: inside the search loop it made the kernel spill SGPRs), then one wave
  // per channel (lanes take the bands; every slot a wave touches is its channel's)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int8_t* sfrow = sf + row * (size_t)M * C + c0;
  for (int s = threadIdx.x; s < M * cg; s += blockDim.x) {
    const int j = s / cg, c = s - j * cg;
    kt[j * CG + c] = band_meta(off[j + 1] - off[j], kt[j * CG + c]);
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
  if constexpr (IT > 0) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = it * (int)blockDim.x + (int)threadIdx.x;
      if (i < N) {
#pragma unroll
        for (int c = 0; c < CGT; ++c) {
          codes[rowN + (size_t)i * C + c0 + c] = code_or_zero(xr[it * CGT + c], inv[jr[it] * CG + c]);
        }
      }
    }
  } else {
    quantize_bins(X, codes, rowN, band, inv, N, C, c0, cg, CG);
  }
}

}  // namespace

int launch_quantize_budget(const ac_psy_plan* p, const float* X, const float* thr, int budget, const int32_t* row_budget,
                           int kmin, int16_t* codes, int8_t* sf, int16_t* offset, int32_t* row_bits, int B, int F, int C,
                           hipStream_t s) {
  if ((long long)B * F == 0 || C == 0) return AC_OK;
  const int M = p->M, N = p->N;
  RowLaunch l;
  if (int st = row_launch(p, B, F, C, lds_group(C, kRateLdsBytes, 12 * M), &l)) return st;
  const int passes = (N + l.threads - 1) / l.threads, cgt = l.cgt;
  // X in registers where a group is the whole of one or two channels and the row fits four passes of the block
  const int it = passes == 1 ? 1 : passes == 2 ? 2 : passes <= 4 ? 4 : 0;
#define AC_RATE_LAUNCH(IT_, CGT_)                                                                                         \
  hipLaunchKernelGGL((k_quantize_budget<IT_, CGT_>), l.grid(), dim3(l.threads), (size_t)12 * M * l.CG, s, X, thr, budget, \
                     row_budget, kmin, codes, sf, offset, row_bits, p->d_qoff, p->d_qband, N, M, C, l.CG)
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
