// Rate control per clip: one bit budget T_b for the F*C rows of a clip.  k_b is the smallest offset in
// [kmin, 254] at which the clip's padded rows fit T_b; a prefix of the rows (in r = f*C + c order) then takes k_b - 1 as far
// as the remaining bits reach.
//
//   k_clip_stats   X, thr [B,F,N,C] -> per (row, band) the three words band_bits() reads (meta with sf0, largest and
//                  smallest X key): stat [B*F*C][3][M] int32 (band_stats and band_meta of ac_rate_dev.h)
//   k_clip_total   one bisection step: adds the clip's total length at the step's offset into total[step][b]
//   k_clip_rows    each row's bits at k_b and at k_b - 1 -> rowbits [rows][2]; per (clip, split) the sums of the padded
//                  lengths at k_b and of the steps d_r
//   k_clip_fill    the scan of d_r over the clip's rows (block_scan of ac_band_dev.h) -> offset, row_bits_out, clip_offset,
//                  clip_bits_out
//   k_clip_codes   the codes and scale factors at each row's offset (reads X, the meta words and the offsets; band_sf,
//                  store_sf and, for any group, quantize_bins)
//
// A row's bits at an offset are row_bits_at (ac_rate_dev.h), the count k_quantize_budget searches with.
//
// A clip's rows are cut into S equal splits, one workgroup each (grid B x S), so that many short clips and one long clip
// both fill the chip.  Every sum is an integer sum: the results do not depend on the order of the additions.  No kernel
// waits for another inside a launch: a bisection step is one launch, and each launch derives the current [lo, hi] of its
// clip from the totals of the steps before it.
#include <algorithm>

#include "ac_internal.h"
#include "ac_rate_dev.h"

namespace ac {
namespace {

constexpr int kClipThreads = kRowThreads;
constexpr int kClipWaves = kClipThreads / 64;
constexpr int kClipLdsBytes = 32768;      // k_clip_stats: a group's slots, 12 bytes per (band, channel)
constexpr int kClipMaxSteps = 9;          // ceil(log2(509)): bisection steps over [-254, 254]
constexpr int kClipMaxSplits = 256;       // at most one thread of k_clip_fill per split
constexpr int kClipMinSplitRows = 16;     // four rows per wave at least
constexpr int kClipWorkgroups = 2048;     // eight per CU

typedef long long i64;
typedef unsigned long long u64;

struct ClipLayout {
  int S = 1, rps = 0;                     // splits per clip, rows per split
  size_t stat = 0, total = 0, split = 0, rowbits = 0, bytes = 0;   // byte offsets into the scratch
};

ClipLayout clip_layout(int M, long long B, long long R) {
  ClipLayout l;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const long long want = std::min<long long>(kClipMaxSplits, (kClipWorkgroups + B - 1) / B);
  const long long rps = std::max<long long>(kClipMinSplitRows, (R + want - 1) / want);
  l.rps = (int)std::min<long long>(rps, 2147483647ll);
  l.S = (int)std::max<long long>(1, (R + l.rps - 1) / l.rps);
  l.stat = 0;
  l.total = up((size_t)12 * M * B * R);
  l.split = l.total + up((size_t)8 * kClipMaxSteps * B);
  l.rowbits = l.split + up((size_t)16 * B * l.S);
  l.bytes = l.rowbits + up((size_t)8 * B * R);
  return l;
}

__device__ __forceinline__ int padded(int bits) { return (bits + 31) & ~31; }

// the clip's [lo, hi] after `steps` bisection steps: total[s][b] is the clip's length at the mid of step s
__device__ __forceinline__ void clip_range(const i64* __restrict__ total, int B, int b, int steps, int kmin, i64 T, int& lo,
                                           int& hi) {
  lo = kmin;
  hi = kRateMaxOffset;
  for (int s = 0; s < steps; ++s) {
    if (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (total[(size_t)s * B + b] <= T) hi = mid;
      else lo = mid + 1;
    }
  }
}

// ---- band statistics: grid (B*F rows, channel groups), k_quantize_budget's phase 1 and sf0 pass
template <int CGT>
__global__ __launch_bounds__(kClipThreads) void k_clip_stats(const float* __restrict__ X, const float* __restrict__ thr,
                                                              int* __restrict__ stat, const int32_t* __restrict__ off,
                                                              const uint16_t* __restrict__ band, int N, int M, int C, int CG) {
  extern __shared__ int clds[];
  const int slots = M * CG;
  int* kt = clds;               // [M][CG] smallest thr key
  int* kx = clds + slots;       // [M][CG] largest X key
  int* kn = clds + 2 * slots;   // [M][CG] smallest X key
  const int c0 = blockIdx.y * CG, cg = CGT > 0 ? CGT : min(CG, C - c0);
  const size_t row = (size_t)blockIdx.x;
  const size_t rowN = row * (size_t)N * C;
  band_stats<CGT>(X, thr, rowN, band, N, M, C, c0, cg, CG, kt, kx, kn);
  // per (channel, band) in the order the words are stored: consecutive threads write consecutive bands
  for (int s = threadIdx.x; s < M * cg; s += blockDim.x) {
    const int c = s / M, j = s - c * M, slot = j * CG + c;
    int* st = stat + (row * C + c0 + c) * (size_t)(3 * M);
    st[j] = band_meta(off[j + 1] - off[j], kt[slot]);
    st[M + j] = kx[slot];
    st[2 * M + j] = kn[slot];
  }
}

// ---- one bisection step: grid (B, S); waves take rows, lanes take bands
__global__ __launch_bounds__(kClipThreads) void k_clip_total(const int* __restrict__ stat, i64* __restrict__ total, i64 budget,
                                                              const i64* __restrict__ clip_budget, int kmin, int step, int B,
                                                              int R, int rps, int M) {
  __shared__ i64 part[kClipWaves];
  const int b = blockIdx.x;
  const i64 T = clip_budget ? clip_budget[b] : budget;
  int lo, hi;
  clip_range(total, B, b, step, kmin, T, lo, hi);
  if (lo >= hi) return;                                   // (uniform over the workgroup) the clip's search has ended
  const int mid = lo + ((hi - lo) >> 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.y * rps, r1 = min(R, r0 + rps);
  i64 acc = 0;
  for (int r = r0 + wave; r < r1; r += kClipWaves)
    acc += padded(row_bits_at(stat + ((size_t)b * R + r) * (size_t)(3 * M), 1, M, M, lane, mid));
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    i64 sum = 0;
#pragma unroll
    for (int w = 0; w < kClipWaves; ++w) sum += part[w];
    atomicAdd(reinterpret_cast<u64*>(total + (size_t)step * B + b), (u64)sum);
  }
}

// ---- each row's bits at k_b and at k_b - 1, and their sums per split: grid (B, S)
__global__ __launch_bounds__(kClipThreads) void k_clip_rows(const int* __restrict__ stat, const i64* __restrict__ total,
                                                             i64* __restrict__ split, int* __restrict__ rowbits, i64 budget,
                                                             const i64* __restrict__ clip_budget, int kmin, int steps, int B,
                                                             int R, int rps, int M) {
  __shared__ i64 part[2 * kClipWaves];
  const int b = blockIdx.x;
  const i64 T = clip_budget ? clip_budget[b] : budget;
  int k, hi;
  clip_range(total, B, b, steps, kmin, T, k, hi);
  const bool below = k > kmin;                            // there is an offset k_b - 1 in the range
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.y * rps, r1 = min(R, r0 + rps);
  i64 len = 0, step_sum = 0;
  for (int r = r0 + wave; r < r1; r += kClipWaves) {
    const int* st = stat + ((size_t)b * R + r) * (size_t)(3 * M);
    const int at = row_bits_at(st, 1, M, M, lane, k);
    const int under = below ? row_bits_at(st, 1, M, M, lane, k - 1) : at;
    if (lane == 0) {
      rowbits[2 * ((size_t)b * R + r)] = at;
      rowbits[2 * ((size_t)b * R + r) + 1] = under;
    }
    len += padded(at);
    step_sum += padded(under) - padded(at);
  }
  if (lane == 0) {
    part[wave] = len;
    part[kClipWaves + wave] = step_sum;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    i64 sum = 0;
#pragma unroll
    for (int w = 0; w < kClipWaves; ++w) sum += part[threadIdx.x * kClipWaves + w];
    split[2 * ((size_t)b * gridDim.y + blockIdx.y) + threadIdx.x] = sum;
  }
}

// ---- the fill: grid (B, S).  Every workgroup reads the clip's split sums (S <= kClipMaxSplits), so it knows the clip's
// length at k_b, the bits left, the sum of d over the splits before its own, and which split holds the end of the prefix.
__global__ __launch_bounds__(kClipThreads) void k_clip_fill(const i64* __restrict__ total, const i64* __restrict__ split,
                                                             const int* __restrict__ rowbits, int16_t* __restrict__ offset,
                                                             int32_t* __restrict__ row_bits, int16_t* __restrict__ clip_offset,
                                                             i64* __restrict__ clip_bits, i64 budget,
                                                             const i64* __restrict__ clip_budget, int kmin, int steps, int B,
                                                             int R, int rps) {
  __shared__ uint64_t sc[16];
  __shared__ i64 wbest[kClipWaves];
  const int b = blockIdx.x, S = gridDim.y, me = blockIdx.y;
  const i64 T = clip_budget ? clip_budget[b] : budget;
  int k, hi;
  clip_range(total, B, b, steps, kmin, T, k, hi);
  i64 len = 0;
  for (int s = 0; s < S; ++s) len += split[2 * ((size_t)b * S + s)];
  const bool fill = k > kmin && len <= T;                 // rule 3: not at kmin, and the budget is met
  const i64 left = T - len;                               // (may wrap for an unchecked T near INT64_MIN: fill is false there)
  // base = the sum of d over the splits before this one; last = the last split whose base is within the bits left: the
  // prefix ends in it (every split before it is filled whole), and it writes the clip's results
  i64 base = 0, run = 0;
  int last = 0;
  for (int s = 0; s < S; ++s) {
    if (s == me) base = run;
    if (fill && run <= left) last = s;
    run += split[2 * ((size_t)b * S + s) + 1];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = me * rps, r1 = min(R, r0 + rps);
  i64 carry = base, best = base;                          // best: the largest inclusive prefix sum within the bits left
  for (int c0 = r0; c0 < r1; c0 += kClipThreads) {
    const int r = c0 + (int)threadIdx.x;
    const bool valid = r < r1;
    int at = 0, under = 0;
    if (valid) {
      at = rowbits[2 * ((size_t)b * R + r)];
      under = rowbits[2 * ((size_t)b * R + r) + 1];
    }
    const i64 v = padded(under) - padded(at);
    uint64_t all;
    const i64 incl = carry + (i64)block_scan<kClipWaves>((uint64_t)v, &all, sc) + v;
    const bool lower = fill && incl <= left;
    if (valid) {
      offset[(size_t)b * R + r] = (int16_t)(lower ? k - 1 : k);
      if (row_bits) row_bits[(size_t)b * R + r] = lower ? under : at;
      if (lower) best = max(best, incl);
    }
    carry += (i64)all;
  }
  if (me != last) return;
  best = max(best, __shfl_xor(best, 32));
#pragma unroll
  for (int d = 16; d >= 1; d >>= 1) best = max(best, __shfl_xor(best, d));
  if (lane == 0) wbest[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kClipWaves; ++w) best = max(best, wbest[w]);
    if (clip_offset) clip_offset[b] = (int16_t)k;
    if (clip_bits) clip_bits[b] = len + (fill ? best : 0);
  }
}

// ---- the codes at the rows' offsets: grid (B*F rows, channel groups).  CGT = 1 / 2: the group is the whole of one or two
// channels and a thread takes a pair of bins (N is even) with one load and one store
template <int CGT>
__global__ __launch_bounds__(kClipThreads) void k_clip_codes(const float* __restrict__ X, const int* __restrict__ stat,
                                                              const int16_t* __restrict__ offset, int16_t* __restrict__ codes,
                                                              int8_t* __restrict__ sf, const uint16_t* __restrict__ band, int N,
                                                              int M, int C, int CG) {
  extern __shared__ int clds[];
  float* inv = reinterpret_cast<float*>(clds);   // [M][CG] the inverse step, NaN for sf = -128
  const int c0 = blockIdx.y * CG, cg = CGT > 0 ? CGT : min(CG, C - c0);
  const size_t row = (size_t)blockIdx.x;
  const size_t rowN = row * (size_t)N * C;
  int8_t* sfrow = sf + row * (size_t)M * C + c0;
  for (int s = threadIdx.x; s < M * cg; s += blockDim.x) {
    const int c = s / M, j = s - c * M;
    const size_t rc = row * C + c0 + c;
    store_sf(band_sf(stat[rc * (size_t)(3 * M) + j], (int)offset[rc]), &sfrow[(size_t)j * C + c], &inv[j * CG + c]);
  }
  __syncthreads();
  if constexpr (CGT == 2) {
    const float4* X4 = reinterpret_cast<const float4*>(X + rowN);
    short4* out = reinterpret_cast<short4*>(codes + rowN);
    for (int p = threadIdx.x; p < N / 2; p += blockDim.x) {
      const int j0 = band[2 * p], j1 = band[2 * p + 1];
      const float4 x = X4[p];
      short4 q;
      q.x = code_or_zero(x.x, inv[j0 * 2]);
      q.y = code_or_zero(x.y, inv[j0 * 2 + 1]);
      q.z = code_or_zero(x.z, inv[j1 * 2]);
      q.w = code_or_zero(x.w, inv[j1 * 2 + 1]);
      out[p] = q;
    }
  } else if constexpr (CGT == 1) {
    const float2* X2 = reinterpret_cast<const float2*>(X + rowN);
    short2* out = reinterpret_cast<short2*>(codes + rowN);
    for (int p = threadIdx.x; p < N / 2; p += blockDim.x) {
      const float2 x = X2[p];
      short2 q;
      q.x = code_or_zero(x.x, inv[band[2 * p]]);
      q.y = code_or_zero(x.y, inv[band[2 * p + 1]]);
      out[p] = q;
    }
  } else {
    quantize_bins(X, codes, rowN, band, inv, N, C, c0, cg, CG);
  }
}

}  // namespace

size_t clip_budget_scratch_bytes(const ac_psy_plan* p, long long B, long long R) { return clip_layout(p->M, B, R).bytes; }

int launch_quantize_clip_budget(const ac_psy_plan* p, const float* X, const float* thr, int64_t budget,
                                const int64_t* clip_budget, int kmin, int16_t* codes, int8_t* sf, int16_t* offset,
                                int32_t* row_bits, int16_t* clip_offset, int64_t* clip_bits, void* scratch, int B, int F, int C,
                                hipStream_t s) {
  const long long R = (long long)F * C;
  if ((long long)B * F == 0 || C == 0) return AC_OK;
  const int M = p->M, N = p->N;
  RowLaunch rl;
  if (int st = row_launch(p, B, F, C, lds_group(C, kClipLdsBytes, 12 * M), &rl, R)) return st;
  const ClipLayout l = clip_layout(M, B, R);
  char* base = static_cast<char*>(scratch);
  int* stat = reinterpret_cast<int*>(base + l.stat);
  i64* total = reinterpret_cast<i64*>(base + l.total);
  i64* split = reinterpret_cast<i64*>(base + l.split);
  int* rowbits = reinterpret_cast<int*>(base + l.rowbits);
  const i64* cb = reinterpret_cast<const i64*>(clip_budget);

  const int CG = rl.CG, threads = rl.threads, cgt = rl.cgt;
  const dim3 row_grid = rl.grid(), clip_grid((unsigned)B, (unsigned)l.S);
  int steps = 0;
  while ((1 << steps) < kRateMaxOffset - kmin + 1) ++steps;
  if (steps) AC_HIP_CHECK(hipMemsetAsync(total, 0, sizeof(i64) * steps * B, s));

#define AC_CLIP_STATS(CGT_)                                                                                              \
  hipLaunchKernelGGL((k_clip_stats<CGT_>), row_grid, dim3(threads), (size_t)12 * M * CG, s, X, thr, stat, p->d_qoff,      \
                     p->d_qband, N, M, C, CG)
  if (cgt == 1) AC_CLIP_STATS(1);
  else if (cgt == 2) AC_CLIP_STATS(2);
  else AC_CLIP_STATS(0);
#undef AC_CLIP_STATS
  for (int step = 0; step < steps; ++step)
    hipLaunchKernelGGL(k_clip_total, clip_grid, dim3(kClipThreads), 0, s, stat, total, (i64)budget, cb, kmin, step, B, (int)R,
                       l.rps, M);
  hipLaunchKernelGGL(k_clip_rows, clip_grid, dim3(kClipThreads), 0, s, stat, total, split, rowbits, (i64)budget, cb, kmin,
                     steps, B, (int)R, l.rps, M);
  hipLaunchKernelGGL(k_clip_fill, clip_grid, dim3(kClipThreads), 0, s, total, split, rowbits, offset, row_bits, clip_offset,
                     reinterpret_cast<i64*>(clip_bits), (i64)budget, cb, kmin, steps, B, (int)R, l.rps);
#define AC_CLIP_CODES(CGT_)                                                                                              \
  hipLaunchKernelGGL((k_clip_codes<CGT_>), row_grid, dim3(kClipThreads), (size_t)4 * M * CG, s, X, stat, offset, codes, sf, \
                     p->d_qband, N, M, C, CG)
  if (cgt == 1) AC_CLIP_CODES(1);
  else if (cgt == 2) AC_CLIP_CODES(2);
  else AC_CLIP_CODES(0);
#undef AC_CLIP_CODES
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
