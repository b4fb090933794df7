// Packed bitstream of quantised spectra (no counterpart in the reference): every (clip, frame, channel)
// row of codes int16 [B,F,N,C] and sf int8 [B,F,M,C] becomes a run of little-endian 32-bit words that stores each
// scale-factor band at the bit width its largest zigzag code needs.  No variable-length codes: a row's 5-bit width fields
// fix the bit position of every field in it, so packing and unpacking are parallel within a row.
//
//   k_pack_sizes   codes, sf -> byte length of every row (into index, scanned in place)
//   k_scan_reduce  \
//   k_scan_top      > exclusive scan of the row lengths into index [B,F,C] + the total byte count (reduce, then scan)
//   k_scan_apply   /
//   k_pack         codes, sf, index -> data (the row staged in LDS, every field ORed in with ds_or_b32, stored as dwords)
//   k_unpack       data, index -> the canonical codes and sf (the row staged in LDS from loads clamped to nbytes)
//
// One workgroup per (clip, frame) and group of channels, as in k_quantize: the [N, C] block of a frame is read and written
// coalesced.  The band maximum of zz(code) is the run-wise segmented reduction of ac_band_dev.h (band_runs, run_reduce) with
// one ds_max per run.  A band's bit offset comes from a block-wide exclusive scan (block_scan, ac_band_dev.h) over the bands
// of (stored bands, code bits) in one 64-bit sum.  zigzag is ac_quant_dev.h's; rows and threads come from row_launch
// (ac_internal.h).
#include "ac_band_dev.h"
#include "ac_internal.h"

namespace ac {
namespace {

constexpr int kPackThreads = kRowThreads;
constexpr int kPackLdsBytes = 32768;   // the LDS a workgroup's channel group aims at (one channel may take more, < 64 KB)
constexpr int kScanThreads = 256;
constexpr int kScanPer = 8;            // row lengths per thread of the scan
constexpr int kScanTile = kScanThreads * kScanPer;

__device__ __forceinline__ int16_t unzigzag(uint32_t z) { return (int16_t)((z >> 1) ^ (0u - (z & 1u))); }
__device__ __forceinline__ uint32_t bit_length(uint32_t m) { return 32u - (uint32_t)__clz(m); }
__device__ __forceinline__ bool stores(uint32_t w) { return w - 1u < 16u; }   // widths 1 .. 16 store an sf and codes

// LDS words of one channel's staged row: the worst case 5M + sum_j (8 + 16 len_j) bits, in whole words
__host__ __device__ inline int row_words(int N, int M) { return (16 * N + 13 * M + 31) / 32; }

// ORs the w-bit field v (v < 2^w, w <= 16) into bit p of the LDS row st: at most two words
__device__ __forceinline__ void put_bits(uint32_t* st, uint32_t p, uint32_t v, uint32_t w) {
  if (v == 0) return;
  const uint32_t q = p >> 5, sh = p & 31;
  atomicOr(&st[q], v << sh);
  if (sh + w > 32) atomicOr(&st[q + 1], v >> (32 - sh));
}
// the w-bit field at bit p of the LDS row st (w <= 16): v_alignbit_b32 over the one or two words it touches
__device__ __forceinline__ uint32_t get_bits(const uint32_t* st, uint32_t p, uint32_t w) {
  const uint32_t q = p >> 5, sh = p & 31;
  const uint32_t lo = st[q], hi = sh + w > 32 ? st[q + 1] : 0u;
  return __builtin_amdgcn_alignbit(hi, lo, sh) & ((1u << w) - 1u);
}

// the largest zz(code) of every band and channel of the group into mx[j * CG + c] (zeroed by the caller): the segmented
// reduction of ac_band_dev.h with one ds_max per run
__device__ void band_max(const int16_t* __restrict__ codes, size_t rowN, const uint16_t* __restrict__ band, int N, int C,
                         int c0, int cg, int CG, uint32_t* mx) {
  const int lane = threadIdx.x & 63;
  for (int base = 0; base < N; base += blockDim.x) {
    const int i = base + (int)threadIdx.x;
    const BandRuns r = band_runs(band, i, N, lane);
    for (int c = 0; c < cg; ++c) {
      uint32_t v = i < N ? zigzag(codes[rowN + (size_t)i * C + c0 + c]) : 0u;
      v = run_reduce(r, v, MaxOp());
      if (r.head && v) atomicMax(&mx[r.key * CG + c], v);
    }
  }
}

// the width field of band j: 31 for sf = -128, else the bit length of the band's largest zz (0: empty or all zeros)
__device__ __forceinline__ uint32_t band_width(uint32_t mx, int s) { return s == -128 ? 31u : bit_length(mx); }

// grid (B*F rows, channel groups): the byte length of every row, ((5M + sum over stored bands of 8 + w len) + 31) / 32 * 4
__global__ __launch_bounds__(kPackThreads) void k_pack_sizes(const int16_t* __restrict__ codes, const int8_t* __restrict__ sf,
                                                            int64_t* __restrict__ lens, const int32_t* __restrict__ off,
                                                            const uint16_t* __restrict__ band, int N, int M, int C, int CG) {
  extern __shared__ uint32_t plds[];
  uint32_t* mx = plds;              // [M][CG]
  uint32_t* bits = plds + M * CG;   // [CG]
  const int c0 = blockIdx.y * CG, cg = min(CG, C - c0);
  const size_t row = (size_t)blockIdx.x;
  for (int s = threadIdx.x; s < M * CG + CG; s += blockDim.x) plds[s] = 0;
  __syncthreads();
  band_max(codes, row * (size_t)N * C, band, N, C, c0, cg, CG, mx);
  __syncthreads();
  const int8_t* sfrow = sf + row * (size_t)M * C + c0;
  for (int s = threadIdx.x; s < M * cg; s += blockDim.x) {
    const int j = s / cg, c = s - j * cg;
    const uint32_t w = band_width(mx[j * CG + c], sfrow[(size_t)j * C + c]);
    if (stores(w)) atomicAdd(&bits[c], 8u + w * (uint32_t)(off[j + 1] - off[j]));
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cg; c += blockDim.x)
    lens[row * C + c0 + c] = (int64_t)((5u * M + bits[c] + 31u) >> 5) * 4;
}

// scan, step 1: the sum of every tile of kScanTile lengths
__global__ __launch_bounds__(kScanThreads) void k_scan_reduce(const int64_t* __restrict__ lens, int64_t* __restrict__ part,
                                                             int64_t R) {
  __shared__ uint64_t sc[16];
  const int64_t t0 = (int64_t)blockIdx.x * kScanTile;
  uint64_t v = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    const int64_t e = t0 + k * kScanThreads + threadIdx.x;
    if (e < R) v += (uint64_t)lens[e];
  }
  uint64_t all;
  block_scan(v, &all, sc);
  if (threadIdx.x == 0) part[blockIdx.x] = (int64_t)all;
}

// scan, step 2 (one workgroup): the tile sums -> their exclusive prefix, in place; *total = the byte count of the stream
__global__ __launch_bounds__(kScanThreads) void k_scan_top(int64_t* __restrict__ part, int64_t T, int64_t* __restrict__ total) {
  __shared__ uint64_t sc[16];
  uint64_t carry = 0;
  for (int64_t b = 0; b < T; b += blockDim.x) {
    const int64_t e = b + threadIdx.x;
    const uint64_t v = e < T ? (uint64_t)part[e] : 0;
    uint64_t all;
    const uint64_t ex = block_scan(v, &all, sc);
    if (e < T) part[e] = (int64_t)(carry + ex);
    carry += all;
  }
  if (threadIdx.x == 0) *total = (int64_t)carry;
}

// scan, step 3: every tile's exclusive scan plus its prefix from step 2 (part = NULL for a single tile, which also writes
// the total)
__global__ __launch_bounds__(kScanThreads) void k_scan_apply(int64_t* __restrict__ index, const int64_t* __restrict__ part,
                                                            int64_t R, int64_t* __restrict__ total) {
  __shared__ uint64_t sc[16];
  const int64_t e0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
  uint64_t v[kScanPer], sum = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    v[k] = e0 + k < R ? (uint64_t)index[e0 + k] : 0;
    sum += v[k];
  }
  uint64_t all;
  uint64_t run = block_scan(sum, &all, sc) + (part ? (uint64_t)part[blockIdx.x] : 0);
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    if (e0 + k < R) index[e0 + k] = (int64_t)run;
    run += v[k];
  }
  if (!part && threadIdx.x == 0) *total = (int64_t)all;
}

// LDS of one channel group: staged rows [CG][W], band slots [M][CG], the 16 scan slots and per channel the code base and
// row length (k_unpack: also the sf field number of every band [M][CG], uint16)
__host__ __device__ inline size_t pack_lds_bytes(int N, int M, int CG, bool unpack) {
  return 16 * 8 + (size_t)CG * (4 * row_words(N, M) + 4 * M + 8) + (unpack ? (size_t)CG * M * 2 + 2 : 0);
}

// grid (B*F rows, channel groups): every row of the group staged in LDS, written at index[row] as whole dwords
__global__ __launch_bounds__(kPackThreads) void k_pack(const int16_t* __restrict__ codes, const int8_t* __restrict__ sf,
                                                      const int64_t* __restrict__ index, uint8_t* __restrict__ data,
                                                      const int32_t* __restrict__ off, const uint16_t* __restrict__ band,
                                                      int N, int M, int C, int CG) {
  extern __shared__ uint64_t pk_lds[];
  uint64_t* sc = pk_lds;                                          // [16]
  uint32_t* stage = reinterpret_cast<uint32_t*>(pk_lds + 16);    // [CG][W]
  const int W = row_words(N, M);
  uint32_t* slot = stage + (size_t)CG * W;                         // [M][CG]: mx, then (code bit offset << 5) | width
  uint32_t* cbase = slot + M * CG;                                 // [CG] first code bit
  uint32_t* rbits = cbase + CG;                                    // [CG] bits of the row before padding
  const int c0 = blockIdx.y * CG, cg = min(CG, C - c0);
  const size_t row = (size_t)blockIdx.x;
  const size_t rowN = row * (size_t)N * C;
  for (int s = threadIdx.x; s < CG * W + M * CG; s += blockDim.x) stage[s] = 0;
  __syncthreads();
  band_max(codes, rowN, band, N, C, c0, cg, CG, slot);
  __syncthreads();

  // widths, scale factors and the band offsets, channel by channel: one block-wide scan of (stored bands << 32 | code bits)
  const int8_t* sfrow = sf + row * (size_t)M * C + c0;
  for (int c = 0; c < cg; ++c) {
    uint32_t* st = stage + (size_t)c * W;
    uint64_t carry = 0;
    for (int jb = 0; jb < M; jb += blockDim.x) {
      const int j = jb + (int)threadIdx.x;
      uint32_t w = 0;
      int s = 0;
      if (j < M) {
        s = sfrow[(size_t)j * C + c];
        w = band_width(slot[j * CG + c], s);
      }
      const uint64_t v = stores(w) ? (1ull << 32) | (uint64_t)(w * (uint32_t)(off[j + 1] - off[j])) : 0ull;
      uint64_t all;
      const uint64_t ex = carry + block_scan(v, &all, sc);
      carry += all;
      if (j < M) {
        put_bits(st, 5u * j, w, 5);
        if (stores(w)) put_bits(st, 5u * M + 8u * (uint32_t)(ex >> 32), (uint32_t)(uint8_t)s, 8);
        slot[j * CG + c] = ((uint32_t)ex << 5) | w;
      }
    }
    if (threadIdx.x == 0) {
      cbase[c] = 5u * M + 8u * (uint32_t)(carry >> 32);
      rbits[c] = cbase[c] + (uint32_t)carry;
    }
  }
  __syncthreads();

  // codes: bin i of band j at cbase + (band offset) + w (i - o_j)
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const int j = band[i];
    const uint32_t di = (uint32_t)(i - off[j]);
    for (int c = 0; c < cg; ++c) {
      const uint32_t sl = slot[j * CG + c], w = sl & 31u;
      if (stores(w))
        put_bits(stage + (size_t)c * W, cbase[c] + (sl >> 5) + w * di, zigzag(codes[rowN + (size_t)i * C + c0 + c]), w);
    }
  }
  __syncthreads();

  for (int c = 0; c < cg; ++c) {
    const int nw = (int)((rbits[c] + 31u) >> 5);
    uint32_t* dst = reinterpret_cast<uint32_t*>(data + index[row * C + c0 + c]);
    const uint32_t* st = stage + (size_t)c * W;
    for (int k = threadIdx.x; k < nw; k += blockDim.x) dst[k] = st[k];
  }
}

// the little-endian word at byte a of data; bytes outside [0, nbytes) read as 0 (never loaded)
__device__ __forceinline__ uint32_t load_word(const uint8_t* __restrict__ data, int64_t nbytes, int64_t a) {
  if (a >= 0 && a + 4 <= nbytes && (a & 3) == 0) return *reinterpret_cast<const uint32_t*>(data + a);
  uint32_t r = 0;
  for (int k = 0; k < 4; ++k) {
    const int64_t e = a + k;
    if (e >= 0 && e < nbytes) r |= (uint32_t)data[e] << (8 * k);
  }
  return r;
}

// grid (B'*F' rows of index, channel groups): the rows at index[row] staged in LDS, decoded into the canonical codes and sf
__global__ __launch_bounds__(kPackThreads) void k_unpack(const uint8_t* __restrict__ data, int64_t nbytes,
                                                        const int64_t* __restrict__ index, int16_t* __restrict__ codes,
                                                        int8_t* __restrict__ sf, const int32_t* __restrict__ off,
                                                        const uint16_t* __restrict__ band, int N, int M, int C, int CG) {
  extern __shared__ uint64_t pk_lds[];
  uint64_t* sc = pk_lds;
  uint32_t* stage = reinterpret_cast<uint32_t*>(pk_lds + 16);    // [CG][W]
  const int W = row_words(N, M);
  uint32_t* slot = stage + (size_t)CG * W;                         // [M][CG] (code bit offset << 5) | width
  uint32_t* cbase = slot + M * CG;                                 // [CG]
  uint32_t* rbits = cbase + CG;                                    // [CG]
  uint16_t* sfno = reinterpret_cast<uint16_t*>(rbits + CG);       // [M][CG] the band's sf field number
  const int c0 = blockIdx.y * CG, cg = min(CG, C - c0);
  const size_t row = (size_t)blockIdx.x;
  const int hw = (5 * M + 31) >> 5;   // words holding the width fields
  // a row start beyond the buffer reads nothing; clamping it keeps start + 4 k from overflowing
  auto start_of = [&](int c) {
    const int64_t a = index[row * C + c0 + c];
    return a > nbytes ? nbytes : (a < -(1ll << 40) ? -(1ll << 40) : a);
  };

  for (int c = 0; c < cg; ++c) {
    const int64_t a = start_of(c);
    for (int k = threadIdx.x; k < hw; k += blockDim.x) stage[(size_t)c * W + k] = load_word(data, nbytes, a + 4ll * k);
  }
  __syncthreads();

  for (int c = 0; c < cg; ++c) {
    const uint32_t* st = stage + (size_t)c * W;
    uint64_t carry = 0;
    for (int jb = 0; jb < M; jb += blockDim.x) {
      const int j = jb + (int)threadIdx.x;
      uint32_t w = 0;
      if (j < M) {
        w = get_bits(st, 5u * j, 5);
        if (w > 16) w = 31;   // 17 .. 30: damaged, read as a non-finite band
      }
      const uint64_t v = stores(w) ? (1ull << 32) | (uint64_t)(w * (uint32_t)(off[j + 1] - off[j])) : 0ull;
      uint64_t all;
      const uint64_t ex = carry + block_scan(v, &all, sc);
      carry += all;
      if (j < M) {
        slot[j * CG + c] = ((uint32_t)ex << 5) | w;
        sfno[j * CG + c] = (uint16_t)(ex >> 32);
      }
    }
    if (threadIdx.x == 0) {
      cbase[c] = 5u * M + 8u * (uint32_t)(carry >> 32);
      rbits[c] = cbase[c] + (uint32_t)carry;   // <= 32 W whatever the widths say
    }
  }
  __syncthreads();

  for (int c = 0; c < cg; ++c) {
    const int64_t a = start_of(c);
    const int nw = (int)((rbits[c] + 31u) >> 5);
    for (int k = hw + threadIdx.x; k < nw; k += blockDim.x) stage[(size_t)c * W + k] = load_word(data, nbytes, a + 4ll * k);
  }
  __syncthreads();

  int8_t* sfrow = sf + row * (size_t)M * C + c0;
  for (int s = threadIdx.x; s < M * cg; s += blockDim.x) {
    const int j = s / cg, c = s - j * cg;
    const uint32_t w = slot[j * CG + c] & 31u;
    int q = 0;
    if (w == 31) q = -128;
    else if (stores(w)) q = (int8_t)get_bits(stage + (size_t)c * W, 5u * M + 8u * sfno[j * CG + c], 8);
    sfrow[(size_t)j * C + c] = (int8_t)q;
  }

  const size_t rowN = row * (size_t)N * C;
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const int j = band[i];
    const uint32_t di = (uint32_t)(i - off[j]);
    for (int c = 0; c < cg; ++c) {
      const uint32_t sl = slot[j * CG + c], w = sl & 31u;
      int16_t q = 0;
      if (stores(w)) q = unzigzag(get_bits(stage + (size_t)c * W, cbase[c] + (sl >> 5) + w * di, w));
      codes[rowN + (size_t)i * C + c0 + c] = q;
    }
  }
}

// channels per workgroup: as many as kPackLdsBytes holds, at least one (at most 40 KB at N = 8192, M = 4096)
int pack_group(int N, int M, int C, bool unpack) {
  int CG = C;
  while (CG > 1 && pack_lds_bytes(N, M, CG, unpack) > (size_t)kPackLdsBytes) CG = (CG + 1) / 2;
  return CG;
}

}  // namespace

size_t pack_scratch_bytes(long long R) {
  const long long T = (R + kScanTile - 1) / kScanTile;
  return T > 1 ? (size_t)T * 8 : 0;
}

int launch_pack_index(const ac_psy_plan* p, const int16_t* codes, const int8_t* sf, int64_t* index, int64_t* total,
                      void* scratch, int B, int F, int C, hipStream_t s) {
  const int M = p->M, N = p->N;
  RowLaunch l;
  if (int st = row_launch(p, B, F, C, lds_group(C, kPackLdsBytes, 4 * M + 4), &l)) return st;
  hipLaunchKernelGGL(k_pack_sizes, l.grid(), dim3(l.threads), (size_t)4 * (M * l.CG + l.CG), s, codes, sf, index, p->d_qoff,
                     p->d_qband, N, M, C, l.CG);
  AC_HIP_CHECK(hipGetLastError());
  const long long R = l.rows * C, T = (R + kScanTile - 1) / kScanTile;
  if (T > 1) {
    int64_t* part = static_cast<int64_t*>(scratch);
    hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)T), dim3(kScanThreads), 0, s, index, part, (int64_t)R);
    AC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kScanThreads), 0, s, part, (int64_t)T, total);
    AC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)T), dim3(kScanThreads), 0, s, index, (const int64_t*)part, (int64_t)R,
                       total);
  } else {
    hipLaunchKernelGGL(k_scan_apply, dim3(1), dim3(kScanThreads), 0, s, index, (const int64_t*)nullptr, (int64_t)R, total);
  }
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

int launch_pack(const ac_psy_plan* p, const int16_t* codes, const int8_t* sf, const int64_t* index, uint8_t* data, int B,
                int F, int C, hipStream_t s) {
  const int M = p->M, N = p->N;
  RowLaunch l;
  if (int st = row_launch(p, B, F, C, pack_group(N, M, C, false), &l)) return st;
  hipLaunchKernelGGL(k_pack, l.grid(), dim3(l.threads), pack_lds_bytes(N, M, l.CG, false), s, codes, sf, index, data,
                     p->d_qoff, p->d_qband, N, M, C, l.CG);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

int launch_unpack(const ac_psy_plan* p, const uint8_t* data, int64_t nbytes, const int64_t* index, int16_t* codes, int8_t* sf,
                  int B, int F, int C, hipStream_t s) {
  const int M = p->M, N = p->N;
  RowLaunch l;
  if (int st = row_launch(p, B, F, C, pack_group(N, M, C, true), &l)) return st;
  hipLaunchKernelGGL(k_unpack, l.grid(), dim3(l.threads), pack_lds_bytes(N, M, l.CG, true), s, data, nbytes, index, codes, sf,
                     p->d_qoff, p->d_qband, N, M, C, l.CG);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
