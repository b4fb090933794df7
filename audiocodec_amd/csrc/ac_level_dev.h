// The level of packed rows in one launch, without decoding (k_level_p, defined in ac_level.hip on level_row below; DESIGN.md
// section 8j), on the shared steps of ac_rows_dev.h: the sibling of k_transrate_p and k_mix_p that stops after the parse.  One
// wave owns one row and lane j holds band j; a tail wave simply exits.
//
// What this kernel adds behind the parse and the extract of the lane's 16 codes:
//   square   q q as a 32-bit integer (at most 2^30), added to the bin's band in 64 64-bit LDS words (ds_add_u64): Q_j is exact.
//   level    lane j: e_j = fp32(fp32(Q_j) w(s_j)), w(s) = fp32(step(s) step(s)), +0 in a band whose stored sf is -128 -- a
//            product that is never half of a multiply-add -- then six xor steps of float32 adds: lane 0 holds the fold tree's
//            sum.  Lane 0 stores energy[r] and bad[r] (1 where any band's sf is -128).
// No output slot is staged and no search runs.  The values are those of the composition: ac_unpack, int64 squares summed per
// band, the float32 product with the table of w, the fold tree as float32 adds.
#pragma once
#include "ac_rows_dev.h"

namespace ac {
namespace {

constexpr int L_WAVE_WORDS = T_IN_WORDS + 3 * P_M;   // staged input, records in, the bands' sums of squares (64 bits each)
static_assert((T_IN_WORDS + P_M) % 2 == 0 && L_WAVE_WORDS % 2 == 0, "the 64-bit sums lie at 8-byte phase");
static_assert(T_WAVES * L_WAVE_WORDS * 4 <= 65536, "a workgroup's slices fit LDS");

struct LevelArgs {
  PackedRows in;       // data, nbytes, index [rows], band32, off
  float* energy;       // [rows]
  uint8_t* bad;        // [rows] or null
  long long rows;
};

// row r of a.in -> energy[r], bad[r]; w: the wave's slice of LDS (L_WAVE_WORDS words)
__device__ __forceinline__ void level_row(const LevelArgs& a, long long r, int lane, uint32_t* w) {
  uint32_t* st_in = w;
  uint32_t* rec_in = w + T_IN_WORDS;
  unsigned long long* qs = reinterpret_cast<unsigned long long*>(rec_in + P_M);
  const PackedRows& pr = a.in;

  const int64_t at = row_start(pr.index, r, pr.nbytes);
  stage_header(st_in, pr.data, pr.nbytes, at, lane);
  qs[lane] = 0ull;
  const uint32_t len = (uint32_t)pr.off[lane + 1] - (uint32_t)pr.off[lane];   // bins of the lane's band
  stage_row(st_in, rec_in, pr.data, pr.nbytes, at, len, lane);

  // ---- extract and square: the lane's 16 codes into their bands' sums
  uint32_t bw[8];
  load_bw_p<8>(pr, lane, bw);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t j0 = bw[i] & 63u, j1 = (bw[i] >> 6) & 63u;
    uint32_t cw, sfs;
    extract_pair(st_in, rec_in, bw[i], cw, sfs);
    const int q0 = (int)(int16_t)(cw & 0xffffu), q1 = (int)(int16_t)(cw >> 16);
    const uint32_t u0 = (uint32_t)(q0 * q0), u1 = (uint32_t)(q1 * q1);   // <= 2^30 each
    if (j0 == j1) {
      if (u0 | u1) atomicAdd(&qs[j0], (unsigned long long)(u0 + u1));
    } else {
      if (u0) atomicAdd(&qs[j0], (unsigned long long)u0);
      if (u1) atomicAdd(&qs[j1], (unsigned long long)u1);
    }
  }
  wave_sync();

  // ---- level: band `lane`'s energy, then the fold tree over the wave
  const int s = rec_sf(rec_in[lane]);
  const bool isbad = s == -128;
  const float step = quant_step(isbad ? 0 : s);
  const float wgt = qmul(step, step);
  float v = isbad ? 0.f : opaque(qmul((float)qs[lane], wgt));   // (u64 -> float32 rounds to nearest even)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
  const unsigned long long anybad = __ballot(isbad);
  if (lane == 0) {
    a.energy[r] = v;
    if (a.bad) a.bad[r] = anybad ? 1 : 0;
  }
}

}  // namespace
}  // namespace ac
