// The level of packed rows in one launch, without decoding (k_level_p, defined in ac_level.hip on level_row below; DESIGN.md
// section 8j): the sibling of k_transrate_p and k_mix_p that stops after the parse.  filters_n = 1024 with bark_bands_n = 64; one
// wave owns one row and lane j holds band j; a tail wave simply exits.
//
// Per row, with mix_row's steps as they are:
//   parse    the 26 header words through p_load_word, lane j reads band j's width, one wave-wide scan gives its sf field and
//            first code bit; the rest of the row is staged with plain dword loads where it is plain, clamped loads elsewhere.
//   extract  extract_sig_p on the staged row: the lane's 16 codes.
//   square   q q as a 32-bit integer (at most 2^30), added to the bin's band in 64 64-bit LDS words (ds_add_u64): Q_j is exact.
//   level    lane j: e_j = fp32(fp32(Q_j) w(s_j)), w(s) = fp32(step(s) step(s)), +0 in a band whose stored sf is -128 -- a
//            product that is never half of a multiply-add -- then six xor steps of float32 adds: lane 0 holds the fold tree's
//            sum.  Lane 0 stores energy[r] and bad[r] (1 where any band's sf is -128).
// No output slot is staged and no search runs.  The values are those of the composition: ac_unpack, int64 squares summed per
// band, the float32 product with the table of w, the fold tree as float32 adds.
#pragma once
#include "ac_mix_dev.h"

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

  // ---- parse: the header, the band records, then the rest of the row
  int64_t at = pr.index[r];
  // a row start beyond the buffer reads nothing; clamping it keeps start + 4 k from overflowing
  at = at > pr.nbytes ? pr.nbytes : (at < -(1ll << 40) ? -(1ll << 40) : at);
  if (lane < P_HDR_WORDS) st_in[lane] = p_load_word(pr.data, pr.nbytes, at + 4ll * lane);
  qs[lane] = 0ull;
  wave_sync();
  const uint32_t len = (uint32_t)pr.off[lane + 1] - (uint32_t)pr.off[lane];   // bins of the lane's band
  uint32_t nw_in;
  {
    uint32_t wd = p_get_bits(st_in, 5u * lane, 5);
    if (wd > 16) wd = 31;   // 17 .. 30: damaged, read as a non-finite band
    const uint32_t v = p_stores(wd) ? (1u << 16) | (wd * len) : 0u;   // (code bits of a row <= 16 N = 2^14)
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += up;
    }
    const uint32_t ex = incl - v;
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    const uint32_t cbase = 5u * P_M + 8u * (total >> 16);   // first code bit
    uint32_t sfb = 0;
    if (wd == 31) sfb = 0x80u;
    else if (p_stores(wd)) sfb = p_get_bits(st_in, 5u * P_M + 8u * (ex >> 16), 8);
    rec_in[lane] = ((cbase + (ex & 0xffffu)) << 13) | (sfb << 5) | wd;
    nw_in = (cbase + (total & 0xffffu) + 31u) >> 5;   // <= (T_IN_BITS + 31) / 32 whatever the widths say
  }
  // (words behind the row's last are never staged: a window's second word may read what LDS held there, and is masked off)
  if (at >= 0 && (at & 3) == 0 && at + 4ll * nw_in <= pr.nbytes) {
    const uint32_t* row = reinterpret_cast<const uint32_t*>(pr.data + at);
    for (uint32_t k = P_HDR_WORDS + lane; k < nw_in; k += 64) st_in[k] = row[k];
  } else {
    for (uint32_t k = P_HDR_WORDS + lane; k < nw_in; k += 64) st_in[k] = p_load_word(pr.data, pr.nbytes, at + 4ll * k);
  }
  wave_sync();

  // ---- extract and square: the lane's 16 codes into their bands' sums
  uint32_t bw[8];
  load_bw_p<8>(pr, lane, bw);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t j0 = bw[i] & 63u, j1 = (bw[i] >> 6) & 63u;
    const uint32_t wi = p_pos(rec_in[j0], bw[i] >> 12) >> 5;   // < T_IN_WORDS - 1: a field starts inside the longest row
    uint32_t cw, sfs;
    extract_sig_p(rec_in, bw[i], st_in[wi], st_in[wi + 1], cw, sfs);
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
  const int s = t_rec_sf(rec_in[lane]);
  const bool isbad = s == -128;
  const float step = quant_step(isbad ? 0 : s);
  const float wgt = qmul(step, step);
  float v = isbad ? 0.f : x_opaque(qmul((float)qs[lane], wgt));   // (u64 -> float32 rounds to nearest even)
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
