// Packed rows of S sources to the packed rows of O mixes at the plan's budget in one launch (k_route_p, defined in ac_route.hip on
// route_row below): k_mix_p's sibling (ac_mix_dev.h) for a bridge, which stages every source row once and
// packs O rows from it.  One wave owns one row position r; a tail wave simply exits.  Output o is, byte for byte, mix_row's on
// the sources it hears, in source order, at its gains: both run x_add_source and x_pack_sum.
//
// What this kernel adds is the order of its loads.  Every source that is active at r and heard by at least one output is staged
// into its own slice of LDS: the 26 header words of ALL such sources are loaded before the first scan, and the first 128 body
// words of every plain row before the first of them is written to LDS, so the wave waits for memory twice, not 2 S times.  Rows
// that are off phase, negative or past the end take the clamped loads, a row longer than 154 words its further words in a loop
// (stage_body, ac_rows_dev.h).  An inactive or unheard row is never read.  Then o = 0 .. O-1 in order: the accumulators, band
// `lane`'s s0 / bad and the slot start afresh, the heard staged sources are summed in source order, the sum is packed into slot r
// of output o.  Gains and mutes are kernel arguments, wave-uniform.  The waves of a workgroup share nothing.
#pragma once
#include "ac_mix_dev.h"

namespace ac {
namespace {

constexpr int R_WAVES = 2;                               // row positions per workgroup
constexpr int R_SRC_WORDS = T_IN_WORDS + P_M;            // a staged source row, then its band records
constexpr int R_OUT_WORDS = T_OUT_WORDS + 4 * P_M;       // the staged slot, records out, flags, kx, kn
constexpr int R_BATCH = 2;                               // body words a lane loads per source before the first is written
// a wave's slice at S sources: the launch sizes the workgroup's (dynamic) LDS by it
constexpr int r_wave_words(int S) { return S * R_SRC_WORDS + R_OUT_WORDS; }
static_assert(R_WAVES * r_wave_words(AC_ROUTE_MAX_SOURCES) * 4 <= 65536, "a workgroup's slices fit 64 KB of LDS");

struct RouteArgs {
  const uint8_t* data[AC_ROUTE_MAX_SOURCES];
  int64_t nbytes[AC_ROUTE_MAX_SOURCES];
  const int64_t* index[AC_ROUTE_MAX_SOURCES];                // [rows] each
  int gain[AC_ROUTE_MAX_OUTPUTS * AC_ROUTE_MAX_SOURCES];     // [o * sources_n + i], scale-factor units in [-254, 254]
  uint32_t heard[AC_ROUTE_MAX_OUTPUTS];                      // bit i: output o hears source i
  uint32_t heard_any;                                        // the union: sources that are staged where active
  const uint8_t* active;                                     // [S][rows] or null: every row is read
  int sources_n, outputs_n;
  const uint32_t* band32;                                    // as PackedRows'
  const int32_t* off;
  PackOut out;                                               // data [O][rows row_bytes], fits [O][rows], row_bytes
  int16_t* offset;                                           // [O][rows] or null
  long long rows;
  int row_bits;                                              // the budget R
};

// rows r of the sources -> slot r of every output; w: the wave's slice of LDS (r_wave_words(a.sources_n) words)
__device__ __forceinline__ void route_row(const RouteArgs& a, long long r, int lane, uint32_t* w) {
  constexpr int SN = AC_ROUTE_MAX_SOURCES;
  uint32_t* st_out = w + a.sources_n * R_SRC_WORDS;
  int* rec_out = reinterpret_cast<int*>(st_out + T_OUT_WORDS);
  uint32_t* nz = reinterpret_cast<uint32_t*>(rec_out + P_M);
  int* kxs = reinterpret_cast<int*>(nz + P_M);
  int* kns = kxs + P_M;
  const uint32_t first = (uint32_t)a.off[lane];
  const uint32_t len = (uint32_t)a.off[lane + 1] - first;   // bins of the lane's band
  PackedRows pr;
  pr.band32 = a.band32;
  pr.off = a.off;
  uint32_t bw[8];
  load_bw_p<8>(pr, lane, bw);

  // ---- stage: the sources that are heard and active here (wave-uniform), every load of a kind before its first use
  uint32_t live = 0;
#pragma unroll
  for (int i = 0; i < SN; ++i)
    if (i < a.sources_n && ((a.heard_any >> i) & 1u) && (!a.active || a.active[(size_t)i * (size_t)a.rows + (size_t)r] != 0))
      live |= 1u << i;
  int64_t at[SN];
  uint32_t hdr[SN];
#pragma unroll
  for (int i = 0; i < SN; ++i) {
    at[i] = 0;
    hdr[i] = 0u;
    if ((live >> i) & 1u) {
      at[i] = row_start(a.index[i], r, a.nbytes[i]);
      if (lane < P_HDR_WORDS) hdr[i] = p_load_word(a.data[i], a.nbytes[i], at[i] + 4ll * lane);
    }
  }
#pragma unroll
  for (int i = 0; i < SN; ++i)
    if (((live >> i) & 1u) && lane < P_HDR_WORDS) w[i * R_SRC_WORDS + lane] = hdr[i];
  wave_sync();
  uint32_t nw_in[SN];
#pragma unroll
  for (int i = 0; i < SN; ++i) {
    nw_in[i] = 0u;
    if ((live >> i) & 1u) nw_in[i] = scan_header(w + i * R_SRC_WORDS, w + i * R_SRC_WORDS + T_IN_WORDS, lane, len);
  }
  uint32_t plain = 0, body[SN][R_BATCH];
#pragma unroll
  for (int i = 0; i < SN; ++i) {
    if (!((live >> i) & 1u) || !row_is_plain(at[i], nw_in[i], a.nbytes[i])) continue;
    plain |= 1u << i;
    const uint32_t* row = reinterpret_cast<const uint32_t*>(a.data[i] + at[i]);
#pragma unroll
    for (int b = 0; b < R_BATCH; ++b) {
      const uint32_t k = P_HDR_WORDS + 64 * b + lane;
      body[i][b] = k < nw_in[i] ? row[k] : 0u;
    }
  }
#pragma unroll
  for (int i = 0; i < SN; ++i) {
    if (!((live >> i) & 1u)) continue;
    uint32_t* st_in = w + i * R_SRC_WORDS;
    const bool pl = (plain >> i) & 1u;
    if (pl) {
#pragma unroll
      for (int b = 0; b < R_BATCH; ++b) {
        const uint32_t k = P_HDR_WORDS + 64 * b + lane;
        if (k < nw_in[i]) st_in[k] = body[i][b];
      }
    }
    stage_body(st_in, a.data[i], a.nbytes[i], at[i], pl, P_HDR_WORDS + (pl ? 64 * R_BATCH : 0), nw_in[i], lane);
  }

  // ---- per output: the sum of what it hears, its s0, then the pack
#pragma unroll 1
  for (int o = 0; o < a.outputs_n; ++o) {
    const uint32_t hears = a.heard[o] & live;
    wave_sync();   // (the output before is done with the slot, the extremes and the flags; the staged rows are written)
    for (int k = lane; k < (a.out.row_bytes >> 2); k += 64) st_out[k] = 0u;
    kxs[lane] = INT_MIN;
    kns[lane] = INT_MAX;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    int s0 = INT_MIN;   // band `lane`: the largest gained sf of a heard source that stores it
    bool bad = false;   // ... or a heard source holds it with sf = -128
#pragma unroll 1
    for (int src = 0; src < a.sources_n; ++src) {
      if (!((hears >> src) & 1u)) continue;   // (wave-uniform)
      const uint32_t* st_in = w + src * R_SRC_WORDS;
      wave_sync();   // (the source before is done with nz)
      nz[lane] = 0u;
      wave_sync();
      x_add_source(st_in, st_in + T_IN_WORDS, bw, a.gain[o * a.sources_n + src], nz, lane, acc, s0, bad);
    }
    wave_sync();
    const size_t slot0 = (size_t)o * (size_t)a.rows;
    PackOut po;
    po.data = a.out.data + slot0 * (size_t)a.out.row_bytes;
    po.fits = a.out.fits + slot0;
    po.row_bytes = a.out.row_bytes;
    x_pack_sum(acc, bw, s0, bad, first, len, lane, st_out, rec_out, kxs, kns, po, a.offset ? a.offset + slot0 : nullptr, r,
               a.row_bits);
  }
}

}  // namespace
}  // namespace ac
