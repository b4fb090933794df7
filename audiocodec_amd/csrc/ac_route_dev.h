// Packed rows of S sources to the packed rows of O mixes at the plan's budget in one launch (k_route_p, defined in ac_route.hip on
// route_row below): k_mix_p's sibling (ac_mix_dev.h) for a bridge, which stages every source row once and
// packs O rows from it.  filters_n = 1024 with bark_bands_n = 64; one wave owns one row position r and lane j holds band j; a
// tail wave simply exits.  Output o is, byte for byte, mix_row's on the sources it hears, in source order, at its gains.
//
//   stage    every source that is active at r and heard by at least one output, into its own slice of LDS, with mix_row's parse:
//            the 26 header words of ALL such sources are loaded before the first scan, and the first 128 body words of every
//            plain row before the first of them is written to LDS, so the wave waits for memory twice, not 2 S times.  Rows that
//            are off phase, negative or past the end take p_load_word's clamped loads, a row longer than 154 words its further
//            words in a loop.  An inactive or unheard row is never read.
//   output   o = 0 .. O-1 in order: 16 float32 accumulators, band `lane`'s s0 / bad and the non-zero band flags start afresh;
//            over the heard staged sources in source order mix_row's extract and sum at x_gained(sf, gain[o][i]); then
//            r_pack_sum (mix_row's tail) into slot r of output o, fits[o][r] and offset[o][r].
// Gains and mutes are kernel arguments, wave-uniform.  The waves of a workgroup share nothing: no workgroup barrier.
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

// mix_row's scan of a staged header: band `lane`'s record into rec_in; returns the row's length in words
__device__ __forceinline__ uint32_t r_scan(const uint32_t* st_in, uint32_t* rec_in, int lane, uint32_t len) {
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
  return (cbase + (total & 0xffffu) + 31u) >> 5;   // <= (T_IN_BITS + 31) / 32 whatever the widths say
}

// mix_row's tail, word for word, run per output: the sum acc of the lane's 16 bins, band `lane`'s s0 / bad
// -> the band extremes, the search at row_bits, the pack into st_out (zeroed; kxs / kns at INT_MIN / INT_MAX) and the stores
// of slot r of out, fits[r] and offset[r]
__device__ __forceinline__ void r_pack_sum(const float (&acc)[16], const uint32_t (&bw)[8], int s0, bool bad, uint32_t first,
                                           uint32_t len, int lane, uint32_t* st_out, int* rec_out, int* kxs, int* kns,
                                           const PackOut& out, int16_t* offset, long long r, int row_bits) {
  const int nw_out = out.row_bytes >> 2;
  // ---- the band extremes of the sum
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t j0 = bw[i] & 63u, j1 = (bw[i] >> 6) & 63u;
    const int k0 = ordered_key(acc[2 * i]), k1 = ordered_key(acc[2 * i + 1]);
    if (j0 == j1) {
      atomicMax(&kxs[j0], max(k0, k1));
      atomicMin(&kns[j0], min(k0, k1));
    } else {
      atomicMax(&kxs[j0], k0);
      atomicMin(&kns[j0], k0);
      atomicMax(&kxs[j1], k1);
      atomicMin(&kns[j1], k1);
    }
  }
  wave_sync();

  // ---- search: band `lane`'s meta word from s0, the smallest offset whose row meets the budget
  const int sb = s0 == INT_MIN ? 0 : s0;   // nothing stored: the band comes out with width 0
  const int meta = len == 0 ? 0 : bad ? -1 : (int)(len << 8) | (sb & 0xff);
  const int kx = kxs[lane], kn = kns[lane];
  int lo = 0, hi = kRateMaxOffset;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int bits = __builtin_amdgcn_readfirstlane(5 * P_M + wave_sum(band_bits(meta, kx, kn, mid)));
    if (bits <= row_bits) hi = mid;
    else lo = mid + 1;
  }

  // ---- pack: widths, positions and fits, then the fields
  bool fits;
  {
    const int s = band_sf(meta, lo);
    uint32_t wd = band_width_at(meta, kx, kn, s);
    const uint32_t v = qp_stores(wd) ? (1u << 16) | (wd * len) : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += up;
    }
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    const uint32_t cbase = 5u * P_M + 8u * (total >> 16);   // first code bit
    fits = cbase + (total & 0xffffu) <= 32u * (uint32_t)nw_out;
    uint32_t ex = incl - v;
    if (!fits) {   // the marked row
      wd = 31u;
      ex = 0u;
    }
    const uint32_t e = qp_stores(wd) ? wd : 0u;
    qp_put(st_out, 5u * (uint32_t)lane, wd);
    if (e) qp_put(st_out, 5u * P_M + 8u * (ex >> 16), (uint32_t)(uint8_t)s);
    const int base = (int)(cbase + (ex & 0xffffu)) - (int)(e * first);
    rec_out[lane] = (int)(((uint32_t)base << 13) | ((uint32_t)(uint8_t)s << 5) | wd);
  }
  wave_sync();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t j0 = bw[i] & 63u, j1 = (bw[i] >> 6) & 63u;
    t_code_fields(st_out, rec_out[j0], rec_out[j1], acc[2 * i], acc[2 * i + 1], (uint32_t)(128 * i + 2 * lane));
  }
  wave_sync();
  uint32_t* dst = reinterpret_cast<uint32_t*>(out.data + (size_t)r * (size_t)out.row_bytes);
  for (int k = lane; k < nw_out; k += 64) dst[k] = st_out[k];
  if (lane == 0) {
    out.fits[r] = fits ? 1 : 0;
    if (offset) offset[r] = (int16_t)lo;
  }
}

// rows r of the sources -> slot r of every output; w: the wave's slice of LDS (r_wave_words(a.sources_n) words)
__device__ __forceinline__ void route_row(const RouteArgs& a, long long r, int lane, uint32_t* w) {
  constexpr int SN = AC_ROUTE_MAX_SOURCES;
  uint32_t* st_out = w + a.sources_n * R_SRC_WORDS;
  int* rec_out = reinterpret_cast<int*>(st_out + T_OUT_WORDS);
  uint32_t* nz = reinterpret_cast<uint32_t*>(rec_out + P_M);
  int* kxs = reinterpret_cast<int*>(nz + P_M);
  int* kns = kxs + P_M;
  const int nw_out = a.out.row_bytes >> 2;
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
      const int64_t nbytes = a.nbytes[i], v = a.index[i][r];
      // a row start beyond the buffer reads nothing; clamping it keeps start + 4 k from overflowing
      at[i] = v > nbytes ? nbytes : (v < -(1ll << 40) ? -(1ll << 40) : v);
      if (lane < P_HDR_WORDS) hdr[i] = p_load_word(a.data[i], nbytes, at[i] + 4ll * lane);
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
    if ((live >> i) & 1u) nw_in[i] = r_scan(w + i * R_SRC_WORDS, w + i * R_SRC_WORDS + T_IN_WORDS, lane, len);
  }
  // (words behind a row's last are never staged: a window's second word may read what LDS held there, and is masked off)
  uint32_t plain = 0, body[SN][R_BATCH];
#pragma unroll
  for (int i = 0; i < SN; ++i) {
    if (!((live >> i) & 1u)) continue;
    if (at[i] >= 0 && (at[i] & 3) == 0 && at[i] + 4ll * nw_in[i] <= a.nbytes[i]) {
      plain |= 1u << i;
      const uint32_t* row = reinterpret_cast<const uint32_t*>(a.data[i] + at[i]);
#pragma unroll
      for (int b = 0; b < R_BATCH; ++b) {
        const uint32_t k = P_HDR_WORDS + 64 * b + lane;
        body[i][b] = k < nw_in[i] ? row[k] : 0u;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < SN; ++i) {
    if (!((live >> i) & 1u)) continue;
    uint32_t* st_in = w + i * R_SRC_WORDS;
    if ((plain >> i) & 1u) {
      const uint32_t* row = reinterpret_cast<const uint32_t*>(a.data[i] + at[i]);
#pragma unroll
      for (int b = 0; b < R_BATCH; ++b) {
        const uint32_t k = P_HDR_WORDS + 64 * b + lane;
        if (k < nw_in[i]) st_in[k] = body[i][b];
      }
      for (uint32_t k = P_HDR_WORDS + 64 * R_BATCH + lane; k < nw_in[i]; k += 64) st_in[k] = row[k];
    } else {
      for (uint32_t k = P_HDR_WORDS + lane; k < nw_in[i]; k += 64) st_in[k] = p_load_word(a.data[i], a.nbytes[i], at[i] + 4ll * k);
    }
  }

  // ---- per output: the sum of what it hears, its s0, then mix_row's tail
#pragma unroll 1
  for (int o = 0; o < a.outputs_n; ++o) {
    const uint32_t hears = a.heard[o] & live;
    wave_sync();   // (the output before is done with the slot, the extremes and the flags; the staged rows are written)
    for (int k = lane; k < nw_out; k += 64) st_out[k] = 0u;
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
      const uint32_t* rec_in = st_in + T_IN_WORDS;
      const int gain = a.gain[o * a.sources_n + src];
      wave_sync();   // (the source before is done with nz)
      nz[lane] = 0u;
      wave_sync();
      // extract and sum: the lane's 16 codes at their bands' gained steps into acc; the bands that hold a non-zero code
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t j0 = bw[i] & 63u, j1 = (bw[i] >> 6) & 63u;
        const uint32_t wi = p_pos(rec_in[j0], bw[i] >> 12) >> 5;   // < T_IN_WORDS - 1: a field starts inside the longest row
        uint32_t cw, sfs;
        extract_sig_p(rec_in, bw[i], st_in[wi], st_in[wi + 1], cw, sfs);
        const int q0 = (int)(int16_t)(cw & 0xffffu), q1 = (int)(int16_t)(cw >> 16);
        const float x0 = x_opaque(dequant(q0, x_gained((int)(int8_t)(sfs & 0xffu), gain)));
        const float x1 = x_opaque(dequant(q1, x_gained((int)(int8_t)((sfs >> 16) & 0xffu), gain)));
        acc[2 * i] = acc[2 * i] + x0;
        acc[2 * i + 1] = acc[2 * i + 1] + x1;
        if (q0) atomicOr(&nz[j0], 1u);
        if (q1) atomicOr(&nz[j1], 1u);
      }
      wave_sync();
      const int s_in = t_rec_sf(rec_in[lane]);
      if (s_in == -128) bad = true;
      else if (nz[lane]) s0 = max(s0, x_gained(s_in, gain));
    }
    wave_sync();
    const size_t slot0 = (size_t)o * (size_t)a.rows;
    PackOut po;
    po.data = a.out.data + slot0 * (size_t)a.out.row_bytes;
    po.fits = a.out.fits + slot0;
    po.row_bytes = a.out.row_bytes;
    r_pack_sum(acc, bw, s0, bad, first, len, lane, st_out, rec_out, kxs, kns, po, a.offset ? a.offset + slot0 : nullptr, r,
               a.row_bits);
  }
}

}  // namespace
}  // namespace ac
