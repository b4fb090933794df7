// Packed rows of several sources to one packed row at the plan's budget in one launch (k_mix_p, defined in ac_mix.hip on mix_row
// below), on the shared steps of ac_rows_dev.h: the sibling of k_transrate_p that reads S rows where that
// one reads one.  One wave owns one output row; a tail wave simply exits.
//
// What this kernel adds, per active source, in source order, behind the parse (x_add_source):
//   sum      g = -128 for a stored sf of -128, else clamp(sf + gain, -127, 127); x = dequant(code, g) -- the exact product of
//            ac_quant_dev.h, kept apart from the add -- and acc += x in 16 float32 registers.  A code of 0 adds +0, whatever
//            its band; a band with sf = -128 adds NaN.  A non-zero code flags its band in LDS, so that lane j folds band j's
//            s0: bad where any source's sf is -128, else the largest g over the sources that flagged it.
// Then x_pack_sum, which k_route_p runs per output too: the band extremes of the sum through ordered keys, band j's meta word
// from s0 (not from a threshold), the search and the pack, codes by qcode on the sum.  The bytes are those of the composition:
// ac_unpack and ac_dequantize per source, float32 adds in source order, ac_quantize_budget at kmin 0 under thr = crit(s0), rows
// longer than the slot marked, ac_pack.
#pragma once
#include "ac_rows_dev.h"

namespace ac {
namespace {

constexpr int X_WAVE_WORDS = T_IN_WORDS + T_OUT_WORDS + 5 * P_M;   // staged input, staged slot, records in, records out, flags, kx, kn
static_assert(T_WAVES * X_WAVE_WORDS * 4 <= 65536, "a workgroup's slices fit LDS");

struct MixArgs {
  const uint8_t* data[AC_MIX_MAX_SOURCES];
  int64_t nbytes[AC_MIX_MAX_SOURCES];
  const int64_t* index[AC_MIX_MAX_SOURCES];   // [rows] each
  int gain[AC_MIX_MAX_SOURCES];               // scale-factor units, in [-254, 254]
  const uint8_t* active;                      // [S][rows] or null: every row is read
  int sources_n;
  const uint32_t* band32;                     // as PackedRows'
  const int32_t* off;
  PackOut out;                                // data [rows row_bytes], fits [rows], row_bytes
  int16_t* offset;                            // [rows] or null
  long long rows;
  int row_bits;                               // the budget R
};

// the scale factor a source's band is dequantised with (section 8h rule 1); -128 stays: dequant gives NaN
__device__ __forceinline__ int x_gained(int sf, int gain) { return sf == -128 ? -128 : max(-127, min(127, sf + gain)); }

// one staged source row (nz: the band flags, zero) into the sum: the lane's 16 codes at their bands' gained steps into acc,
// the bands that hold a non-zero code into nz, then band `lane`'s s0 / bad
__device__ __forceinline__ void x_add_source(const uint32_t* st_in, const uint32_t* rec_in, const uint32_t (&bw)[8], int gain,
                                             uint32_t* nz, int lane, float (&acc)[16], int& s0, bool& bad) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint32_t cw, sfs;
    extract_pair(st_in, rec_in, bw[i], cw, sfs);
    const int q0 = (int)(int16_t)(cw & 0xffffu), q1 = (int)(int16_t)(cw >> 16);
    const float x0 = opaque(dequant(q0, x_gained((int)(int8_t)(sfs & 0xffu), gain)));
    const float x1 = opaque(dequant(q1, x_gained((int)(int8_t)((sfs >> 16) & 0xffu), gain)));
    acc[2 * i] = acc[2 * i] + x0;
    acc[2 * i + 1] = acc[2 * i + 1] + x1;
    if (q0) atomicOr(&nz[bw[i] & 63u], 1u);
    if (q1) atomicOr(&nz[(bw[i] >> 6) & 63u], 1u);
  }
  wave_sync();
  const int s_in = rec_sf(rec_in[lane]);
  if (s_in == -128) bad = true;
  else if (nz[lane]) s0 = max(s0, x_gained(s_in, gain));
}

// the sum acc of the lane's 16 bins, band `lane`'s s0 / bad -> the band extremes, the search at row_bits, the pack through
// st_out (zero; kxs / kns at INT_MIN / INT_MAX) and the stores of slot r of out, fits[r] and offset[r]
__device__ __forceinline__ void x_pack_sum(const float (&acc)[16], const uint32_t (&bw)[8], int s0, bool bad, uint32_t first,
                                           uint32_t len, int lane, uint32_t* st_out, int* rec_out, int* kxs, int* kns,
                                           const PackOut& out, int16_t* offset, long long r, int row_bits) {
  const int nw_out = out.row_bytes >> 2;
#pragma unroll
  for (int i = 0; i < 8; ++i) fold_extremes(kxs, kns, bw[i], ordered_key(acc[2 * i]), ordered_key(acc[2 * i + 1]));
  wave_sync();
  const int sb = s0 == INT_MIN ? 0 : s0;   // nothing stored: the band comes out with width 0
  const int meta = len == 0 ? 0 : bad ? -1 : (int)(len << 8) | (sb & 0xff);
  const int kx = kxs[lane], kn = kns[lane];
  const int lo = search_offset(meta, kx, kn, row_bits);
  const bool fits = pack_header(st_out, rec_out, meta, kx, kn, lo, first, len, nw_out, lane);
#pragma unroll
  for (int i = 0; i < 8; ++i)
    code_fields(st_out, rec_out[bw[i] & 63u], rec_out[(bw[i] >> 6) & 63u], acc[2 * i], acc[2 * i + 1],
                (uint32_t)(128 * i + 2 * lane));
  store_slot(reinterpret_cast<uint32_t*>(out.data + (size_t)r * (size_t)out.row_bytes), st_out, nw_out, lane);
  store_fits(fits, lo, out.fits, offset, r, lane);
}

// rows r of the sources -> slot r of a.out; w: the wave's slice of LDS (X_WAVE_WORDS words)
__device__ __forceinline__ void mix_row(const MixArgs& a, long long r, int lane, uint32_t* w) {
  uint32_t* st_in = w;
  uint32_t* st_out = w + T_IN_WORDS;
  uint32_t* rec_in = st_out + T_OUT_WORDS;
  int* rec_out = reinterpret_cast<int*>(rec_in + P_M);
  uint32_t* nz = reinterpret_cast<uint32_t*>(rec_out + P_M);
  int* kxs = reinterpret_cast<int*>(nz + P_M);
  int* kns = kxs + P_M;

  for (int k = lane; k < (a.out.row_bytes >> 2); k += 64) st_out[k] = 0u;
  kxs[lane] = INT_MIN;
  kns[lane] = INT_MAX;
  const uint32_t first = (uint32_t)a.off[lane];
  const uint32_t len = (uint32_t)a.off[lane + 1] - first;   // bins of the lane's band
  PackedRows pr;
  pr.band32 = a.band32;
  pr.off = a.off;
  uint32_t bw[8];
  load_bw_p<8>(pr, lane, bw);

  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  int s0 = INT_MIN;   // band `lane`: the largest gained sf of a source that stores it
  bool bad = false;   // ... or a source holds it with sf = -128

#pragma unroll 1
  for (int src = 0; src < a.sources_n; ++src) {
    if (a.active && a.active[(size_t)src * (size_t)a.rows + (size_t)r] == 0) continue;   // (wave-uniform) never read
    const uint8_t* data = a.data[src];
    const int64_t nbytes = a.nbytes[src];
    const int64_t at = row_start(a.index[src], r, nbytes);
    wave_sync();   // (the source before is done with st_in, rec_in and nz)
    stage_header(st_in, data, nbytes, at, lane);
    nz[lane] = 0u;
    stage_row(st_in, rec_in, data, nbytes, at, len, lane);
    x_add_source(st_in, rec_in, bw, a.gain[src], nz, lane, acc, s0, bad);
  }
  x_pack_sum(acc, bw, s0, bad, first, len, lane, st_out, rec_out, kxs, kns, a.out, a.offset, r, a.row_bits);
}

}  // namespace
}  // namespace ac
