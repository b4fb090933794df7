// Packed rows to packed rows at a lower budget in one launch (k_transrate_p, defined in ac_transrate.hip on transrate_row below;
// DESIGN.md section 8e), on the shared steps of ac_rows_dev.h.  Rows are independent, so no wave waits for another and a tail
// wave simply exits.
//
// What this kernel adds to the parse and the pack: the search runs on the codes themselves.  The 16 codes of a lane stay in 8
// registers and each band's largest and smallest code are folded in LDS; lane j forms band j's meta word from the stored sf and
// the ordered keys of dequant(qmax, sf), dequant(qmin, sf) (fp32(q step) is monotone in q); the fields are requantised on
// dequant(q, stored sf).  The bytes are those of ac_unpack, k_requantize_budget at kmin 0, rows longer than the slot marked,
// ac_pack at r row_bytes into zero-filled data.
#pragma once
#include "ac_rows_dev.h"

namespace ac {
namespace {

// a wave's slice: staged input, staged slot, input records, output records, qmax, qmin
constexpr int T_WAVE_WORDS = T_IN_WORDS + T_OUT_WORDS + 4 * P_M;
static_assert(T_WAVES * T_WAVE_WORDS * 4 <= 65536, "a workgroup's slices fit LDS");

struct TransArgs {
  PackedRows in;       // data, nbytes, index [rows], band32, off
  PackOut out;         // data [rows row_bytes], fits [rows], row_bytes
  int16_t* offset;     // [rows] or null
  long long rows;
  int row_bits;        // the target budget R'
};

// the lane's 16 codes of the staged row into cw, every band's largest and smallest through qmx / qmn (at INT_MIN / INT_MAX);
// band `lane`'s (len bins) meta word and the ordered keys of its extremes
__device__ __forceinline__ void t_code_stats(const uint32_t* st_in, const uint32_t* rec_in, const uint32_t (&bw)[8], int* qmx,
                                             int* qmn, uint32_t len, int lane, uint32_t (&cw)[8], int& meta, int& kx, int& kn) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint32_t sfs;
    extract_pair(st_in, rec_in, bw[i], cw[i], sfs);
    fold_extremes(qmx, qmn, bw[i], (int)(int16_t)(cw[i] & 0xffffu), (int)(int16_t)(cw[i] >> 16));
  }
  wave_sync();
  const int s_in = rec_sf(rec_in[lane]);
  meta = len == 0 ? 0 : s_in == -128 ? -1 : (int)(len << 8) | (s_in & 0xff);
  kx = ordered_key(dequant(qmx[lane], s_in));
  kn = ordered_key(dequant(qmn[lane], s_in));
}

// the search at `budget` bits and the pack of the codes cw into nw_out words at dst, through st_out (zero) and rec_out;
// returns (offset << 1) | fits in every lane
__device__ __forceinline__ int t_repack(const uint32_t (&bw)[8], const uint32_t (&cw)[8], const uint32_t* rec_in, int* rec_out,
                                        uint32_t* st_out, int meta, int kx, int kn, uint32_t first, uint32_t len, int budget,
                                        int nw_out, uint32_t* dst, int lane) {
  const int lo = search_offset(meta, kx, kn, budget);
  const bool fits = pack_header(st_out, rec_out, meta, kx, kn, lo, first, len, nw_out, lane);
  // (a pair's values are formed where they are packed: all 16 ahead of the fields cost 5 us a launch)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t j0 = bw[i] & 63u, j1 = (bw[i] >> 6) & 63u;
    const float x0 = dequant((int)(int16_t)(cw[i] & 0xffffu), rec_sf(rec_in[j0]));
    const float x1 = dequant((int)(int16_t)(cw[i] >> 16), rec_sf(rec_in[j1]));
    code_fields(st_out, rec_out[j0], rec_out[j1], x0, x1, (uint32_t)(128 * i + 2 * lane));
  }
  store_slot(dst, st_out, nw_out, lane);
  return (lo << 1) | (fits ? 1 : 0);
}

// row r of a.in -> slot r of a.out; w: the wave's slice of LDS (T_WAVE_WORDS words)
__device__ __forceinline__ void transrate_row(const TransArgs& a, long long r, int lane, uint32_t* w) {
  uint32_t* st_in = w;
  uint32_t* st_out = w + T_IN_WORDS;
  uint32_t* rec_in = st_out + T_OUT_WORDS;
  int* rec_out = reinterpret_cast<int*>(rec_in + P_M);
  int* qmx = rec_out + P_M;
  int* qmn = qmx + P_M;
  const PackedRows& pr = a.in;
  const int nw_out = a.out.row_bytes >> 2;

  const int64_t at = row_start(pr.index, r, pr.nbytes);
  stage_header(st_in, pr.data, pr.nbytes, at, lane);
  for (int k = lane; k < nw_out; k += 64) st_out[k] = 0u;
  qmx[lane] = INT_MIN;
  qmn[lane] = INT_MAX;
  const uint32_t first = (uint32_t)pr.off[lane];
  const uint32_t len = (uint32_t)pr.off[lane + 1] - first;   // bins of the lane's band
  stage_row(st_in, rec_in, pr.data, pr.nbytes, at, len, lane);

  uint32_t bw[8], cw[8];
  int meta, kx, kn;
  load_bw_p<8>(pr, lane, bw);
  t_code_stats(st_in, rec_in, bw, qmx, qmn, len, lane, cw, meta, kx, kn);
  const int p = t_repack(bw, cw, rec_in, rec_out, st_out, meta, kx, kn, first, len, a.row_bits, nw_out,
                         reinterpret_cast<uint32_t*>(a.out.data + (size_t)r * (size_t)a.out.row_bytes), lane);
  store_fits(p & 1, p >> 1, a.out.fits, a.offset, r, lane);
}

}  // namespace
}  // namespace ac
