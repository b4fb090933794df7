// Packed rows to packed rows at a lower budget in one launch (k_transrate_p, defined in ac_transrate.hip on transrate_row below;
// DESIGN.md section 8e): filters_n = 1024 with bark_bands_n = 64, so a row has as many bands as a wave has lanes.  One wave owns one
// row and lane j holds band j; rows are independent, so no wave waits for another and a tail wave simply exits.
//
// Per row, on the pieces of the two fused kernels that read and write packed rows:
//   parse    as parse_strip_p (ac_fast_inv_p_dev.h): the 26 header words staged through p_load_word, lane j reads band j's
//            width (17 .. 30 -> 31), one wave-wide scan of (stored << 16) | w len gives its sf field and first code bit; the
//            band's record (first code bit << 13 | sf byte << 5 | width) goes to LDS.  The scan's total is the row's length,
//            so the rest of the row is staged next: plain dword loads where every word lies inside data at a 4-byte phase,
//            p_load_word's clamped loads for any other row.
//   extract  as extract_sig_p: bins 2q and 2q + 1 are neighbouring fields; shift, mask, un-zigzag.  The 16 codes of a lane
//            stay in 8 registers; each band's largest and smallest code are folded into its LDS slot (ds_max / ds_min).
//   search   lane j forms band j's meta word from the stored sf and the ordered keys of dequant(qmax, sf), dequant(qmin, sf)
//            (fp32(q step) is monotone in q), then the bisection of [0, 254] with band_bits and wave_sum (ac_rate_dev.h):
//            every value of it is wave-uniform, the control flow scalar.
//   pack     as PackStage (ac_fast_fwd_qp_dev.h): widths at the offset (band_width_at), one exclusive scan, fits from lane
//            63's inclusive sum before any field is ORed in -- a row that does not fit turns every width into 31, so nothing
//            is written past the 8 row_bytes staged bits -- then widths, scale factors and the code fields, requantised by
//            qcode on dequant(q, stored sf), into the staged row, a lane's two bins as one field of at most 32 bits.  The
//            wave stores row_bytes / 4 dwords; lane 0 the fits byte and, where asked, the offset.
// The bytes are those of ac_unpack, k_requantize_budget at kmin 0, rows longer than the slot marked, ac_pack at r row_bytes
// into zero-filled data.
#pragma once
#include "ac_fast_inv_dev.h"
#include "ac_fast_fwd_qp_dev.h"

namespace ac {
namespace {

constexpr int T_WAVES = 4;                                   // rows per workgroup
constexpr int T_IN_BITS = 16 * 1024 + 13 * P_M;              // the longest row that can be read: every band at width 16
constexpr int T_IN_WORDS = (T_IN_BITS + 31) / 32 + 6;        // ... staged, and the second word of a window at its end
constexpr int T_OUT_WORDS = kPackRowsMaxBits / 32;           // the staged output slot
constexpr int T_WAVE_WORDS = T_IN_WORDS + T_OUT_WORDS + 4 * P_M;   // + input records, output records, qmax, qmin
static_assert(T_IN_WORDS % 4 == 0 && T_WAVES * T_WAVE_WORDS * 4 <= 65536, "a workgroup's slices fit LDS");

struct TransArgs {
  PackedRows in;       // data, nbytes, index [rows], band32, off
  PackOut out;         // data [rows row_bytes], fits [rows], row_bytes
  int16_t* offset;     // [rows] or null
  long long rows;
  int row_bits;        // the target budget R'
};

// the stored scale factor of a band record: -128 for width 31, 0 for width 0 (parse wrote the byte that way)
__device__ __forceinline__ int t_rec_sf(uint32_t rec) { return (int)(int8_t)((rec >> 5) & 0xffu); }

// the codes of bins i and i + 1 (output records re, ro of their bands) into the staged row: PackStage::code_fields
__device__ __forceinline__ void t_code_fields(uint32_t* st, int re, int ro, float xe, float xo, uint32_t i) {
  const uint32_t we = (uint32_t)re & 31u, wo = (uint32_t)ro & 31u;
  const uint32_t ee = qp_stores(we) ? we : 0u, eo = qp_stores(wo) ? wo : 0u;
  const uint32_t ze = ee ? zigzag(qcode(xe, quant_inv_step((int)(int8_t)((uint32_t)re >> 5)))) : 0u;
  const uint32_t zo = eo ? zigzag(qcode(xo, quant_inv_step((int)(int8_t)((uint32_t)ro >> 5)))) : 0u;
  // bin i + 1 follows bin i: in the same band, or first of the next one that holds bins
  const uint32_t p = (uint32_t)((re >> 13) + (int)(ee * i));
  qp_put(st, p, ze | (zo << ee));
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

  // ---- parse: the header, the band records, then the rest of the row
  int64_t at = pr.index[r];
  // a row start beyond the buffer reads nothing; clamping it keeps start + 4 k from overflowing
  at = at > pr.nbytes ? pr.nbytes : (at < -(1ll << 40) ? -(1ll << 40) : at);
  if (lane < P_HDR_WORDS) st_in[lane] = p_load_word(pr.data, pr.nbytes, at + 4ll * lane);
  for (int k = lane; k < nw_out; k += 64) st_out[k] = 0u;
  qmx[lane] = INT_MIN;
  qmn[lane] = INT_MAX;
  wave_sync();
  const uint32_t first = (uint32_t)pr.off[lane];
  const uint32_t len = (uint32_t)pr.off[lane + 1] - first;   // bins of the lane's band
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

  // ---- extract: the lane's 16 codes, and every band's largest and smallest
  uint32_t bw[8], cw[8];
  load_bw_p<8>(pr, lane, bw);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t j0 = bw[i] & 63u, j1 = (bw[i] >> 6) & 63u;
    const uint32_t wi = p_pos(rec_in[j0], bw[i] >> 12) >> 5;   // < T_IN_WORDS - 1: a field starts inside the longest row
    uint32_t sfs;
    extract_sig_p(rec_in, bw[i], st_in[wi], st_in[wi + 1], cw[i], sfs);
    const int q0 = (int)(int16_t)(cw[i] & 0xffffu), q1 = (int)(int16_t)(cw[i] >> 16);
    if (j0 == j1) {
      atomicMax(&qmx[j0], max(q0, q1));
      atomicMin(&qmn[j0], min(q0, q1));
    } else {
      atomicMax(&qmx[j0], q0);
      atomicMin(&qmn[j0], q0);
      atomicMax(&qmx[j1], q1);
      atomicMin(&qmn[j1], q1);
    }
  }
  wave_sync();

  // ---- search: band `lane`'s meta word and extremes, the smallest offset whose row meets the budget
  const int s_in = t_rec_sf(rec_in[lane]);
  const int meta = len == 0 ? 0 : s_in == -128 ? -1 : (int)(len << 8) | (s_in & 0xff);
  const int kx = ordered_key(dequant(qmx[lane], s_in)), kn = ordered_key(dequant(qmn[lane], s_in));
  int lo = 0, hi = kRateMaxOffset;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int bits = __builtin_amdgcn_readfirstlane(5 * P_M + wave_sum(band_bits(meta, kx, kn, mid)));
    if (bits <= a.row_bits) hi = mid;
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
    const float x0 = dequant((int)(int16_t)(cw[i] & 0xffffu), t_rec_sf(rec_in[j0]));
    const float x1 = dequant((int)(int16_t)(cw[i] >> 16), t_rec_sf(rec_in[j1]));
    t_code_fields(st_out, rec_out[j0], rec_out[j1], x0, x1, (uint32_t)(128 * i + 2 * lane));
  }
  wave_sync();
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.out.data + (size_t)r * (size_t)a.out.row_bytes);
  for (int k = lane; k < nw_out; k += 64) dst[k] = st_out[k];
  if (lane == 0) {
    a.out.fits[r] = fits ? 1 : 0;
    if (a.offset) a.offset[r] = (int16_t)lo;
  }
}

}  // namespace
}  // namespace ac
