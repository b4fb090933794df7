// The steps shared by the kernels that work on packed rows without decoding them -- k_transrate_p, k_protect_p / k_protect_ps,
// k_mix_p, k_route_p, k_level_p (DESIGN.md sections 8e, 8g - 8j) -- each written once.  filters_n = 1024 with bark_bands_n = 64,
// so a row has as many bands as a wave has lanes: one wave owns one row, lane j holds band j, and the lanes talk through the
// wave's own slice of LDS (wave_sync, no workgroup barrier).
//
//   parse    as parse_strip_p (ac_fast_inv_p_dev.h): the row start clamped (row_start), the 26 header words through p_load_word
//            (stage_header), then scan_header: lane j reads band j's width (17 .. 30 -> 31), one wave-wide scan of
//            (stored << 16) | w len gives its sf field and first code bit; the band's record (first code bit << 13 | sf byte << 5
//            | width) goes to LDS.  The scan's total is the row's length, so the rest of the row is staged next (stage_body):
//            plain dword loads where every word lies inside data at a 4-byte phase, p_load_word's clamped loads for any other
//            row.  stage_row is the three behind a staged header, between the kernel's own LDS initialisation and the extract.
//   extract  extract_pair, as extract_sig_p: bins 2q and 2q + 1 are neighbouring fields; shift, mask, un-zigzag.
//            fold_extremes: a pair's two values into their bands' largest and smallest in LDS (ds_max / ds_min).
//   search   search_offset: the bisection of [0, 254] with band_bits and wave_sum (ac_rate_dev.h) on band j's meta word and
//            extreme keys: every value of it is wave-uniform, the control flow scalar.
//   pack     as PackStage (ac_fast_fwd_qp_dev.h).  pack_header: widths at the offset (band_width_at), one exclusive scan, fits
//            from lane 63's inclusive sum before any field is ORed in -- a row that does not fit turns every width into 31, so
//            nothing is written past the staged slot -- then widths, scale factors and the output records.  code_fields: a
//            lane's two neighbouring bins, requantised by qcode, as one field of at most 32 bits.  store_slot: the wave's store
//            of row_bytes / 4 dwords.  store_fits: lane 0's fits byte and, where asked, the offset.
// plan_rows and row_groups at the top are host code: what the launchers of these kernels (ac_transrate.hip, ac_protect.hip,
// ac_protect_s.hip, ac_mix.hip, ac_route.hip, ac_level.hip) fill and refuse the same way.
#pragma once
#include "ac_fast_inv_dev.h"
#include "ac_fast_fwd_qp_dev.h"

namespace ac {
namespace {

constexpr int T_WAVES = 4;                                   // rows per workgroup
constexpr int T_IN_BITS = 16 * 1024 + 13 * P_M;              // the longest row that can be read: every band at width 16
constexpr int T_IN_WORDS = (T_IN_BITS + 31) / 32 + 6;        // ... staged, and the second word of a window at its end
constexpr int T_OUT_WORDS = kPackRowsMaxBits / 32;           // the staged output slot
static_assert(T_IN_WORDS % 4 == 0, "the slices behind a staged row keep its phase");

// ---- host: what every launcher of these kernels fills and refuses the same way

// the rows of a buffer under the plan's band layout
inline PackedRows plan_rows(const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes, const int64_t* index) {
  PackedRows pr;
  pr.data = data;
  pr.nbytes = nbytes;
  pr.index = index;
  pr.band32 = reinterpret_cast<const uint32_t*>(psy->d_qband);
  pr.off = psy->d_qoff;
  return pr;
}

// *groups: workgroups of `waves` rows each (rows >= 0); false, with the error set, where one launch cannot hold them
inline bool row_groups(long long rows, int waves, long long* groups) {
  *groups = (rows + waves - 1) / waves;
  if (*groups <= 2147483647ll) return true;
  set_error("problem too large for one launch (%lld rows)", rows);
  return false;
}

// ---- parse

// a row start beyond the buffer reads nothing; clamping it keeps start + 4 k from overflowing
__device__ __forceinline__ int64_t row_start(const int64_t* index, long long r, int64_t nbytes) {
  const int64_t at = index[r];
  return at > nbytes ? nbytes : (at < -(1ll << 40) ? -(1ll << 40) : at);
}

__device__ __forceinline__ void stage_header(uint32_t* st_in, const uint8_t* data, int64_t nbytes, int64_t at, int lane) {
  if (lane < P_HDR_WORDS) st_in[lane] = p_load_word(data, nbytes, at + 4ll * lane);
}

// the scan of a staged header: band `lane`'s record (len bins) into rec_in; returns the row's length in words
__device__ __forceinline__ uint32_t scan_header(const uint32_t* st_in, uint32_t* rec_in, int lane, uint32_t len) {
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

// every word of the row lies inside data at a 4-byte phase
__device__ __forceinline__ bool row_is_plain(int64_t at, uint32_t nw_in, int64_t nbytes) {
  return at >= 0 && (at & 3) == 0 && at + 4ll * nw_in <= nbytes;
}

// words k0 + lane, k0 + lane + 64, ... below nw_in of the row
// (words behind the row's last are never staged: a window's second word may read what LDS held there, and is masked off)
__device__ __forceinline__ void stage_body(uint32_t* st_in, const uint8_t* data, int64_t nbytes, int64_t at, bool plain,
                                           uint32_t k0, uint32_t nw_in, int lane) {
  if (plain) {
    const uint32_t* row = reinterpret_cast<const uint32_t*>(data + at);
    for (uint32_t k = k0 + lane; k < nw_in; k += 64) st_in[k] = row[k];
  } else {
    for (uint32_t k = k0 + lane; k < nw_in; k += 64) st_in[k] = p_load_word(data, nbytes, at + 4ll * k);
  }
}

// behind stage_header and whatever LDS the kernel initialises beside it: the band records, the rest of the row
__device__ __forceinline__ void stage_row(uint32_t* st_in, uint32_t* rec_in, const uint8_t* data, int64_t nbytes, int64_t at,
                                          uint32_t len, int lane) {
  wave_sync();
  const uint32_t nw_in = scan_header(st_in, rec_in, lane, len);
  stage_body(st_in, data, nbytes, at, row_is_plain(at, nw_in, nbytes), P_HDR_WORDS, nw_in, lane);
  wave_sync();
}

// ---- extract

// the stored scale factor of a band record: -128 for width 31, 0 for width 0 (the scan wrote the byte that way)
__device__ __forceinline__ int rec_sf(uint32_t rec) { return (int)(int8_t)((rec >> 5) & 0xffu); }

// a value the compiler cannot see through: the product above it is a product, never half of a multiply-add
__device__ __forceinline__ float opaque(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// the codes of the bins of bw[i] (low, high half) and their scale-factor bytes (bits 0-7, 16-23) from the staged row
__device__ __forceinline__ void extract_pair(const uint32_t* st_in, const uint32_t* rec_in, uint32_t bwi, uint32_t& cw,
                                             uint32_t& sfs) {
  const uint32_t wi = p_pos(rec_in[bwi & 63u], bwi >> 12) >> 5;   // < T_IN_WORDS - 1: a field starts inside the longest row
  extract_sig_p(rec_in, bwi, st_in[wi], st_in[wi + 1], cw, sfs);
}

// v0, v1 of the bins of bw[i] into their bands' largest and smallest (mx at INT_MIN, mn at INT_MAX before the first)
__device__ __forceinline__ void fold_extremes(int* mx, int* mn, uint32_t bwi, int v0, int v1) {
  const uint32_t j0 = bwi & 63u, j1 = (bwi >> 6) & 63u;
  if (j0 == j1) {
    atomicMax(&mx[j0], max(v0, v1));
    atomicMin(&mn[j0], min(v0, v1));
  } else {
    atomicMax(&mx[j0], v0);
    atomicMin(&mn[j0], v0);
    atomicMax(&mx[j1], v1);
    atomicMin(&mn[j1], v1);
  }
}

// ---- search and pack

// the smallest offset whose row meets the budget; lane j holds band j's meta word and extreme keys
__device__ __forceinline__ int search_offset(int meta, int kx, int kn, int budget) {
  int lo = 0, hi = kRateMaxOffset;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int bits = __builtin_amdgcn_readfirstlane(5 * P_M + wave_sum(band_bits(meta, kx, kn, mid)));
    if (bits <= budget) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// widths, positions and fits of the row at offset k: the header fields into st_out (nw_out words, zero), band `lane`'s output
// record into rec_out; returns fits.  The sync ahead of the first field orders it behind the zeroing of st_out wherever the
// caller did that: k_protect_p zeroes between two packs, with nothing but the search in between; the others zeroed several
// syncs ago, and one more costs no instruction (wave_sync only pins the compiler's order).
__device__ __forceinline__ bool pack_header(uint32_t* st_out, int* rec_out, int meta, int kx, int kn, int k, uint32_t first,
                                            uint32_t len, int nw_out, int lane) {
  const int s = band_sf(meta, k);
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
  const bool fits = cbase + (total & 0xffffu) <= 32u * (uint32_t)nw_out;
  uint32_t ex = incl - v;
  if (!fits) {   // the marked row
    wd = 31u;
    ex = 0u;
  }
  const uint32_t e = qp_stores(wd) ? wd : 0u;
  wave_sync();
  qp_put(st_out, 5u * (uint32_t)lane, wd);
  if (e) qp_put(st_out, 5u * P_M + 8u * (ex >> 16), (uint32_t)(uint8_t)s);
  const int base = (int)(cbase + (ex & 0xffffu)) - (int)(e * first);
  rec_out[lane] = (int)(((uint32_t)base << 13) | ((uint32_t)(uint8_t)s << 5) | wd);
  wave_sync();
  return fits;
}

// the codes of bins i and i + 1 (output records re, ro of their bands) into the staged row: PackStage::code_fields
__device__ __forceinline__ void code_fields(uint32_t* st, int re, int ro, float xe, float xo, uint32_t i) {
  const uint32_t we = (uint32_t)re & 31u, wo = (uint32_t)ro & 31u;
  const uint32_t ee = qp_stores(we) ? we : 0u, eo = qp_stores(wo) ? wo : 0u;
  const uint32_t ze = ee ? zigzag(qcode(xe, quant_inv_step((int)(int8_t)((uint32_t)re >> 5)))) : 0u;
  const uint32_t zo = eo ? zigzag(qcode(xo, quant_inv_step((int)(int8_t)((uint32_t)ro >> 5)))) : 0u;
  // bin i + 1 follows bin i: in the same band, or first of the next one that holds bins
  const uint32_t p = (uint32_t)((re >> 13) + (int)(ee * i));
  qp_put(st, p, ze | (zo << ee));
}

// behind the code fields: the nw_out staged words to dst
__device__ __forceinline__ void store_slot(uint32_t* dst, const uint32_t* st_out, int nw_out, int lane) {
  wave_sync();
  for (int k = lane; k < nw_out; k += 64) dst[k] = st_out[k];
}

// lane 0's stores of what became of row r: fits[r] and, where asked (offset not null), offset[r]
__device__ __forceinline__ void store_fits(bool fit, int k, uint8_t* fits, int16_t* offset, long long r, int lane) {
  if (lane == 0) {
    fits[r] = fit ? 1 : 0;
    if (offset) offset[r] = (int16_t)k;
  }
}

}  // namespace
}  // namespace ac
