// Packed rows of several sources to one packed row at the plan's budget in one launch (k_mix_p, defined in ac_mix.hip on mix_row
// below): the sibling of k_transrate_p (ac_transrate_dev.h) that reads S rows where that one reads one.
// filters_n = 1024 with bark_bands_n = 64; one wave owns one output row and lane j holds band j; a tail wave simply exits.
//
// Per active source, in source order, with transrate_row's steps as they are:
//   parse    the 26 header words through p_load_word, lane j reads band j's width, one wave-wide scan gives its sf field and
//            first code bit; the rest of the row is staged with plain dword loads where it is plain, clamped loads elsewhere.
//   extract  extract_sig_p on the staged row: the lane's 16 codes and the sf bytes of their bands.
//   sum      g = -128 for a stored sf of -128, else clamp(sf + gain, -127, 127); x = dequant(code, g) -- the exact product of
//            ac_quant_dev.h, kept apart from the add -- and acc += x in 16 float32 registers.  A code of 0 adds +0, whatever
//            its band; a band with sf = -128 adds NaN.  A non-zero code flags its band in LDS, so that lane j folds band j's
//            s0: bad where any source's sf is -128, else the largest g over the sources that flagged it.
// Then the band extremes of the sum through ordered keys (ds_max / ds_min), band j's meta word from s0 (not from a threshold),
// the bisection of [0, 254] with band_bits and wave_sum, and the packer as transrate_row's: fits before any field is ORed in,
// codes by qcode on the sum.  The bytes are those of the composition: ac_unpack and ac_dequantize per source, float32 adds in
// source order, ac_quantize_budget at kmin 0 under thr = crit(s0), rows longer than the slot marked, ac_pack.
#pragma once
#include "ac_transrate_dev.h"

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

// a value the compiler cannot see through: the product above it is a product, never half of a multiply-add
__device__ __forceinline__ float x_opaque(float v) {
  asm volatile("" : "+v"(v));
  return v;
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
  const int nw_out = a.out.row_bytes >> 2;

  for (int k = lane; k < nw_out; k += 64) st_out[k] = 0u;
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
    const int gain = a.gain[src];
    // ---- parse: the header, the band records, then the rest of the row
    int64_t at = a.index[src][r];
    // a row start beyond the buffer reads nothing; clamping it keeps start + 4 k from overflowing
    at = at > nbytes ? nbytes : (at < -(1ll << 40) ? -(1ll << 40) : at);
    wave_sync();   // (the source before is done with st_in, rec_in and nz)
    if (lane < P_HDR_WORDS) st_in[lane] = p_load_word(data, nbytes, at + 4ll * lane);
    nz[lane] = 0u;
    wave_sync();
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
    if (at >= 0 && (at & 3) == 0 && at + 4ll * nw_in <= nbytes) {
      const uint32_t* row = reinterpret_cast<const uint32_t*>(data + at);
      for (uint32_t k = P_HDR_WORDS + lane; k < nw_in; k += 64) st_in[k] = row[k];
    } else {
      for (uint32_t k = P_HDR_WORDS + lane; k < nw_in; k += 64) st_in[k] = p_load_word(data, nbytes, at + 4ll * k);
    }
    wave_sync();

    // ---- extract and sum: the lane's 16 codes at their bands' gained steps into acc; the bands that hold a non-zero code
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
    t_code_fields(st_out, rec_out[j0], rec_out[j1], acc[2 * i], acc[2 * i + 1], (uint32_t)(128 * i + 2 * lane));
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
