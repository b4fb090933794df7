// Packed rows to protected slots in one launch (k_protect_p, defined in ac_protect.hip): the
// sibling of k_transrate_p (ac_transrate_dev.h), on its device functions as they are.  A slot of slot_bytes = row_bytes +
// red_bytes holds the row at the plan's budget R (the primary part) and, behind it, the row of the frame before at the
// redundant budget R2 (the redundant part).  One wave owns one input row r = (b F + f) C + c and lane j holds band j; rows are
// independent, so no wave waits for another and a tail wave simply exits.
//
// Per input row the parse, the staging of the row, extract_sig_p into 8 registers and the band extremes run once, exactly as
// in transrate_row; the bisection and the pack run twice on the staged output slot, which is zeroed before each:
//   at R   into slot r, bytes [0, row_bytes): fits[r], offset[r];
//   at R2  into slot r + C -- frame f + 1 of the same clip and channel -- bytes [row_bytes, slot_bytes): red_fits[r + C],
//          red_offset[r + C].  Skipped at f = F - 1: that copy has no slot.
// The wave of a frame-0 row also zeroes the redundant part of its own slot (no wave packs into it) and sets red_fits there
// to 1, red_offset to 0.  So every output byte is written by exactly one wave.
//
// As one chunk of a stream (protect_row<true>, k_protect_ps in ac_protect_s.hip; DESIGN.md section 8g, "Streams"): the copy of
// the chunk's last input row is not dropped but packed into the carry (ProtectCarry), and the wave of a frame-0 row copies the
// carried words and flags of the chunk before into its slot where it zeroes above; on a fresh stream (row_in NULL) it zeroes.
// The carry is double buffered -- read from one half, written to the other, flipped by the host -- so still no wave waits for
// another and every output byte has one writer.
#pragma once
#include "ac_transrate_dev.h"

namespace ac {
namespace {

struct ProtectArgs {
  PackedRows in;         // data, nbytes, index [rows], band32, off
  uint8_t* data;         // [rows slot_bytes]
  uint8_t* fits;         // [rows]
  uint8_t* red_fits;     // [rows], indexed by the slot that holds the copy
  int16_t* offset;       // [rows] or null
  int16_t* red_offset;   // [rows] or null
  long long rows;
  int F, C;
  int row_bits, red_bits;     // R, R2
  int row_bytes, red_bytes;   // ceil(R / 32) * 4, ceil(R2 / 32) * 4
};

// (streams) the copy of the last input row of a chunk, per clip and channel sg = b C + c: what the next chunk's frame-0 slots hold
struct ProtectCarry {
  const uint8_t* row_in;      // [B, C, red_bytes], or null: a fresh stream
  const uint8_t* fits_in;     // [B, C]
  const int16_t* offset_in;   // [B, C]
  uint8_t* row_out;           // the other half: written by the waves of the frame-(F-1) rows
  uint8_t* fits_out;
  int16_t* offset_out;
};

// the search and the pack of transrate_row at `budget` bits into nw_out words at dst; returns (offset << 1) | fits in every lane
__device__ __forceinline__ int protect_pack(const uint32_t (&bw)[8], const uint32_t (&cw)[8], const uint32_t* rec_in,
                                            int* rec_out, uint32_t* st_out, int meta, int kx, int kn, uint32_t first,
                                            uint32_t len, int budget, int nw_out, uint32_t* dst, int lane) {
  for (int k = lane; k < nw_out; k += 64) st_out[k] = 0u;
  // ---- search: the smallest offset whose row meets the budget
  int lo = 0, hi = kRateMaxOffset;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int bits = __builtin_amdgcn_readfirstlane(5 * P_M + wave_sum(band_bits(meta, kx, kn, mid)));
    if (bits <= budget) hi = mid;
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
    wave_sync();   // (the slot is zero in every lane's view before a field is ORed in)
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
  for (int k = lane; k < nw_out; k += 64) dst[k] = st_out[k];
  wave_sync();   // (the staged slot and the output records are free again)
  return (lo << 1) | (fits ? 1 : 0);
}

// row r of a.in -> the primary part of slot r and the redundant part of slot r + C; w: the wave's slice of LDS
template <bool STREAM = false>
__device__ __forceinline__ void protect_row(const ProtectArgs& a, long long r, int lane, uint32_t* w, const ProtectCarry* pc = nullptr) {
  uint32_t* st_in = w;
  uint32_t* st_out = w + T_IN_WORDS;
  uint32_t* rec_in = st_out + T_OUT_WORDS;
  int* rec_out = reinterpret_cast<int*>(rec_in + P_M);
  int* qmx = rec_out + P_M;
  int* qmn = qmx + P_M;
  const PackedRows& pr = a.in;
  const int f = (int)((r / a.C) % a.F);
  const size_t slot_bytes = (size_t)a.row_bytes + (size_t)a.red_bytes;
  const size_t sg = (size_t)(r / ((long long)a.F * a.C)) * (size_t)a.C + (size_t)(r % a.C);   // (STREAM) the row's clip and channel

  // ---- parse: the header, the band records, then the rest of the row (transrate_row's)
  int64_t at = pr.index[r];
  at = at > pr.nbytes ? pr.nbytes : (at < -(1ll << 40) ? -(1ll << 40) : at);
  if (lane < P_HDR_WORDS) st_in[lane] = p_load_word(pr.data, pr.nbytes, at + 4ll * lane);
  qmx[lane] = INT_MIN;
  qmn[lane] = INT_MAX;
  if (f == 0) {   // no wave packs into the redundant part of a frame-0 slot
    uint32_t* red = reinterpret_cast<uint32_t*>(a.data + (size_t)r * slot_bytes + (size_t)a.row_bytes);
    bool fresh = true;
    if constexpr (STREAM) fresh = pc->row_in == nullptr;
    if (fresh) {
      for (int k = lane; k < (a.red_bytes >> 2); k += 64) red[k] = 0u;
      if (lane == 0) {
        a.red_fits[r] = 1;
        if (a.red_offset) a.red_offset[r] = 0;
      }
    } else if constexpr (STREAM) {   // the copy of the chunk before's last row of this clip and channel
      const uint32_t* src = reinterpret_cast<const uint32_t*>(pc->row_in + sg * (size_t)a.red_bytes);
      for (int k = lane; k < (a.red_bytes >> 2); k += 64) red[k] = src[k];
      if (lane == 0) {
        a.red_fits[r] = pc->fits_in[sg];
        if (a.red_offset) a.red_offset[r] = pc->offset_in[sg];
      }
    }
  }
  wave_sync();
  const uint32_t first = (uint32_t)pr.off[lane];
  const uint32_t len = (uint32_t)pr.off[lane + 1] - first;   // bins of the lane's band
  uint32_t nw_in;
  {
    uint32_t wd = p_get_bits(st_in, 5u * lane, 5);
    if (wd > 16) wd = 31;   // 17 .. 30: damaged, read as a non-finite band
    const uint32_t v = p_stores(wd) ? (1u << 16) | (wd * len) : 0u;
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

  // ---- band `lane`'s meta word and extremes, shared by the two searches
  const int s_in = t_rec_sf(rec_in[lane]);
  const int meta = len == 0 ? 0 : s_in == -128 ? -1 : (int)(len << 8) | (s_in & 0xff);
  const int kx = ordered_key(dequant(qmx[lane], s_in)), kn = ordered_key(dequant(qmn[lane], s_in));

  // ---- the primary part of slot r
  uint8_t* slot = a.data + (size_t)r * slot_bytes;
  const int p0 = protect_pack(bw, cw, rec_in, rec_out, st_out, meta, kx, kn, first, len, a.row_bits, a.row_bytes >> 2,
                              reinterpret_cast<uint32_t*>(slot), lane);
  if (lane == 0) {
    a.fits[r] = (uint8_t)(p0 & 1);
    if (a.offset) a.offset[r] = (int16_t)(p0 >> 1);
  }
  if constexpr (STREAM) {
    if (f == a.F - 1) {   // the copy of the chunk's last frame goes into the carry
      const int pl = protect_pack(bw, cw, rec_in, rec_out, st_out, meta, kx, kn, first, len, a.red_bits, a.red_bytes >> 2,
                                  reinterpret_cast<uint32_t*>(pc->row_out + sg * (size_t)a.red_bytes), lane);
      if (lane == 0) {
        pc->fits_out[sg] = (uint8_t)(pl & 1);
        pc->offset_out[sg] = (int16_t)(pl >> 1);
      }
      return;
    }
  } else {
    if (f == a.F - 1) return;   // the copy of a clip's last frame has no slot
  }
  // ---- the redundant part of slot r + C: the same frame of input at R2
  const int p1 = protect_pack(bw, cw, rec_in, rec_out, st_out, meta, kx, kn, first, len, a.red_bits, a.red_bytes >> 2,
                              reinterpret_cast<uint32_t*>(slot + (size_t)a.C * slot_bytes + (size_t)a.row_bytes), lane);
  if (lane == 0) {
    a.red_fits[r + a.C] = (uint8_t)(p1 & 1);
    if (a.red_offset) a.red_offset[r + a.C] = (int16_t)(p1 >> 1);
  }
}

}  // namespace
}  // namespace ac
