// Packed rows to protected slots in one launch (k_protect_p, defined in ac_protect.hip): the
// sibling of k_transrate_p, on its device functions (ac_transrate_dev.h) and the shared steps of ac_rows_dev.h.  A slot of
// slot_bytes = row_bytes + red_bytes holds the row at the plan's budget R (the primary part) and, behind it, the row of the
// frame before at the redundant budget R2 (the redundant part).  One wave owns one input row r = (b F + f) C + c; rows are
// independent, so no wave waits for another and a tail wave simply exits.
//
// Per input row the parse, the extract into 8 registers and the band extremes run once, as in transrate_row; the search and the
// pack (protect_pack on t_repack) run twice on the staged output slot, which is zeroed before each:
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

// (host) the arguments of both kernels from the plan and the caller's buffers
inline ProtectArgs protect_args(const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes, const int64_t* index, uint8_t* out,
                                int64_t row_bytes, int red_bits, uint8_t* fits, uint8_t* red_fits, int16_t* offset,
                                int16_t* red_offset, long long rows, int F, int C) {
  ProtectArgs a;
  a.in = plan_rows(psy, data, nbytes, index);
  a.data = out;
  a.fits = fits;
  a.red_fits = red_fits;
  a.offset = offset;
  a.red_offset = red_offset;
  a.rows = rows;
  a.F = F;
  a.C = C;
  a.row_bits = psy->row_bits;
  a.red_bits = red_bits;
  a.row_bytes = (int)row_bytes;
  a.red_bytes = (red_bits + 31) / 32 * 4;
  return a;
}

// t_repack at `budget` bits into nw words at dst, through a slot zeroed here, between two packs: the sync ahead keeps the
// zeroes behind the last pack's reads of the slot and the output records, pack_header's keeps them ahead of the first field
__device__ __forceinline__ int protect_pack(const uint32_t (&bw)[8], const uint32_t (&cw)[8], const uint32_t* rec_in,
                                            int* rec_out, uint32_t* st_out, int meta, int kx, int kn, uint32_t first,
                                            uint32_t len, int budget, int nw, uint8_t* dst, int lane) {
  wave_sync();
  for (int k = lane; k < nw; k += 64) st_out[k] = 0u;
  return t_repack(bw, cw, rec_in, rec_out, st_out, meta, kx, kn, first, len, budget, nw, reinterpret_cast<uint32_t*>(dst),
                  lane);
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

  const int64_t at = row_start(pr.index, r, pr.nbytes);
  stage_header(st_in, pr.data, pr.nbytes, at, lane);
  qmx[lane] = INT_MIN;
  qmn[lane] = INT_MAX;
  if (f == 0) {   // no wave packs into the redundant part of a frame-0 slot
    uint32_t* red = reinterpret_cast<uint32_t*>(a.data + (size_t)r * slot_bytes + (size_t)a.row_bytes);
    bool fresh = true;
    if constexpr (STREAM) fresh = pc->row_in == nullptr;
    if (fresh) {
      for (int k = lane; k < (a.red_bytes >> 2); k += 64) red[k] = 0u;
      store_fits(true, 0, a.red_fits, a.red_offset, r, lane);
    } else if constexpr (STREAM) {   // the copy of the chunk before's last row of this clip and channel
      const uint32_t* src = reinterpret_cast<const uint32_t*>(pc->row_in + sg * (size_t)a.red_bytes);
      for (int k = lane; k < (a.red_bytes >> 2); k += 64) red[k] = src[k];
      if (lane == 0) {
        a.red_fits[r] = pc->fits_in[sg];
        if (a.red_offset) a.red_offset[r] = pc->offset_in[sg];
      }
    }
  }
  const uint32_t first = (uint32_t)pr.off[lane];
  const uint32_t len = (uint32_t)pr.off[lane + 1] - first;   // bins of the lane's band
  stage_row(st_in, rec_in, pr.data, pr.nbytes, at, len, lane);

  // ---- the codes, band `lane`'s meta word and extremes: shared by the two searches
  uint32_t bw[8], cw[8];
  int meta, kx, kn;
  load_bw_p<8>(pr, lane, bw);
  t_code_stats(st_in, rec_in, bw, qmx, qmn, len, lane, cw, meta, kx, kn);

  // ---- the primary part of slot r
  uint8_t* slot = a.data + (size_t)r * slot_bytes;
  const int p0 = protect_pack(bw, cw, rec_in, rec_out, st_out, meta, kx, kn, first, len, a.row_bits, a.row_bytes >> 2, slot,
                              lane);
  store_fits(p0 & 1, p0 >> 1, a.fits, a.offset, r, lane);
  if constexpr (STREAM) {
    if (f == a.F - 1) {   // the copy of the chunk's last frame goes into the carry
      const int pl = protect_pack(bw, cw, rec_in, rec_out, st_out, meta, kx, kn, first, len, a.red_bits, a.red_bytes >> 2,
                                  pc->row_out + sg * (size_t)a.red_bytes, lane);
      if (lane == 0) {   // (not store_fits: the carry always holds the offset)
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
                              slot + (size_t)a.C * slot_bytes + (size_t)a.row_bytes, lane);
  store_fits(p1 & 1, p1 >> 1, a.red_fits, a.red_offset, r + a.C, lane);
}

}  // namespace
}  // namespace ac
