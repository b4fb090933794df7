// The third spectrum source of the wave-level synthesis (inv_fast_body, ac_fast_inv_dev.h): rows of the packed bitstream
// (ac_pack.hip), read where k_inv_fast_q reads codes and scale factors.  filters_n = 1024 with
// bark_bands_n = 64 only: a row has as many bands as a wave has lanes.
//
//   parse_strip_p  once per strip, before the frame loop: the header words (5M width bits + 8M scale-factor bits = 26 words)
//                  of every row the strip reads -- at most P_SLOTS frames x 2 signals -- are loaded in one round trip into
//                  the wave's FFT buffer; lane j reads band j's width, a wave-wide scan of (stored bands << 16 | code bits)
//                  gives its sf field and the bit position of its codes, and the lane leaves the band's record
//                  (first code bit << 13 | sf byte << 5 | width) in the wave's record region of LDS.
//   load_row_p     in place of load_row_q, one frame ahead: bins 2q and 2q+1 of a granule are adjacent fields of the row
//                  (a band's codes follow the band before it), so one two-dword window at the first field's bit covers both.
//   extract_row_p  where the frame is dequantised: shift, mask, un-zigzag -> the QGran load_row_q would have loaded from
//                  ac_unpack's codes and sf.
//
// Row semantics are ac_unpack's (k_unpack): a width of 17 .. 30 reads as 31; width 31 gives codes 0 and sf -128, width 0 sf 0;
// bits outside [0, nbytes) read as 0 and are never loaded; a row start may be any int64.  A row whose words all lie inside
// data at a 4-byte phase takes plain dword loads; any other row (the last one of data, damaged input) takes p_load_word.
//
// Concealment of lost rows (parse_strip_p<true>, k_inv_fast_pl in ac_fast_inv_pl.hip): a row that did not
// arrive is read from the last row of its clip and channel that did, at most max_age frames back, with every scale factor
// lowered by AC_CONCEAL_FADE per frame of age; a row with no such source reads as a row that starts at nbytes (silence).
// Only the row start and the sf byte of the band records change: load_row_p and extract_row_p see a row like any other.
//
// ... in a stream (parse_strip_p<true, true>, k_inv_fast_pls in ac_fast_inv_pls.hip): the launch is one chunk, and the last row
// that arrived before it is carried in the stream's state (ConcealState) with its gap, the frames of the stream since it.  A
// lane that looks at a frame before the chunk finds that row there, the row is read from the state buffer -- a second base
// the row's loads select with a wave-uniform flag -- and the wave that owns a signal's last strip leaves the new state in the
// other half of a double buffer (carry_state_p).
//
// Recovery from the redundant copy (parse_strip_p<true, false, true>, k_inv_fast_plr in ac_fast_inv_plr.hip; DESIGN.md section
// 8g): a lost row whose successor arrived is read from index[b, f+1, c] + redundant_at -- the copy the successor's slot
// carries -- with age 0, ahead of every rule above.  Beside the look-back the row's half wave loads lost[b, f+1, c] and, with
// it, index[b, f+1, c]: frame f + 1 is usually outside the strip and only an address, as the source of a concealed row is.
//
// ... in a stream (parse_strip_p<true, true, true>, k_inv_fast_plsr in ac_fast_inv_plsr.hip; DESIGN.md section 8g, "Streams"):
// the chunk is synthesised one frame behind its rows, so that the successor of every frame it synthesises is a row of the chunk
// in hand.  The caller passes `base` in rows: synthesis frame n reads row n - 1, and row -1 is the deferred row D, the last row
// of the chunk before -- lost unless gap == 0, and then the carried row itself, read from the state buffer at age 0.  The
// look-back below gives that at f = -1 as it stands (lane k finds the carried row where k == gap); only the loads of `lost` and
// `index` at f itself are kept to f >= 0.
#pragma once
#include "ac_fast_dev.h"

namespace ac {
namespace {

struct PackedRows {
  const uint8_t* data;
  int64_t nbytes;
  const int64_t* index;    // [B, Kp, C]
  const uint32_t* band32;  // [N/2]: bands of bins 2q | 2q+1 << 16
  const int32_t* off;      // [M + 1]: first bin of every band
};

struct ConcealRows {
  const uint8_t* lost;     // [B, Kp, C]: nonzero = the row did not arrive
  int max_age;             // 0 .. AC_CONCEAL_MAX_AGE (31: a lane of half a wave per frame looked back at)
};

// (streams) the concealment state of a chunked decode, double buffered: other strips of a signal still read what its last strip
// replaces.  A carried row is the P_CARRY_WORDS words from the row's start -- the most a row of 64 bands and 1024 bins takes --
// at a stride that keeps the two further words a code window may touch inside the buffer (they stay 0): plain dword loads.
struct ConcealState {
  const uint8_t* gap;      // [B, C]: frames since the last row that arrived, at the end of the previous chunk; 32 = none in reach
  const uint8_t* row;      // [B, C] carried rows, P_CARRY_STRIDE bytes apart
  uint8_t* gap_out;        // the state after this chunk
  uint8_t* row_out;
  int64_t row_bytes;       // B C P_CARRY_STRIDE
  int stale;               // nonzero: every gap reads as 32 (a new stream, after a reset or a chunk that did not conceal)
};
struct RedundRows {
  int64_t at;              // redundant_at: bytes from a row's start to the copy of the frame before it, in [1, 2^31)
};
constexpr int P_CARRY_WORDS = (5 * 64 + 8 * 64 + 16 * 1024) / 32;   // 538
constexpr int P_CARRY_STRIDE = 2176;
constexpr int P_NO_SOURCE = 32;               // a gap no max_age (<= 31) reaches

constexpr int P_M = 64;                       // bands of a row = lanes of a wave
constexpr int P_SLOTS = 4;                    // frames a strip reads: at most 3 output blocks and the frame before them
constexpr int P_ROWS = 2 * P_SLOTS;           // row r = 2 slot + signal
constexpr int P_HDR_WORDS = (13 * P_M) / 32;  // words that can hold widths and scale factors
constexpr int P_REC_BYTES = P_ROWS * (P_M * 4 + 16);   // per wave: the records [P_ROWS][64], then (start lo, hi, fast, age) per row

struct PGran {   // the two-dword window of a granule, per signal
  uint32_t lo0, hi0, lo1, hi1;
};

__device__ __forceinline__ bool p_stores(uint32_t w) { return w - 1u < 16u; }   // widths 1 .. 16 store an sf and codes
__device__ __forceinline__ int16_t p_unzigzag(uint32_t z) { return (int16_t)((z >> 1) ^ (0u - (z & 1u))); }
// the little-endian word at byte a of data; bytes outside [0, nbytes) read as 0 (never loaded) -- as in ac_pack.hip
__device__ __forceinline__ uint32_t p_load_word(const uint8_t* __restrict__ data, int64_t nbytes, int64_t a) {
  if (a >= 0 && a + 4 <= nbytes && (a & 3) == 0) return *reinterpret_cast<const uint32_t*>(data + a);
  uint32_t r = 0;
  for (int k = 0; k < 4; ++k) {
    const int64_t e = a + k;
    if (e >= 0 && e < nbytes) r |= (uint32_t)data[e] << (8 * k);
  }
  return r;
}
// the w-bit field at bit p of the staged header st (w <= 16)
__device__ __forceinline__ uint32_t p_get_bits(const uint32_t* st, uint32_t p, uint32_t w) {
  const uint32_t q = p >> 5, sh = p & 31;
  const uint32_t lo = st[q], hi = sh + w > 32 ? st[q + 1] : 0u;
  return __builtin_amdgcn_alignbit(hi, lo, sh) & ((1u << w) - 1u);
}
// first bit of the field of the bin d bins into the band of record rec (a band that stores nothing takes no bits)
__device__ __forceinline__ uint32_t p_pos(uint32_t rec, uint32_t d) {
  const uint32_t w = rec & 31u;
  return (rec >> 13) + (p_stores(w) ? w * d : 0u);
}

// The records of the rows of frames base + slot, slot in [slot_lo, slot_hi), of the wave's two signals.  buf: the wave's FFT
// buffer (free before the frame loop); rec: the wave's record region.  CONCEAL: the rows are looked up through cl (above);
// STREAM: frame -1 - gap is the carried row of cs.  REDUND: a lost row whose successor arrived is read from the successor's
// copy of it (rd).
template <bool CONCEAL = false, bool STREAM = false, bool REDUND = false>
__device__ __forceinline__ void parse_strip_p(const PackedRows& pr, long long b0, long long b1, int c0, int c1, int Kp, int C,
                                              int base, int slot_lo, int slot_hi, bool has1, int lane, char* buf,
                                              uint32_t* rec, const ConcealRows* cl = nullptr, const ConcealState* cs = nullptr,
                                              const RedundRows* rd = nullptr) {
  static_assert(CONCEAL || !STREAM, "the carried row is a source of concealment");
  static_assert(!REDUND || CONCEAL, "recovery comes ahead of concealment");
  constexpr bool DELAYED = STREAM && REDUND;         // frames base + slot may be row -1, the deferred row (above)
  uint32_t* st = reinterpret_cast<uint32_t*>(buf);   // [P_ROWS][P_HDR_WORDS]
  uint32_t* info = rec + P_ROWS * P_M;
  const int sig = lane >> 5, k = lane & 31;          // half a wave per row: slot t, signal sig
  int gap = P_NO_SOURCE;                             // (STREAM) of the half wave's signal: one load, ahead of every slot's `lost`
  if constexpr (STREAM) {
    if ((sig == 0 || has1) && !cs->stale) gap = (int)cs->gap[(size_t)(sig ? b1 : b0) * (size_t)C + (size_t)(sig ? c1 : c0)];
  }
#pragma unroll
  for (int t = 0; t < P_SLOTS; ++t) {
    int age = 0;         // (CONCEAL) frames back to the row that is read in this one's place ...
    bool muted = false;  // ... or there is none
    int64_t own = 0;     // (CONCEAL) the row's own start, loaded beside `lost`: the start of every row that arrived
    bool recover = false;  // (REDUND) the row is lost and its successor arrived ...
    int64_t nxt = 0;       // ... at this start
    if constexpr (CONCEAL) {
      // lane k of the row's half wave looks at frame f - k: the first one that arrived is the source
      const bool on = t >= slot_lo && t < slot_hi && (sig == 0 || has1);
      const long long b = sig ? b1 : b0;
      const int c = sig ? c1 : c0;
      const int f = base + t;
      if (on && k < P_HDR_WORDS && (!DELAYED || f >= 0)) own = pr.index[((size_t)b * (size_t)Kp + (size_t)f) * (size_t)C + (size_t)c];
      bool succ = false;   // (REDUND) frame f + 1 of the signal exists and arrived: one byte, the same in the half wave's lanes
      if constexpr (REDUND) {
        if (on && f + 1 < Kp) {
          const size_t e = ((size_t)b * (size_t)Kp + (size_t)(f + 1)) * (size_t)C + (size_t)c;
          succ = cl->lost[e] == 0;
          if (k < P_HDR_WORDS) nxt = pr.index[e];
        }
      }
      bool there;
      if constexpr (STREAM) {
        // a frame before the chunk is there exactly where the carried row sits: gap frames before frame 0 (32: nowhere)
        const bool look = on && k <= cl->max_age;
        there = look && k > f && f - k == -1 - gap;
        if (look && k <= f) there = cl->lost[((size_t)b * (size_t)Kp + (size_t)(f - k)) * (size_t)C + (size_t)c] == 0;
      } else {
        there = on && k <= min(cl->max_age, f) &&
                cl->lost[((size_t)b * (size_t)Kp + (size_t)(f - k)) * (size_t)C + (size_t)c] == 0;
      }
      const uint64_t m = __builtin_amdgcn_ballot_w64(there);
      const uint32_t mh = sig ? (uint32_t)(m >> 32) : (uint32_t)m;
      muted = mh == 0u;
      age = muted ? 0 : __builtin_ctz(mh);
      if constexpr (REDUND) {   // lane 0 of the half wave looked at the row itself: bit 0 clear = lost
        recover = succ && (mh & 1u) == 0u;
        if (recover) {
          age = 0;
          muted = false;
        }
      }
    }
    if (t >= slot_lo && t < slot_hi && (sig == 0 || has1) && k < P_HDR_WORDS) {
      const int r = 2 * t + sig;
      const long long b = sig ? b1 : b0;
      const int c = sig ? c1 : c0;
      int64_t a;
      bool carried = false;   // (STREAM) the source lies before the chunk: the carried row of (b, c)
      if constexpr (STREAM) carried = !muted && !recover && age > base + t;   // (D that arrived: age 0 > -1)
      if constexpr (CONCEAL) {
        a = own;
        if (age != 0 && !carried) a = pr.index[((size_t)b * (size_t)Kp + (size_t)(base + t - age)) * (size_t)C + (size_t)c];
        if (muted) a = pr.nbytes;
        if constexpr (REDUND) {
          if (recover) a = (int64_t)((uint64_t)nxt + (uint64_t)rd->at);   // (wraps as the int64 sum of the definition does)
        }
      } else {
        a = pr.index[((size_t)b * (size_t)Kp + (size_t)(base + t)) * (size_t)C + (size_t)c];
      }
      // a row start beyond the buffer reads nothing; clamping it keeps start + 4 k from overflowing
      a = a > pr.nbytes ? pr.nbytes : (a < -(1ll << 40) ? -(1ll << 40) : a);
      const uint8_t* src = pr.data;
      int64_t bound = pr.nbytes;
      if constexpr (STREAM) {
        if (carried) {
          a = ((int64_t)b * C + c) * P_CARRY_STRIDE;
          src = cs->row;
          bound = cs->row_bytes;
        }
      }
      st[r * P_HDR_WORDS + k] = p_load_word(src, bound, a + 4ll * k);
      if (k == 0) {
        info[4 * r] = (uint32_t)(uint64_t)a;
        info[4 * r + 1] = (uint32_t)((uint64_t)a >> 32);
        if constexpr (CONCEAL) info[4 * r + 3] = (uint32_t)age | (carried ? 0x100u : 0u);   // bit 8: read from the state buffer
      }
    }
  }
  wave_sync();
  const uint32_t len = (uint32_t)(pr.off[lane + 1] - pr.off[lane]);   // bins of the lane's band
#pragma unroll 1
  for (int r = 2 * slot_lo; r < 2 * slot_hi; ++r) {
    if ((r & 1) && !has1) continue;
    const uint32_t* sr = st + r * P_HDR_WORDS;
    uint32_t w = p_get_bits(sr, 5u * lane, 5);
    if (w > 16) w = 31;   // 17 .. 30: damaged, read as a non-finite band
    const uint32_t v = p_stores(w) ? (1u << 16) | (w * len) : 0u;   // (code bits of a row <= 16 N = 2^14)
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
    if (w == 31) sfb = 0x80u;
    else if (p_stores(w)) sfb = p_get_bits(sr, 5u * P_M + 8u * (ex >> 16), 8);
    if constexpr (CONCEAL) {   // every sf but -128 fades: max(s - AC_CONCEAL_FADE * age, -127)
      const int fade = 4 * (__builtin_amdgcn_readfirstlane((int)info[4 * r + 3]) & (STREAM ? 0xff : -1));
      if (sfb != 0x80u) sfb = (uint32_t)max((int)(int8_t)sfb - fade, -127) & 0xffu;
    }
    rec[r * P_M + lane] = ((cbase + (ex & 0xffffu)) << 13) | (sfb << 5) | w;
    if (lane == 0) {
      // plain loads where every word a window of this row can touch -- its ceil(bits / 32) words and two more -- is in data
      const int64_t a = (int64_t)((uint64_t)info[4 * r] | ((uint64_t)info[4 * r + 1] << 32));
      const int64_t nw = (int64_t)((cbase + (total & 0xffffu) + 31u) >> 5);
      if constexpr (STREAM) {   // bit 1: the row is read from the state buffer
        const uint32_t sel = (info[4 * r + 3] >> 8) & 1u;
        info[4 * r + 2] = ((a >= 0 && (a & 3) == 0 && a + 4 * (nw + 2) <= (sel ? cs->row_bytes : pr.nbytes)) ? 1u : 0u) | (sel << 1);
      } else {
        info[4 * r + 2] = (a >= 0 && (a & 3) == 0 && a + 4 * (nw + 2) <= pr.nbytes) ? 1u : 0u;
      }
    }
  }
  wave_sync();
}

// bw[i]: band of bin 2q | band of bin 2q+1 << 6 | (2q - first bin of its band) << 12, q = 64 i + lane
template <int R>
__device__ __forceinline__ void load_bw_p(const PackedRows& pr, int lane, uint32_t (&bw)[R]) {
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int q = 64 * i + lane;
    const uint32_t b = pr.band32[q], j0 = b & 0xffffu, j1 = b >> 16;
    bw[i] = j0 | (j1 << 6) | ((uint32_t)(2 * q - pr.off[j0]) << 12);
  }
}

// the window loads of row r: only loads, LDS reads and address arithmetic
// (STREAM: bit 1 of the row's flag word selects the state buffer of cs as base and bound -- one choice per row and wave)
template <int R, bool STREAM = false>
__device__ __forceinline__ void load_sig_p(const PackedRows& pr, const uint32_t* rec, int r, const uint32_t (&bw)[R],
                                           uint32_t (&lo)[R], uint32_t (&hi)[R], const ConcealState* cs = nullptr) {
  const uint32_t* info = rec + P_ROWS * P_M;
  const uint32_t* rr = rec + r * P_M;
  const uint32_t a_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)info[4 * r]);
  const uint32_t a_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)info[4 * r + 1]);
  const int64_t a = (int64_t)((uint64_t)a_lo | ((uint64_t)a_hi << 32));
  const int flag = __builtin_amdgcn_readfirstlane((int)info[4 * r + 2]);
  const uint8_t* data = pr.data;
  int64_t nbytes = pr.nbytes;
  if constexpr (STREAM) {
    data = (flag & 2) ? cs->row : pr.data;
    nbytes = (flag & 2) ? cs->row_bytes : pr.nbytes;
  }
  if (STREAM ? (flag & 1) : flag) {
    const uint32_t* row = reinterpret_cast<const uint32_t*>(data + a);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const uint32_t wi = p_pos(rr[bw[i] & 63u], bw[i] >> 12) >> 5;
      lo[i] = row[wi];
      hi[i] = row[wi + 1];
    }
  } else {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const uint32_t wi = p_pos(rr[bw[i] & 63u], bw[i] >> 12) >> 5;
      lo[i] = p_load_word(data, nbytes, a + 4ll * wi);
      hi[i] = p_load_word(data, nbytes, a + 4ll * wi + 4);
    }
  }
}
// issues the window loads of the frame in `slot`, one frame ahead as load_row_q
template <int R, bool STREAM = false>
__device__ __forceinline__ void load_row_p(const PackedRows& pr, const uint32_t* rec, int slot, const uint32_t (&bw)[R],
                                           bool has1, PGran (&g)[R], const ConcealState* cs = nullptr) {
  uint32_t lo[R], hi[R];
  load_sig_p<R, STREAM>(pr, rec, 2 * slot, bw, lo, hi, cs);
#pragma unroll
  for (int i = 0; i < R; ++i) {
    g[i].lo0 = lo[i];
    g[i].hi0 = hi[i];
    g[i].lo1 = g[i].hi1 = 0u;
  }
  if (has1) {
    load_sig_p<R, STREAM>(pr, rec, 2 * slot + 1, bw, lo, hi, cs);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      g[i].lo1 = lo[i];
      g[i].hi1 = hi[i];
    }
  }
}

// the two fields of a window -> codes of bins 2q, 2q+1 (low, high half) and their scale-factor bytes (bits 0-7, 16-23)
__device__ __forceinline__ void extract_sig_p(const uint32_t* rr, uint32_t bwi, uint32_t lo, uint32_t hi, uint32_t& codes,
                                              uint32_t& sfs) {
  const uint32_t r0 = rr[bwi & 63u], r1 = rr[(bwi >> 6) & 63u];
  const uint32_t w0 = r0 & 31u, w1 = r1 & 31u;
  const uint32_t e0 = p_stores(w0) ? w0 : 0u, e1 = p_stores(w1) ? w1 : 0u;
  const uint32_t sh = p_pos(r0, bwi >> 12) & 31u;
  const uint64_t win = (uint64_t)lo | ((uint64_t)hi << 32);
  // bin 2q+1 follows bin 2q: in the same band, or first of the next one that holds bins
  const uint32_t z0 = (uint32_t)(win >> sh) & ((1u << e0) - 1u);
  const uint32_t z1 = (uint32_t)(win >> (sh + e0)) & ((1u << e1) - 1u);
  codes = (uint32_t)(uint16_t)p_unzigzag(z0) | ((uint32_t)(uint16_t)p_unzigzag(z1) << 16);
  sfs = ((r0 >> 5) & 0xffu) | (((r1 >> 5) & 0xffu) << 16);
}
// the loaded windows -> the raw codes and scale-factor bytes of the frame, in load_row_q's order
template <int R>
__device__ __forceinline__ void extract_row_p(const uint32_t* rec, int slot, const uint32_t (&bw)[R], bool has1,
                                              const PGran (&g)[R], QGran (&out)[R]) {
  const uint32_t* rr0 = rec + 2 * slot * P_M;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    uint32_t c0, f0, c1 = 0u, f1 = 0u;
    extract_sig_p(rr0, bw[i], g[i].lo0, g[i].hi0, c0, f0);
    if (has1) extract_sig_p(rr0 + P_M, bw[i], g[i].lo1, g[i].hi1, c1, f1);
    out[i].code = s4{(short)(c0 & 0xffffu), (short)(c1 & 0xffffu), (short)(c0 >> 16), (short)(c1 >> 16)};
    out[i].sfw = f0 | (f1 << 8);
  }
}

// (streams) The concealment state a chunk of Kp frames leaves for the wave's two signals, written into the other half of the
// double buffer by the wave that owns their last strip.  Lane k of a signal's half wave looks at frame Kp-1 - k, whatever
// max_age is: the first one that arrived is the new carried row and k the new gap; a frame before the chunk is there where the
// old carried row sits, which is then kept; none in 32 frames: gap 32, and the row is left unspecified.
// the P_CARRY_WORDS words at src (4-byte aligned, all readable) to dst: every load of a lane in flight before its first store
__device__ __forceinline__ void copy_carried_row(uint32_t* dst, const uint32_t* src, int lane) {
  constexpr int PER = (P_CARRY_WORDS + 63) / 64;
  uint32_t v[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) v[i] = (64 * i + lane < P_CARRY_WORDS) ? src[64 * i + lane] : 0u;
#pragma unroll
  for (int i = 0; i < PER; ++i)
    if (64 * i + lane < P_CARRY_WORDS) dst[64 * i + lane] = v[i];
}

__device__ __forceinline__ void carry_state_p(const PackedRows& pr, const ConcealRows& cl, const ConcealState& cs, long long b0,
                                              long long b1, int c0, int c1, int Kp, int C, bool has1, int lane) {
  const int sig = lane >> 5, k = lane & 31;
  const bool on = sig == 0 || has1;
  const long long b = sig ? b1 : b0;
  const int c = sig ? c1 : c0;
  const int f = Kp - 1 - k;
  const int gap = (on && !cs.stale) ? (int)cs.gap[(size_t)b * (size_t)C + (size_t)c] : P_NO_SOURCE;
  const bool there = on && (f >= 0 ? cl.lost[((size_t)b * (size_t)Kp + (size_t)f) * (size_t)C + (size_t)c] == 0 : f == -1 - gap);
  const uint64_t m = __builtin_amdgcn_ballot_w64(there);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (s && !has1) break;
    const uint32_t mh = s ? (uint32_t)(m >> 32) : (uint32_t)m;   // (wave-uniform: the branches below are scalar)
    const long long bs = s ? b1 : b0;
    const int csg = s ? c1 : c0;
    const size_t sg = (size_t)bs * (size_t)C + (size_t)csg;
    const int ngap = mh ? __builtin_ctz(mh) : P_NO_SOURCE;
    if (lane == 0) cs.gap_out[sg] = (uint8_t)ngap;
    if (mh == 0u) continue;
    uint32_t* dst = reinterpret_cast<uint32_t*>(cs.row_out + sg * (size_t)P_CARRY_STRIDE);
    const int fs = Kp - 1 - ngap;
    if (fs >= 0) {
      const int64_t own = pr.index[((size_t)bs * (size_t)Kp + (size_t)fs) * (size_t)C + (size_t)csg];
      int64_t a = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)own) |
                            ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)own >> 32)) << 32));
      a = a > pr.nbytes ? pr.nbytes : (a < -(1ll << 40) ? -(1ll << 40) : a);
      if (a >= 0 && (a & 3) == 0 && a + 4ll * P_CARRY_WORDS <= pr.nbytes) {   // the usual row: plain loads
        copy_carried_row(dst, reinterpret_cast<const uint32_t*>(pr.data + a), lane);
      } else {
        for (int w = lane; w < P_CARRY_WORDS; w += 64) dst[w] = p_load_word(pr.data, pr.nbytes, a + 4ll * w);
      }
    } else {
      copy_carried_row(dst, reinterpret_cast<const uint32_t*>(cs.row + sg * (size_t)P_CARRY_STRIDE), lane);
    }
  }
}

}  // namespace
}  // namespace ac
