// The packer as the last stage of the budgeted fused encode at filters_n = 1024 (k_fwd_fast_qp, instantiated in
// ac_fast_fwd_qp.hip): QuantStage's BUDGET form (ac_fast_quant_dev.h) up to the end of the offset search, then the wave
// writes the frame's packed rows itself -- fixed-stride "packed rows" (DESIGN.md section 8b): row r = (b F + f) C + c takes
// bytes [r row_bytes, (r + 1) row_bytes) of data, row_bytes = ceil(row_bits / 32) * 4, so a row's address is arithmetic and
// no workgroup waits for another.  Neither codes nor scale factors, X, t or thr reach HBM.
//
// Behind the search lane j holds band j's meta word and extremes of both signals of the pair.  Per signal:
//   width     31 for sf = -128, 0 for an empty band, else the bit length of max(zz(q(xmax)), zz(q(xmin))) at the band's scale
//             factor -- band_bits' arithmetic (ac_rate_dev.h), which is what k_pack finds from the codes;
//   positions one wave-wide scan over the lanes of (stored << 16) | w_j len_j, as parse_strip_p (ac_fast_inv_p_dev.h) does on
//             the decode side; lane 63's inclusive sum is the row's length, so bits_r costs no further reduction;
//   fits      bits_r <= 8 row_bytes.  A row that does not fit becomes the marked row: every width 31, nothing stored;
//   record    (first code bit - e_j first bin << 13) | (sf byte << 5) | width per band, e_j = the width of a band that stores:
//             bin i of band j starts at (record >> 13) + e_j i.
// Both rows are staged in the 4 KB of the wave's buffer below QSLOT_OFF, which the masking model is done with when
// psy_stage returns (its entry table, the first 1 KB, is read for the last time by the threshold emit) -- two rows of
// kPackRowsMaxBits / 8 = 2 KB.  The records live behind the search's slots.  Widths and scale factors are ORed in by the
// band's lane, codes from the row still in registers: a lane's bins 2g and 2g + 1 of one signal are neighbouring fields
// whether or not they share a band, and go in as one field of at most 32 bits.  The wave then stores row_bytes / 4 dwords
// per row, lane l taking words l, l + 64, ..., and lane 0 the fits bytes.
#pragma once
#include "ac_fast_quant_dev.h"

namespace ac {
namespace {

static_assert(kPackRowsMaxBits % 32 == 0 && 2 * (kPackRowsMaxBits / 8) <= QSLOT_OFF, "two staged rows below the search's slots");
constexpr int QSTAGE1_OFF = kPackRowsMaxBits / 8;   // the second signal's staged row
constexpr int QREC_OFF = QKN_OFF + 512;             // [64 bands][2 signals] int: the band records
static_assert(QREC_OFF + 512 <= S8_OFF, "the records lie inside the intensity image");

struct PackOut {
  uint8_t* data;   // [B F C row_bytes]
  uint8_t* fits;   // [B, F, C]
  int row_bytes;
};

__device__ __forceinline__ bool qp_stores(uint32_t w) { return w - 1u < 16u; }   // widths 1 .. 16 store an sf and codes

// the width field of a band with this meta word and extremes at scale factor s: band_bits' w (ac_rate_dev.h)
__device__ __forceinline__ uint32_t band_width_at(int meta, int kx, int kn, int s) {
  const float r = quant_inv_step(s);
  const uint32_t z = max(zigzag(qcode(key_value(kx), r)), zigzag(qcode(key_value(kn), r)));
  const uint32_t w = z ? 32u - (uint32_t)__builtin_clz(z) : 0u;
  return meta == 0 ? 0u : meta < 0 ? 31u : w;
}
// ORs the field v into bit p of the staged row st: at most two words
__device__ __forceinline__ void qp_put(uint32_t* st, uint32_t p, uint32_t v) {
  const uint64_t win = (uint64_t)v << (p & 31u);
  const uint32_t lo = (uint32_t)win, hi = (uint32_t)(win >> 32);
  if (lo) atomicOr(&st[p >> 5], lo);
  if (hi) atomicOr(&st[(p >> 5) + 1], hi);
}

template <int R, int CMODE, int SPREAD>
struct PackStage : QuantStage<R, CMODE, SPREAD, true> {
  using Q = QuantStage<R, CMODE, SPREAD, true>;
  static constexpr int M = Q::M;
  PackOut po;
  // loop invariants, per lane and in vector registers as QuantStage's: the lane's first word in slot 0 of data, the fits
  // bytes, words per slot, and the first bin of band `lane`
  uint32_t* data_l;
  uint8_t* fits_l;
  uint32_t nw_l;
  uint32_t first;

  __device__ __forceinline__ void init(int lane) {
    Q::init(lane);
    data_l = reinterpret_cast<uint32_t*>(po.data) + lane;
    fits_l = po.fits;
    nw_l = (uint32_t)po.row_bytes >> 2;
    first = (uint32_t)this->q.off[lane];
    asm volatile("" : "+v"(data_l), "+v"(fits_l), "+v"(nw_l), "+v"(first));
  }

  // band `lane` of one signal at the row's offset k: its width and scale factor into the staged row st, its record into
  // rec[2 lane]; returns whether the row fits max_bits (wave-uniform)
  __device__ __forceinline__ bool band_fields(int meta, int kx, int kn, int k, uint32_t L, uint32_t max_bits, uint32_t* st,
                                              int* rec, int lane) const {
    const int s = band_sf(meta, k);
    uint32_t w = band_width_at(meta, kx, kn, s);
    const uint32_t v = qp_stores(w) ? (1u << 16) | (w * L) : 0u;   // (code bits of a row <= 16 N = 2^14)
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += up;
    }
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    const uint32_t cbase = 5u * M + 8u * (total >> 16);   // first code bit
    const bool fits = cbase + (total & 0xffffu) <= max_bits;
    uint32_t ex = incl - v;
    if (!fits) {   // the marked row
      w = 31u;
      ex = 0u;
    }
    const uint32_t e = qp_stores(w) ? w : 0u;
    qp_put(st, 5u * (uint32_t)lane, w);
    if (e) qp_put(st, 5u * M + 8u * (ex >> 16), (uint32_t)(uint8_t)s);
    const int base = (int)(cbase + (ex & 0xffffu)) - (int)(e * in_loop(first));
    rec[2 * lane] = (int)(((uint32_t)base << 13) | ((uint32_t)(uint8_t)s << 5) | w);
    return fits;
  }
  // the codes of bins i and i + 1 of one signal (records re, ro of their bands) into the staged row: one field
  static __device__ __forceinline__ void code_fields(uint32_t* st, int re, int ro, float xe, float xo, uint32_t i) {
    const uint32_t we = (uint32_t)re & 31u, wo = (uint32_t)ro & 31u;
    const uint32_t ee = qp_stores(we) ? we : 0u, eo = qp_stores(wo) ? wo : 0u;
    const uint32_t ze = ee ? zigzag(qcode(xe, quant_inv_step((int)(int8_t)((uint32_t)re >> 5)))) : 0u;
    const uint32_t zo = eo ? zigzag(qcode(xo, quant_inv_step((int)(int8_t)((uint32_t)ro >> 5)))) : 0u;
    // bin i + 1 follows bin i: in the same band, or first of the next one that holds bins
    const uint32_t p = (uint32_t)((re >> 13) + (int)(ee * i));
    qp_put(st, p, ze | (zo << ee));
  }

  // the masking model on the frame in `row`, the offset search, then the packed rows of the pair (t0, t1: their row numbers)
  __device__ __forceinline__ void frame(const FwdArgs& a, const v4f (&row)[R], char* lds, char* buf, const uint32_t* pimg,
                                        const PsyLane<R>& pc, int lane, const Pair& pq, size_t, size_t, size_t t0,
                                        size_t t1) const {
    // every address the frame still needs, per lane and in vector registers, before the masking model (see QuantStage::frame)
    const size_t rw = (size_t)__builtin_amdgcn_readfirstlane((int)nw_l);
    uint32_t* d0 = data_l + t0 * rw;
    uint32_t* d1 = data_l + t1 * rw;
    uint8_t* f0 = fits_l + t0;
    uint8_t* f1 = fits_l + t1;
    asm volatile("" : "+v"(d0), "+v"(d1), "+v"(f0), "+v"(f1));
    typename Q::Emit e{*this, row, buf, lane, nullptr, nullptr, pq.has1, a.C};
    v2f tt;
    v4f th[R];
    psy_stage<R, true, true, SPREAD, false, typename Q::Emit&>(row, lds, buf, pimg, pc, this->pp, lane, tt, th, e);
    *reinterpret_cast<int2*>(buf + QKX_OFF + 8 * lane) = make_int2(INT_MIN, INT_MIN);
    *reinterpret_cast<int2*>(buf + QKN_OFF + 8 * lane) = make_int2(INT_MAX, INT_MAX);
#pragma unroll
    for (int k = 0; k < QSLOT_OFF / 1024; ++k) *reinterpret_cast<v4f*>(buf + 1024 * k + 16 * lane) = v4f{0.f, 0.f, 0.f, 0.f};
    wave_sync();
    this->extremes(row, buf);
    wave_sync();
    uint32_t* st0 = reinterpret_cast<uint32_t*>(buf);
    uint32_t* st1 = reinterpret_cast<uint32_t*>(buf + QSTAGE1_OFF);
    int* rec = reinterpret_cast<int*>(buf + QREC_OFF);
    const bool two = CMODE == 0 || pq.has1;
    bool fit0, fit1 = false;
    {
      const int2 kt = *reinterpret_cast<const int2*>(buf + QSLOT_OFF + 8 * lane);
      const int2 kx = *reinterpret_cast<const int2*>(buf + QKX_OFF + 8 * lane);
      const int2 kn = *reinterpret_cast<const int2*>(buf + QKN_OFF + 8 * lane);
      const uint32_t lk = in_loop(this->len);
      const int L = (int)(lk & 0x7ffu);
      const int m0 = band_meta<true>(L, kt.x), m1 = band_meta<true>(L, kt.y);
      const int rb = __builtin_amdgcn_readlane((int)(lk >> 11), 0), k0 = __builtin_amdgcn_readlane((int)(lk >> 11), 1) - kRateMaxOffset;
      const uint32_t max_bits = 32u * (uint32_t)__builtin_amdgcn_readfirstlane((int)nw_l);
      const int off0 = Q::row_offset(m0, kx.x, kn.x, rb, k0);
      fit0 = band_fields(m0, kx.x, kn.x, off0, (uint32_t)L, max_bits, st0, rec, lane);
      if (two) {
        const int off1 = Q::row_offset(m1, kx.y, kn.y, rb, k0);
        fit1 = band_fields(m1, kx.y, kn.y, off1, (uint32_t)L, max_bits, st1, rec + 1, lane);
      }
    }
    wave_sync();
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const uint32_t w = in_loop(this->bw[i]);
      const int2 re = *reinterpret_cast<const int2*>(buf + QREC_OFF + 8 * (w & 0xffffu));
      const int2 ro = *reinterpret_cast<const int2*>(buf + QREC_OFF + 8 * (w >> 16));
      const v4f x = row[i];
      const uint32_t bin = (uint32_t)(128 * i + 2 * lane);
      code_fields(st0, re.x, ro.x, x.x, x.z, bin);
      if (two) code_fields(st1, re.y, ro.y, x.y, x.w, bin);
    }
    wave_sync();
    const int nw = __builtin_amdgcn_readfirstlane((int)nw_l);
#pragma unroll 1
    for (int k = 0; k < nw; k += 64) {
      if (k + lane < nw) {
        d0[k] = st0[k + lane];
        if (two) d1[k] = st1[k + lane];
      }
    }
    if (lane == 0) {
      *f0 = fit0 ? 1 : 0;
      if (two) *f1 = fit1 ? 1 : 0;
    }
    wave_sync();
  }
};

// k_fwd_fast_qb with the packer behind the search: data and fits are all it writes
template <int CMODE, int SPREAD>
__global__ __launch_bounds__(AC_WAVES_PSY * 64, 2) void k_fwd_fast_qp(FwdArgs a, QuantOut q, PackOut po, int row_bits, int kmin) {
  __shared__ __attribute__((aligned(16))) char lds[fwd_lds_bytes<8, true, AC_WAVES_PSY, SPREAD>()];
  PackStage<8, CMODE, SPREAD> qz;
  // what the launcher fixes for this kernel, as constants: no tensor of the encode or the quantiser is written
  q.codes = nullptr;
  q.sf = nullptr;
  qz.q = q;
  qz.po = po;
  qz.pp = a.psy;
  qz.row_bits = row_bits;
  qz.kmin = kmin;
  a.C = CMODE == 0 ? 2 : 1;
  a.X = a.t = a.thr = nullptr;
  a.prev_block = nullptr;
  a.state_out = nullptr;
  a.noisy = a.dbn = nullptr;
  fwd_fast_body<8, CMODE, true, AC_WAVES_PSY, 0, SPREAD, false, PackStage<8, CMODE, SPREAD>>(a, lds, (int)blockIdx.x, (int)gridDim.x, qz);
}

// k_fwd_fast_qp on a chunk of a stream (instantiated in ac_fast_fwd_qps.hip): F == Kin, a.prev_block is block -1 of every
// signal and the wave that loads block Kin - 1 stores it to a.state_out, as k_fwd_fast does for ac_stream_encode.  A kernel
// of its own, so that the one-shot instances keep their registers and their text.
template <int CMODE, int SPREAD>
__global__ __launch_bounds__(AC_WAVES_PSY * 64, 2) void k_fwd_fast_qps(FwdArgs a, QuantOut q, PackOut po, int row_bits, int kmin) {
  __shared__ __attribute__((aligned(16))) char lds[fwd_lds_bytes<8, true, AC_WAVES_PSY, SPREAD>()];
  PackStage<8, CMODE, SPREAD> qz;
  q.codes = nullptr;
  q.sf = nullptr;
  qz.q = q;
  qz.po = po;
  qz.pp = a.psy;
  qz.row_bits = row_bits;
  qz.kmin = kmin;
  a.C = CMODE == 0 ? 2 : 1;
  a.X = a.t = a.thr = nullptr;
  a.noisy = a.dbn = nullptr;
  fwd_fast_body<8, CMODE, true, AC_WAVES_PSY, 0, SPREAD, false, PackStage<8, CMODE, SPREAD>>(a, lds, (int)blockIdx.x, (int)gridDim.x, qz);
}

}  // namespace
}  // namespace ac
