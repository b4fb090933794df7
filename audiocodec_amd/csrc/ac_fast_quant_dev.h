// The quantiser as the last stage of the fused encode at filters_n = 1024 (k_fwd_fast_q, instantiated in
// ac_fast_fwd_q.hip): fwd_fast_body (ac_fast_fwd_dev.h) with QuantStage as its QUANT.  A frame's spectrum row stays in the
// wave's registers across the masking model; the threshold row is consumed granule by granule as psy_stage's entry lookup
// emits it and is never held.  codes and sf equal k_quantize (ac_quant.hip) on the X and thr of k_fwd_fast bit for bit:
// the arithmetic is the one definition of ac_quant_dev.h / ac_band_dev.h.
//
// Layout the reduction rests on: lane l holds granules l + 64 i, a granule being bins 2g, 2g + 1 of both signals of the
// pair, so register step i covers 128 consecutive bins across the wave and the band of the even bins is monotone along the
// lanes: a band is a run of lanes (band_runs).  A lane folds the key of its odd bin into the even bin's where both lie in
// one band; where they do not, the odd bin is the first bin of its band inside this step and goes to that band's slot on its
// own (no two lanes of a step do so for the same band).  Run heads fold into 64 x 2 integer slots with ds_min.  The slots,
// and the inverse steps behind them, live in the wave's 8 KB intensity image, which the masking model is done with once the
// entry table (the first 1 KB of the region) is written.
//
// BUDGET (k_fwd_fast_qb, instantiated in ac_fast_fwd_qb.hip): rate control in the same launch.  Behind
// the masking model the wave adds the other two statistics of ac_rate_dev.h -- the largest and smallest X key per band and
// signal, reduced from the row in registers over the same runs into two more slot arrays -- and, lane j holding band j's
// meta word and extremes, bisects [kmin, 254] once per signal of the pair as k_quantize_budget does: band_bits per lane,
// wave_sum for the row.  codes and sf equal k_quantize_budget on the X and thr of k_fwd_fast bit for bit.
//
// PackStage (ac_fast_fwd_qp_dev.h; k_fwd_fast_qp) derives from the BUDGET form and packs the rows behind the search.
#pragma once
#include "ac_band_dev.h"
#include "ac_fast_fwd_dev.h"
#include "ac_rate_dev.h"

namespace ac {
namespace {

constexpr int QSLOT_OFF = 4096;           // [64 bands][2 signals] int: smallest threshold key of the band
constexpr int QINV_OFF = QSLOT_OFF + 512; // [64 bands][2 signals] float: inverse step, NaN for sf = -128
constexpr int QKX_OFF = QINV_OFF + 512;   // [64 bands][2 signals] int: largest X key of the band (BUDGET)
constexpr int QKN_OFF = QKX_OFF + 512;    // [64 bands][2 signals] int: smallest X key of the band (BUDGET)

struct QuantOut {
  int16_t* codes;            // [B, F, N, C]
  int8_t* sf;                // [B, F, M, C], M = 64
  const uint16_t* band;      // ac_psy_plan::d_qband: band of every bin
  const int32_t* off;        // ac_psy_plan::d_qoff: band offsets [M + 1]
};

// the plan's row budget (ac_psy_plan_with_row_budget) and what the search keeps per lane
struct QuantBudget {
  int row_bits, kmin;
  uint32_t len;   // one register for all three: bins of band `lane` in bits 0-10; above them row_bits (lane 0; at most 2^20,
                  // beyond any row's length) and kmin + 254 (lane 1)
};
struct NoQuantBudget {};

template <int R, int CMODE, int SPREAD, bool BUDGET = false>
struct QuantStage : std::conditional<BUDGET, QuantBudget, NoQuantBudget>::type {
  static_assert(CMODE == 0 || CMODE == 2, "quantised spectra: mono / stereo");
  static constexpr int M = 64;   // lane j = band j
  QuantOut q;
  // frame-invariant, per lane: bands of bins 2g (low half) and 2g + 1, g = 64 i + lane; the runs of the even bins' bands
  // along the wave, one byte per step (bits 0-5: same[k], bit 6: head); whether band `lane` is empty
  uint32_t bw[R];
  uint32_t rw[R / 4];
  uint32_t empty;
  // loop invariants of the frame loop, held in vector registers (see frame()): the lane's granule in row 0 of codes, its
  // band's byte in row 0 of sf, and the masking model's parameters
  int16_t* codes_l;
  int8_t* sf_l;
  PsyParams pp;

  __device__ __forceinline__ void init(int lane) {
#pragma unroll
    for (int i = 0; i < R / 4; ++i) rw[i] = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int g = 64 * i + lane;
      bw[i] = reinterpret_cast<const uint32_t*>(q.band)[g];
      const BandRuns r = band_runs(q.band, 2 * g, 128 * R, lane);
      uint32_t m = r.head ? 64u : 0u;
#pragma unroll
      for (int k = 0; k < 6; ++k) m |= r.same[k] ? (1u << k) : 0u;
      rw[i >> 2] |= m << (8 * (i & 3));
    }
    empty = q.off[lane] == q.off[lane + 1] ? 1u : 0u;
    codes_l = q.codes + (CMODE == 0 ? 4 : 2) * lane;
    sf_l = q.sf + (CMODE == 0 ? 2 : 1) * lane;
    asm volatile("" : "+v"(codes_l), "+v"(sf_l), "+v"(pp.alpha), "+v"(pp.inv_alpha), "+v"(pp.drown));
    if constexpr (BUDGET) {
      const uint32_t hi = lane == 0 ? (uint32_t)min(this->row_bits, 1 << 20) : (uint32_t)(this->kmin + kRateMaxOffset);
      this->len = (uint32_t)(q.off[lane + 1] - q.off[lane]) | (hi << 11);
    }
  }
  __device__ __forceinline__ BandRuns runs(int i) const {
    // (unpacked inside the frame loop: hoisted, the masks of eight steps would not fit the scalar registers)
    const uint32_t m = in_loop(rw[i >> 2]) >> (8 * (i & 3));
    BandRuns r;
    r.key = (int)(bw[i] & 0xffffu);
    r.head = (m & 64u) != 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) r.same[k] = (m & (1u << k)) != 0;
    return r;
  }

  // EMIT of psy_stage: granule 64 i + lane of the threshold row goes to HBM where the caller asked for thr, and into the
  // band minima
  struct Emit {
    static constexpr bool pin_products = true;   // (psy_stage: the contraction choices of k_fwd_fast's instance)
    const QuantStage& s;
    const v4f (&row)[R];
    char* buf;
    int lane;
    float *thr0, *thr1;   // this lane's first granule in the pair's rows of thr (thr0 null: thr is not written)
    bool has1;
    int C;
    __device__ __forceinline__ void begin() {
      *reinterpret_cast<int2*>(buf + QSLOT_OFF + 8 * lane) = make_int2(INT_MAX, INT_MAX);
      wave_sync();
    }
    __device__ __forceinline__ void operator()(int i, const v4f& th) {
      if (thr0) {
        const v4f one[1] = {th};
        constexpr int step = (CMODE == 0 ? 256 : 128);   // floats per register step and signal row
        store_row<CMODE, 1>(thr0 + step * i, thr1 + step * i, C, has1, 0, one);
      }
      const v4f x = row[i];
      const uint32_t w = in_loop(s.bw[i]);
      const int je = (int)(w & 0xffffu), jo = (int)(w >> 16);
      const int ke0 = thr_key(x.x, th.x), ke1 = thr_key(x.y, th.y), ko0 = thr_key(x.z, th.z), ko1 = thr_key(x.w, th.w);
      const bool split = jo != je;
      const BandRuns r = s.runs(i);
      const int v0 = run_reduce(r, split ? ke0 : min(ke0, ko0), MinOp());
      const int v1 = run_reduce(r, split ? ke1 : min(ke1, ko1), MinOp());
      int* slot = reinterpret_cast<int*>(buf + QSLOT_OFF);
      if (r.head) {
        atomicMin(&slot[2 * je], v0);
        atomicMin(&slot[2 * je + 1], v1);
      }
      if (split) {
        atomicMin(&slot[2 * jo], ko0);
        atomicMin(&slot[2 * jo + 1], ko1);
      }
    }
  };

  // BUDGET: the largest and smallest X key per band and signal of the frame in `row` into the slots at QKX_OFF / QKN_OFF
  // (initialised by the caller), folded over the runs as Emit folds the threshold keys
  __device__ __forceinline__ void extremes(const v4f (&row)[R], char* buf) const {
    int* kxs = reinterpret_cast<int*>(buf + QKX_OFF);
    int* kns = reinterpret_cast<int*>(buf + QKN_OFF);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const v4f x = row[i];
      const uint32_t w = in_loop(bw[i]);
      const int je = (int)(w & 0xffffu), jo = (int)(w >> 16);
      const int ke0 = ordered_key(x.x), ke1 = ordered_key(x.y), ko0 = ordered_key(x.z), ko1 = ordered_key(x.w);
      const bool split = jo != je;
      const BandRuns r = runs(i);
      const int x0 = run_reduce(r, split ? ke0 : max(ke0, ko0), MaxOp());
      const int x1 = run_reduce(r, split ? ke1 : max(ke1, ko1), MaxOp());
      const int n0 = run_reduce(r, split ? ke0 : min(ke0, ko0), MinOp());
      const int n1 = run_reduce(r, split ? ke1 : min(ke1, ko1), MinOp());
      if (r.head) {
        atomicMax(&kxs[2 * je], x0);
        atomicMax(&kxs[2 * je + 1], x1);
        atomicMin(&kns[2 * je], n0);
        atomicMin(&kns[2 * je + 1], n1);
      }
      if (split) {
        atomicMax(&kxs[2 * jo], ko0);
        atomicMax(&kxs[2 * jo + 1], ko1);
        atomicMin(&kns[2 * jo], ko0);
        atomicMin(&kns[2 * jo + 1], ko1);
      }
    }
  }
  // BUDGET: the row's offset -- the smallest k in [kmin, 254] whose bits fit row_bits, else 254: the interval rule of
  // k_quantize_budget (ac_rate.hip).  Lane j holds band j's meta word and extremes; every value of the search is wave-uniform
  static __device__ __forceinline__ int row_offset(int meta, int kx, int kn, int row_bits, int kmin) {
    int lo = kmin, hi = kRateMaxOffset;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      const int bits = 5 * M + __builtin_amdgcn_readfirstlane(wave_sum(band_bits(meta, kx, kn, mid)));
      if (bits <= row_bits) hi = mid;
      else lo = mid + 1;
    }
    return lo;
  }

  // the masking model on the frame in `row`, then scale factors (lane j: band j) and codes
  __device__ __forceinline__ void frame(const FwdArgs& a, const v4f (&row)[R], char* lds, char* buf, const uint32_t* pimg,
                                        const PsyLane<R>& pc, int lane, const Pair& pq, size_t o0, size_t o1, size_t t0,
                                        size_t t1) const {
    // every address the frame still needs, per lane and in vector registers, before the masking model: the row offsets
    // are scalars, and the scale-factor search below leaves no scalar registers for them
    constexpr int GW = CMODE == 0 ? 4 : 2;   // elements of a granule in one signal's row
    float* thr0 = a.thr ? a.thr + o0 + GW * lane : nullptr;
    float* thr1 = a.thr ? a.thr + o1 + GW * lane : nullptr;
    int16_t* c0 = codes_l + o0;
    int16_t* c1 = codes_l + o1;
    // sf: stereo, the row [M][2] of the clip's frame (t0 = 2 (b F + n)); mono, one row [M] per signal (t0, t1 = b F + n)
    int8_t* f0 = CMODE == 0 ? sf_l + (t0 >> 1) * (size_t)(2 * M) : sf_l + t0 * (size_t)M;
    int8_t* f1 = CMODE == 0 ? f0 + 1 : sf_l + t1 * (size_t)M;
    float* tp0 = a.t ? a.t + t0 : nullptr;
    float* tp1 = a.t ? a.t + t1 : nullptr;
    asm volatile("" : "+v"(thr0), "+v"(thr1), "+v"(c0), "+v"(c1), "+v"(f0), "+v"(f1), "+v"(tp0), "+v"(tp1));
    Emit e{*this, row, buf, lane, thr0, thr1, pq.has1, a.C};
    v2f tt;
    v4f th[R];
    psy_stage<R, true, true, SPREAD, false, Emit&>(row, lds, buf, pimg, pc, pp, lane, tt, th, e);
    if (a.t && lane == 0) {
      *tp0 = tt.x;
      if (pq.has1) *tp1 = tt.y;
    }
    if constexpr (BUDGET) {
      *reinterpret_cast<int2*>(buf + QKX_OFF + 8 * lane) = make_int2(INT_MIN, INT_MIN);
      *reinterpret_cast<int2*>(buf + QKN_OFF + 8 * lane) = make_int2(INT_MAX, INT_MAX);
    }
    wave_sync();
    float* inv = reinterpret_cast<float*>(buf + QINV_OFF);
    if constexpr (BUDGET) {
      extremes(row, buf);
      wave_sync();
      const int2 kt = *reinterpret_cast<const int2*>(buf + QSLOT_OFF + 8 * lane);
      const int2 kx = *reinterpret_cast<const int2*>(buf + QKX_OFF + 8 * lane);
      const int2 kn = *reinterpret_cast<const int2*>(buf + QKN_OFF + 8 * lane);
      const uint32_t lk = in_loop(this->len);
      const int L = (int)(lk & 0x7ffu);
      const int m0 = band_meta<true>(L, kt.x), m1 = band_meta<true>(L, kt.y);
      const int rb = __builtin_amdgcn_readlane((int)(lk >> 11), 0), k0 = __builtin_amdgcn_readlane((int)(lk >> 11), 1) - kRateMaxOffset;
      const int off0 = row_offset(m0, kx.x, kn.x, rb, k0);
      store_sf(band_sf(m0, off0), f0, &inv[2 * lane]);
      if (CMODE == 0 || pq.has1) {
        const int off1 = row_offset(m1, kx.y, kn.y, rb, k0);
        store_sf(band_sf(m1, off1), f1, &inv[2 * lane + 1]);
      }
    } else {
      const int2 k = *reinterpret_cast<const int2*>(buf + QSLOT_OFF + 8 * lane);
      const bool none = in_loop(empty) != 0;
      const int q0 = band_scale_factor<true>(none, k.x), q1 = band_scale_factor<true>(none, k.y);
      store_sf(q0, f0, &inv[2 * lane]);
      if (CMODE == 0 || pq.has1) store_sf(q1, f1, &inv[2 * lane + 1]);
    }
    wave_sync();
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const uint32_t w = in_loop(bw[i]);
      const v2f re = *reinterpret_cast<const v2f*>(buf + QINV_OFF + 8 * (w & 0xffffu));
      const v2f ro = *reinterpret_cast<const v2f*>(buf + QINV_OFF + 8 * (w >> 16));
      const v4f x = row[i];
      if (CMODE == 0) {
        reinterpret_cast<s4*>(c0)[64 * i] =
            s4{code_or_zero(x.x, re.x), code_or_zero(x.y, re.y), code_or_zero(x.z, ro.x), code_or_zero(x.w, ro.y)};
      } else {
        reinterpret_cast<s2*>(c0)[64 * i] = s2{code_or_zero(x.x, re.x), code_or_zero(x.z, ro.x)};
        if (pq.has1) reinterpret_cast<s2*>(c1)[64 * i] = s2{code_or_zero(x.y, re.y), code_or_zero(x.w, ro.y)};
      }
    }
  }
};

template <int CMODE, int SPREAD>
__global__ __launch_bounds__(AC_WAVES_PSY * 64, 2) void k_fwd_fast_q(FwdArgs a, QuantOut q) {
  __shared__ __attribute__((aligned(16))) char lds[fwd_lds_bytes<8, true, AC_WAVES_PSY, SPREAD>()];
  QuantStage<8, CMODE, SPREAD> qz;
  qz.q = q;
  qz.pp = a.psy;
  // what the launcher fixes for this kernel, as constants: the frame loop is short of scalar registers
  a.C = CMODE == 0 ? 2 : 1;
  a.prev_block = nullptr;
  a.state_out = nullptr;
  a.noisy = a.dbn = nullptr;
  fwd_fast_body<8, CMODE, true, AC_WAVES_PSY, 0, SPREAD, false, QuantStage<8, CMODE, SPREAD>>(a, lds, (int)blockIdx.x, (int)gridDim.x, qz);
}

// ... with the row budget of the plan met in the same launch (QuantStage's BUDGET form)
template <int CMODE, int SPREAD>
__global__ __launch_bounds__(AC_WAVES_PSY * 64, 2) void k_fwd_fast_qb(FwdArgs a, QuantOut q, int row_bits, int kmin) {
  __shared__ __attribute__((aligned(16))) char lds[fwd_lds_bytes<8, true, AC_WAVES_PSY, SPREAD>()];
  QuantStage<8, CMODE, SPREAD, true> qz;
  qz.q = q;
  qz.pp = a.psy;
  qz.row_bits = row_bits;
  qz.kmin = kmin;
  a.C = CMODE == 0 ? 2 : 1;
  a.prev_block = nullptr;
  a.state_out = nullptr;
  a.noisy = a.dbn = nullptr;
  fwd_fast_body<8, CMODE, true, AC_WAVES_PSY, 0, SPREAD, false, QuantStage<8, CMODE, SPREAD, true>>(a, lds, (int)blockIdx.x, (int)gridDim.x, qz);
}

// (host) The launcher of every kernel of this family -- k_fwd_fast_q / qb / qp / qps and their 16-bit PCM forms, each in a
// unit of its own: the arguments and grid of prep_fwd_fast, QuantOut from the plan, then the instance of the call's channel
// count and spreading product through `launch(cmode, spread, grid, block, a, q)`, cmode and spread being
// std::integral_constant.  GATE[mono][split-bf16 spreading]: the instances the unit builds; `launch` is not instantiated
// for the others, so they are not compiled either (the unit's *_serves predicate keeps their calls away).
constexpr bool kEveryInstance[2][2] = {{true, true}, {true, true}};

template <const bool (&GATE)[2][2], typename Launch>
int launch_fwd_fast_quant_family(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, int iof, float* X, float* t,
                                 float* thr, float drown, int16_t* codes, int8_t* sf, const float* prev_block, float* state_out,
                                 int B, int Kin, int F, int C, Launch launch) {
  FwdArgs a;
  unsigned grid;
  const int st = prep_fwd_fast(p, psy, x, iof, X, t, thr, drown, prev_block, B, Kin, F, C, state_out, nullptr, nullptr, 0, a, grid);
  if (st) return st;
  QuantOut q;
  q.codes = codes;
  q.sf = sf;
  q.band = psy->d_qband;
  q.off = psy->d_qoff;
  auto one = [&](auto cmode, auto spread) {
    if constexpr (GATE[decltype(cmode)::value == 2][decltype(spread)::value == 2])
      launch(cmode, spread, dim3(grid), dim3(AC_WAVES_PSY * 64), a, q);
  };
  using std::integral_constant;
  if (C == 2) {
    if (psy->spread == 2) one(integral_constant<int, 0>(), integral_constant<int, 2>());
    else one(integral_constant<int, 0>(), integral_constant<int, 0>());
  } else {
    if (psy->spread == 2) one(integral_constant<int, 2>(), integral_constant<int, 2>());
    else one(integral_constant<int, 2>(), integral_constant<int, 0>());
  }
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace
}  // namespace ac
