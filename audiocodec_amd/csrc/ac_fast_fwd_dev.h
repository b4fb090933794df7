// Analysis of the wave-level kernels for filters_n = 1024 / 2048 (ac_fast_dev.h), with the fused masking model: the
// body and the k_fwd_fast template.  Instantiated in ac_fast_fwd.hip, which also runs the body in k_duplex_fast, and in
// ac_fast_fwd_q.hip (k_fwd_fast_q: the body with the quantiser as its last stage, ac_fast_quant_dev.h) and its siblings.
#pragma once
#include <cmath>
#include <cstdlib>

#include "ac_fast.h"
#include "ac_fast_psy_dev.h"

namespace ac {
namespace {

// ------------------------------------------------------------------------------------------------------
// analysis (+ fused epilogue)
// ------------------------------------------------------------------------------------------------------
struct FwdArgs {
  const void* x;             // [B, Kin*N, C] float32, or int16 PCM for the PCM16 kernels
  float* X;                  // [B, F, N, C]
  float* t;                  // [B, F, 1, C]   (PSY)
  float* thr;                // [B, F, N, C]   (PSY)
  const float* prev_block;   // [B, N, C] or null: block -1 of every signal (streaming analysis state)
  float* state_out;          // [B, N, C] or null: receives block Kin-1 of every signal (the next chunk's prev_block;
                             // a different buffer than prev_block: other waves still read that one)
  const float* tab;          // mdct tables (analysis image)
  PsyParams psy;
  // optional element-wise epilogues of the fused encode (EPI kernels): X + thr * Normal(0, 1/6) and amplitude_to_dB_norm(X),
  // both [B, F, N, C]; either may be null
  float* noisy;
  float* dbn;
  uint64_t noise_key;        // mix64(seed) of ac_add_noise
  int B, Kin, F, C;
  long long npairs, nsig;    // wave tasks per frame index (see Pair) and B * C
  int xcd;                   // 1: consecutive logical workgroups share an XCD (gridDim.x is a multiple of 8)
  int T;                     // > 0: workgroup g owns frames [g NW T, (g+1) NW T), wave w takes g NW T + w + NW t;
                             // 0: persistent waves, wave w of W takes frames w, w + W, ...
  long long nframes;         // npairs * F
  float pre_re, pre_im;      // PRE[e] / POST[e] of the analysis image (kernels that keep no pre-twiddles in LDS)
};

// Analysis is frame-independent: frame n of a channel pair needs blocks n-1 and n of the PCM, and a wave that loads
// both needs nothing from its neighbours.  Frames are dealt out in order -- workgroup g owns frames [g NW T, (g+1) NW T)
// and its wave w takes g NW T + w + NW t (or, with T = 0, persistent waves take w, w + W, ...) -- so at any moment the
// chip reads one contiguous window of the PCM and writes one contiguous window of each output tensor, which is what HBM
// rewards (tools/ubench_strips.hip: 10-15 % over per-wave strips); block n-1 is the block the neighbouring wave loads as
// its block n, so the second read is an L2 hit.
//
// Element e = lane + 64 r of the FFT input takes, from each block, the even sample of granule e + 256 (this lane,
// register (r + 4) & 7) and the odd sample of granule 767 - e (lane 63 - lane, register (3 - r) & 7).
// With (A, B) = COEF[e]:  carried part (block n-1) = B xe + A xo;  current part (block n) = B xo - A xe (r < 4),
// A xe - B xo (r >= 4)   (Princen-Bradley windows make the 2x2 fold blocks rotations).
// one LDS object: [NW wave buffers | table image | psy image | bf16 tiles of the spreading matrix (SPREAD > 0)]
// the matrix-core spreading kernels at 8 points per lane pay for their bf16 tiles with the pre-twiddle table, which
// they rebuild from the post-twiddles: the workgroup stays under 53 760 B, three to a CU
template <int R, bool PSY, int SPREAD>
constexpr bool fwd_nopre() { return (R == 8) && PSY && SPREAD > 0; }
template <int R, bool PSY, int NW, int SPREAD>
constexpr int fwd_lds_bytes() {
  return NW * (PSY ? WAVE_LDS_PSY : WAVE_LDS) + (fwd_nopre<R, PSY, SPREAD>() ? Geo<R>::I_LDS_NOPRE : Geo<R>::I_LDS) * 4 +
         (PSY ? PsyGeo<R>::PSY_LDS + mf_lds(SPREAD) : 0);
}
struct NoQuant {};
// the kernel's body: workgroup `bid` of `nblocks` (the kernel below passes blockIdx.x / gridDim.x; the streaming duplex
// kernel runs it on the first part of its grid), lds = fwd_lds_bytes() bytes of LDS, 16-byte aligned
// QUANT other than NoQuant (QuantStage, ac_fast_quant_dev.h): the frame's last stage is qz.frame() -- the masking model
// with the quantiser behind it -- and a.X, a.t, a.thr may each be null (not written)
template <int R, int CMODE, bool PSY, int NW, int IOF = 0, int SPREAD = 0, bool EPI = false, class QUANT = NoQuant>
__device__ __forceinline__ void fwd_fast_body(const FwdArgs& a, char* lds, const int bid, const int nblocks, QUANT qz = QUANT()) {
  static_assert(!EPI || (PSY && CMODE == 0 && IOF == 0), "the element-wise epilogues ride on the stereo float32 fused encode");
  constexpr bool QNT = !std::is_same<QUANT, NoQuant>::value;
  static_assert(!QNT || (PSY && !EPI && (IOF == 0 || IOF == 1) && R == 8),
                "the quantiser rides on the float32 / 16-bit PCM fused encode at 8 points per lane");
  using G = Geo<R>;
  constexpr int WSTRIDE = PSY ? WAVE_LDS_PSY : WAVE_LDS;
  constexpr bool NOPRE = fwd_nopre<R, PSY, SPREAD>();
  constexpr int TABF = NOPRE ? G::I_LDS_NOPRE : G::I_LDS;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  load_tables<NW, WSTRIDE, TABF, PsyGeo<R>::PL_LDS, PsyGeo<R>::PL_MF, mf_lds(SPREAD)>(lds, a.tab, PSY ? a.psy.tab : nullptr);
  char* buf = lds + wave * WSTRIDE;
  gtab_t tab = reinterpret_cast<const float*>(lds + NW * WSTRIDE);
  const uint32_t* pimg = reinterpret_cast<const uint32_t*>(lds + NW * WSTRIDE + TABF * 4);
  if (PSY) *reinterpret_cast<v2f*>(buf + ZERO_OFF) = v2f{0.f, 0.f};   // the gather lists' padding slot
  // (the kernels with element-wise epilogues are short of registers at the end of the masking model: they fetch the
  // lane's pass-1 twiddles per frame, beside the frame's PCM, instead of holding them across the loop)
  v2f p1[R];
  if constexpr (!EPI) load_p1<R>(a.tab, lane, p1);
  PsyLane<R> pc;
  if (PSY) pc = load_psy_lane<R>(a.psy.tab, lane, (uint32_t)(wave * WSTRIDE));
  if constexpr (QNT) qz.init(lane);
  int g = bid;
  if (a.xcd) g = (g & 7) * (nblocks >> 3) + (g >> 3);
  const int C = a.C;
  const size_t blk = (size_t)G::FN * C;   // floats per block / frame row over all channels
  // frame f = (pair, n); everything about it is wave-uniform and lives in scalar registers, advanced without divisions
  const long long stride = a.T > 0 ? (long long)NW : (long long)nblocks * NW;
  const long long f0 = (a.T > 0 ? (long long)g * NW * a.T : (long long)g * NW) + wave;
  int left = a.T > 0 ? a.T : 0x7fffffff;
  const long long dpair = stride / a.F;
  const int dn = (int)(stride % a.F);
  long long pair = f0 / a.F;
  int n = (int)(f0 % a.F);
  const long long npairs = a.npairs;
  using pcm_t = typename std::conditional<IOF != 0, int16_t, float>::type;
  const pcm_t* __restrict__ xin = static_cast<const pcm_t*>(a.x);
  const pcm_t* __restrict__ xstate = IOF != 0 ? nullptr : reinterpret_cast<const pcm_t*>(a.prev_block);
  // bfloat16 tensors (IOF 2) and 16-bit PCM under the quantiser (IOF 1 with QUANT: the k_fwd_fast_*16 kernels): the
  // streaming state stays float32 (a bfloat16 block, and pcm / 32768, are exact in it)
  constexpr bool FSTATE = IOF == 2 || (IOF == 1 && QNT);
  const float* __restrict__ fstate = FSTATE ? a.prev_block : nullptr;

  // loads block fn (WHICH 0) or block fn-1 (WHICH 1) of frame (pr, fn) in natural order.  A missing block (before the
  // first / after the last) is loaded from a neighbouring, valid address and zeroed when it is consumed (returns false),
  // so that the loads stay unconditional and nothing waits for them at the point of issue.
  auto issue_loads = [&](auto which, long long pr, int fn, v4f (&dst)[R]) -> bool {
    const Pair q = make_pair<CMODE>(pr, C, a.nsig);
    const pcm_t *s0, *s1;
    bool ok;
    if (decltype(which)::value == 0) {
      ok = fn < a.Kin;
      const int blkidx = ok ? fn : (a.Kin > 0 ? a.Kin - 1 : 0);
      s0 = xin + row_off(q.b0, a.Kin, blkidx, blk, q.c0);
      s1 = xin + row_off(q.b1, a.Kin, blkidx, blk, q.c1);
    } else {
      if constexpr (FSTATE) {
        if (fn < 1 && fstate) {   // block -1 = the stored float32 state
          load_row<CMODE, R>(fstate + row_off(q.b0, 1, 0, blk, q.c0), fstate + row_off(q.b1, 1, 0, blk, q.c1), C, q.has1, lane, dst);
          return true;
        }
      }
      ok = (fn >= 1) || xstate;
      if (fn >= 1 || !xstate) {
        const int blkidx = fn >= 1 ? fn - 1 : 0;
        s0 = xin + row_off(q.b0, a.Kin, blkidx, blk, q.c0);
        s1 = xin + row_off(q.b1, a.Kin, blkidx, blk, q.c1);
      } else {
        s0 = xstate + row_off(q.b0, 1, 0, blk, q.c0);
        s1 = xstate + row_off(q.b1, 1, 0, blk, q.c1);
      }
    }
    if (a.Kin == 0 && !(decltype(which)::value == 1 && fn == 0 && xstate)) {   // no PCM at all: any mapped address
      s0 = s1 = reinterpret_cast<const pcm_t*>(QNT ? static_cast<const void*>(a.tab) : static_cast<const void*>(a.X));
      ok = false;
    }
    if constexpr (IOF != 0) load_row_h<typename RowFmt<IOF>::type, CMODE, R>(s0, s1, C, q.has1, lane, dst);
    else load_row<CMODE, R>(s0, s1, C, q.has1, lane, dst);
    return ok;
  };
  constexpr std::integral_constant<int, 0> kCur{};
  constexpr std::integral_constant<int, 1> kPrv{};
  auto zero_row = [](v4f (&v)[R]) {
#pragma unroll
    for (int i = 0; i < R; ++i) v[i] = v4f{0.f, 0.f, 0.f, 0.f};
  };

  while (pair < npairs && left > 0) {
    const Pair pq = make_pair<CMODE>(pair, C, a.nsig);
    C2 z[R];
    if (R == 8) {
      // both blocks in flight together; one lane-reversal exchange for the odd halves of both:
      // previous block in [0, 4 KB), current block in [4 KB, 8 KB)
      v4f cb[R], pb[R];
      const bool cur_ok = issue_loads(kCur, pair, n, cb);
      if constexpr (EPI) load_p1<R>(a.tab, lane, p1);
      const bool prv_ok = issue_loads(kPrv, pair, n, pb);
      if (!cur_ok) zero_row(cb);   // edge frames only (wave-uniform)
      if (!prv_ok) zero_row(pb);
      if constexpr (IOF != 1 || QNT) {
        if (a.state_out && n == a.Kin - 1)   // streaming: the chunk's last block is the next chunk's block -1
          store_row<CMODE, R>(a.state_out + row_off(pq.b0, 1, 0, blk, pq.c0), a.state_out + row_off(pq.b1, 1, 0, blk, pq.c1),
                              C, pq.has1, lane, cb);
      }
      wave_sync();
      {
        char* w = buf + 8 * (63 - lane);
#pragma unroll
        for (int c = 0; c < R; ++c) {
          *reinterpret_cast<v2f*>(w + 512 * c) = v2f{pb[c].z, pb[c].w};
          *reinterpret_cast<v2f*>(w + 4096 + 512 * c) = v2f{cb[c].z, cb[c].w};
        }
      }
      wave_sync();
      const char* rd = buf + 8 * lane;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const v2f xop = *reinterpret_cast<const v2f*>(rd + 512 * ((R / 2 - 1 - r) & (R - 1)));
        const v2f xoc = *reinterpret_cast<const v2f*>(rd + 4096 + 512 * ((R / 2 - 1 - r) & (R - 1)));
        const v4f& gp = pb[(r + R / 2) & (R - 1)];
        const v4f& gc = cb[(r + R / 2) & (R - 1)];
        const v2f xep = v2f{gp.x, gp.y}, xec = v2f{gc.x, gc.y};
        const v2f ab = reinterpret_cast<const v2f*>(tab + G::I_COEF)[r * 64 + lane];
        const v2f carry = ab.y * xep + ab.x * xop;
        const v2f cur = (r < R / 2) ? (ab.y * xoc - ab.x * xec) : (ab.x * xec - ab.y * xoc);
        // element e = lane + 64 r: v[2e] + i v[N-1-2e]; for e < N/4 the real part comes from the previous block
        const C2 v = (r < R / 2) ? C2{carry, cur} : C2{cur, carry};
        if constexpr (NOPRE) {
          const C2 v0 = {v.re * a.pre_re - v.im * a.pre_im, v.re * a.pre_im + v.im * a.pre_re};
          z[r] = cmul(v0, reinterpret_cast<const v2f*>(tab + G::I_POST)[r * 64 + lane]);
        } else {
          z[r] = cmul(v, reinterpret_cast<const v2f*>(tab + G::I_PRE)[r * 64 + lane]);
        }
      }
    } else {
      // larger frames: one block at a time (registers), each with its own lane-reversal exchange
      v2f carry[R];
      {
        v4f pb[R];
        const bool prv_ok = issue_loads(kPrv, pair, n, pb);
        if (!prv_ok) zero_row(pb);
        v2f xo_in[R], xo[R];
#pragma unroll
        for (int c = 0; c < R; ++c) xo_in[c] = v2f{pb[c].z, pb[c].w};
        rev_exchange<R / 2 - 1, R>(buf, lane, xo_in, xo);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const v4f& gp = pb[(r + R / 2) & (R - 1)];
          const v2f ab = reinterpret_cast<const v2f*>(tab + G::I_COEF)[r * 64 + lane];
          carry[r] = ab.y * v2f{gp.x, gp.y} + ab.x * xo[r];
        }
      }
      v4f cb[R];
      const bool cur_ok = issue_loads(kCur, pair, n, cb);
      if (!cur_ok) zero_row(cb);
      if constexpr (IOF != 1 || QNT) {
        if (a.state_out && n == a.Kin - 1)
          store_row<CMODE, R>(a.state_out + row_off(pq.b0, 1, 0, blk, pq.c0), a.state_out + row_off(pq.b1, 1, 0, blk, pq.c1),
                              C, pq.has1, lane, cb);
      }
      v2f xo_in[R], xo[R];
#pragma unroll
      for (int c = 0; c < R; ++c) xo_in[c] = v2f{cb[c].z, cb[c].w};
      rev_exchange<R / 2 - 1, R>(buf, lane, xo_in, xo);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const v4f& gc = cb[(r + R / 2) & (R - 1)];
        const v2f xec = v2f{gc.x, gc.y};
        const v2f ab = reinterpret_cast<const v2f*>(tab + G::I_COEF)[r * 64 + lane];
        const v2f cur = (r < R / 2) ? (ab.y * xo[r] - ab.x * xec) : (ab.x * xec - ab.y * xo[r]);
        const C2 v = (r < R / 2) ? C2{carry[r], cur} : C2{cur, carry[r]};
        z[r] = cmul(v, reinterpret_cast<const v2f*>(tab + G::I_PRE)[r * 64 + lane]);
      }
    }
    fft_wave<R>(z, buf, tab, p1, lane);
    v4f row[R];
    {
      // bin k = lane + 64 j: X[2k] = Re (granule k, this lane), X[N-1-2k] = -Im (granule N/2-1-k, lane 63 - lane)
      v2f xe[R], xo_in[R], xo[R];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const C2 r = cmul_negim(z[j], reinterpret_cast<const v2f*>(tab + G::I_POST)[j * 64 + lane]);
        xe[j] = r.re;
        xo_in[j] = r.im;
      }
      rev_exchange<R - 1, R>(buf, lane, xo_in, xo);
#pragma unroll
      for (int i = 0; i < R; ++i) row[i] = v4f{xe[i].x, xe[i].y, xo[i].x, xo[i].y};
    }
    const size_t o0 = row_off(pq.b0, a.F, n, blk, pq.c0), o1 = row_off(pq.b1, a.F, n, blk, pq.c1);
    const size_t t0 = ((size_t)pq.b0 * a.F + (size_t)n) * C + pq.c0, t1 = ((size_t)pq.b1 * a.F + (size_t)n) * C + pq.c1;
    if constexpr (IOF == 2) {
      int16_t* Xh = reinterpret_cast<int16_t*>(a.X);
      store_row_h<Bf16Fmt, CMODE, R>(Xh + o0, Xh + o1, C, pq.has1, lane, row);
    } else if constexpr (QNT) {
      if (a.X) store_row<CMODE, R>(a.X + o0, a.X + o1, C, pq.has1, lane, row);
    } else {
      store_row<CMODE, R>(a.X + o0, a.X + o1, C, pq.has1, lane, row);
    }
    if constexpr (EPI) {
      if (a.dbn) {   // amplitude_to_dB_norm of the coefficients (psychoacoustic.py:87-100), from the registers
        v4f d[R];
#pragma unroll
        for (int i = 0; i < R; ++i) d[i] = v4f{db_of(row[i].x, 1), db_of(row[i].y, 1), db_of(row[i].z, 1), db_of(row[i].w, 1)};
        store_row<CMODE, R>(a.dbn + o0, a.dbn + o1, C, pq.has1, lane, d);
      }
    }
    // next frame of this wave
    pair += dpair;
    n += dn;
    if (n >= a.F) {
      n -= a.F;
      ++pair;
    }
    --left;
    if constexpr (PSY && QNT) {
      qz.frame(a, row, lds, buf, pimg, pc, lane, pq, o0, o1, t0, t1);
    } else if constexpr (PSY) {
      v2f tt;
      v4f th[R];
      if constexpr (IOF == 2) {
        // the masking model sees the spectrum the caller gets: the bfloat16-rounded coefficients
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const s2 lo = Bf16Fmt::enc2(row[i].x, row[i].y), hi = Bf16Fmt::enc2(row[i].z, row[i].w);
          row[i] = v4f{Bf16Fmt::dec(lo.x), Bf16Fmt::dec(lo.y), Bf16Fmt::dec(hi.x), Bf16Fmt::dec(hi.y)};
        }
      }
      bool emitted = false;
      if constexpr (EPI) {
        if (a.noisy) {
          // add_noise (psychoacoustic.py:150-167) on the frame: the coefficients are no longer in registers (the masking
          // model needed them all), so the row the wave stored a moment ago comes back from L2; each granule of the
          // threshold row is stored and turned into its noisy coefficients as it comes out of the entry lookup.  Element
          // pairs of the flattened tensor share one Box-Muller draw, exactly as in ac_add_noise (granule i4 = elements
          // 4 i4 .. 4 i4 + 3)
          NoisyEmit<R> emit;
          emit.X_row = reinterpret_cast<const v4f*>(a.X + o0) + lane;
          emit.thr_row = reinterpret_cast<v4f*>(a.thr + o0) + lane;
          emit.noisy_row = reinterpret_cast<v4f*>(a.noisy + o0) + lane;
          emit.i4base = (uint64_t)(o0 >> 2) + (uint64_t)lane;
          emit.key = a.noise_key;
          psy_stage<R, true, true, SPREAD, false, NoisyEmit<R>&>(row, lds, buf, pimg, pc, a.psy, lane, tt, th, emit);
          emitted = true;
        }
      }
      if (!emitted) psy_stage<R, true, true, SPREAD, IOF == 2>(row, lds, buf, pimg, pc, a.psy, lane, tt, th);
      if constexpr (IOF == 2) {
        int16_t* th_h = reinterpret_cast<int16_t*>(a.thr);
        int16_t* t_h = reinterpret_cast<int16_t*>(a.t);
        store_row_h<Bf16Fmt, CMODE, R>(th_h + o0, th_h + o1, C, pq.has1, lane, th);
        if (lane == 0) {
          const s2 e = Bf16Fmt::enc2(tt.x, tt.y);
          t_h[t0] = e.x;
          if (pq.has1) t_h[t1] = e.y;
        }
      } else {
        if (!emitted) store_row<CMODE, R>(a.thr + o0, a.thr + o1, C, pq.has1, lane, th);
        if (lane == 0) {
          a.t[t0] = tt.x;
          if (pq.has1) a.t[t1] = tt.y;
        }
      }
    }
  }
}

template <int R, int CMODE, bool PSY, int NW, int IOF = 0, int SPREAD = 0, bool EPI = false>
__global__ __launch_bounds__(NW * 64, (wpe<R, CMODE, PSY, SPREAD>())) void k_fwd_fast(FwdArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[fwd_lds_bytes<R, PSY, NW, SPREAD>()];
  fwd_fast_body<R, CMODE, PSY, NW, IOF, SPREAD, EPI>(a, lds, (int)blockIdx.x, (int)gridDim.x);
}

// (host) arguments and grid of the one-frame-per-wave analysis kernels (filters_n 1024 / 2048)
int prep_fwd_fast(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, int iof, float* X, float* t,
                  float* thr, float drown, const float* prev_block, int B, int Kin, int F, int C, float* state_out,
                  float* noisy, float* dbn, uint64_t seed, FwdArgs& a, unsigned& grid) {
  // combinations no kernel is instantiated for (ac_api_encode.hip routes them elsewhere; refuse rather than launch nothing)
  if ((iof == 2 && C > 2) || (psy && p->N == Geo<16>::FN && (C == 1 || (iof == 1 && C > 2)))) {
    set_error("internal: no wave-level analysis kernel for filters_n = %d, %d channels, io format %d%s", p->N, C, iof,
              psy ? ", fused masking model" : "");
    return AC_EUNSUPPORTED;
  }
  a.x = x;
  a.X = X;
  a.t = t;
  a.thr = thr;
  a.prev_block = prev_block;
  a.state_out = state_out;
  a.noisy = noisy;
  a.dbn = dbn;
  a.noise_key = mix64(seed);
  if ((noisy || dbn) && !fast_epilogue_supported(p, psy, iof, C)) {
    set_error("internal: no fused element-wise epilogue for this configuration");
    return AC_EUNSUPPORTED;
  }
  a.tab = p->d_fast;
  if (psy) a.psy = psy_params(psy, drown);
  else a.psy = PsyParams{nullptr, 0.f, 0.f, 0.f};
  a.B = B;
  a.Kin = Kin;
  a.F = F;
  a.C = C;
  a.nsig = (long long)B * C;
  a.npairs = (C == 2) ? (long long)B : (a.nsig + 1) / 2;
  a.nframes = a.npairs * F;
  {
    const double ang = -3.14159265358979323846 / (4.0 * p->N), sc = (double)p->N * 1.4142135623730951;   // 1 / (1 / (N sqrt 2))
    a.pre_re = (float)(std::cos(ang) * sc);
    a.pre_im = (float)(std::sin(ang) * sc);
  }
  // tuning hooks (read once): AC_XCD=1 groups consecutive workgroups per XCD; AC_FWD_T = frames per wave, workgroups
  // dispatched in order (default 4: measured 0.603 ms against 0.615 ms for persistent waves, B = 256, K = 468 -- fresh
  // workgroups keep the window of memory in flight contiguous); AC_FWD_T=0 = persistent waves, AC_WG_PER_CU per CU
  static const int xcd = [] { const char* e = getenv("AC_XCD"); return e ? atoi(e) : 0; }();
  static const int wgcu = [] { const char* e = getenv("AC_WG_PER_CU"); return e ? atoi(e) : 3; }();
  static const int tper = [] { const char* e = getenv("AC_FWD_T"); return e ? atoi(e) : 4; }();
  a.xcd = xcd;
  const int nw = psy ? AC_WAVES_PSY : AC_WAVES;
  // small launches (a streaming chunk of one clip): fewer frames per wave, so that the frames spread over the chip
  // instead of queueing behind each other in a few workgroups
  int tper_eff = tper;
  while (tper_eff > 1 && a.nframes < (long long)nw * tper_eff * p->cus * 2) tper_eff >>= 1;
  a.T = tper_eff;
  if (tper > 0) {
    // workgroups in eights (XCDs): ceil(ceil(nframes / per) / 8) = ceil(nframes / (8 per))
    const long long per8 = 8ll * nw * tper_eff;
    const int st = grid_for((a.nframes + per8 - 1) / per8 * 8, 1, &grid);
    if (st) return st;
  } else {
    grid = persistent_grid(p->cus, wgcu, a.nframes, nw);
  }
  return AC_OK;
}

}  // namespace
}  // namespace ac
