// Instances and launch ladders of the kernels that run the analysis body or the masking-model stage at filters_n = 1024 /
// 2048: k_fwd_fast (analysis, fused encode), k_duplex_fast (streaming duplex) and k_psy_fast (stand-alone tonality /
// threshold).  They share one object because they share instantiations of fwd_fast_body and psy_stage: these have internal
// linkage, the compiler's interprocedural passes look at all callers of such a function in the module before it is
// inlined, and apart the three families get other register allocations for 18 kernels than together (DESIGN_LOG.md 9).
#include "ac_fast_fwd_dev.h"
#include "ac_fast_inv_dev.h"

namespace ac {
namespace {

// Streaming duplex (BASELINE configs[4]): the analysis of chunk i + 1 and the synthesis of chunk i in ONE launch -- the
// first nfwd workgroups run the analysis body, the others the synthesis body.  A chunk of one clip is a few hundred wave
// tasks: two dependent launches of ~8 us each are latency, not bandwidth, and the two halves are independent.
template <int R, int CMODE, bool PSY, int NW, int SPREAD>
__global__ __launch_bounds__(NW * 64, (CMODE == 0 ? wpe<R, CMODE, PSY, SPREAD>() : 2)) void k_duplex_fast(FwdArgs fa, InvArgs ia, int nfwd) {
  constexpr int LF = fwd_lds_bytes<R, PSY, NW, SPREAD>(), LI = NW * WAVE_LDS + Geo<R>::TAB_LDS;
  __shared__ __attribute__((aligned(16))) char lds[LF > LI ? LF : LI];
  const int b = (int)blockIdx.x;   // (uniform per workgroup: the barriers inside the bodies stay consistent)
  if (b < nfwd) fwd_fast_body<R, CMODE, PSY, NW, 0, SPREAD, false>(fa, lds, b, nfwd);
  else inv_fast_body<R, CMODE, NW, 0>(ia, lds, b - nfwd, (int)gridDim.x - nfwd);
}

// ------------------------------------------------------------------------------------------------------
// stand-alone tonality / threshold on a spectrum in HBM: one wave per (b, frame, channel pair)
// ------------------------------------------------------------------------------------------------------
struct PsyArgs {
  const float* X;
  const float* t_in;
  float* t_out;
  float* thr;
  PsyParams psy;
  int C, F;
  long long nsig;     // B * C
  long long ntasks;   // npairs * F
};

template <int R, int CMODE, bool WANT_T, bool WANT_THR, int NW, int SPREAD = 0, int IOF = 0>
__global__ __launch_bounds__(NW * 64, (R == 8 ? AC_WPE : 2)) void k_psy_fast(PsyArgs a) {
  using P = PsyGeo<R>;
  __shared__ __attribute__((aligned(16))) char lds[NW * WAVE_LDS_PSY + P::PSY_LDS + mf_lds(SPREAD)];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t* pimg = reinterpret_cast<const uint32_t*>(lds + NW * WAVE_LDS_PSY);
  if (WANT_THR) load_tables<NW, WAVE_LDS_PSY, 0, P::PL_LDS, P::PL_MF, mf_lds(SPREAD)>(lds, nullptr, a.psy.tab);
  const long long task = (long long)blockIdx.x * NW + wave;
  if (task >= a.ntasks) return;
  char* buf = lds + wave * WAVE_LDS_PSY;
  if (WANT_THR) *reinterpret_cast<v2f*>(buf + ZERO_OFF) = v2f{0.f, 0.f};
  const int f = (int)(task % a.F);
  const int C = a.C;
  const Pair pq = make_pair<CMODE>(task / a.F, C, a.nsig);
  const bool has1 = pq.has1;
  const size_t blk = (size_t)P::FN * C;
  const size_t o0 = row_off(pq.b0, a.F, f, blk, pq.c0), o1 = row_off(pq.b1, a.F, f, blk, pq.c1);
  const size_t t0 = ((size_t)pq.b0 * a.F + (size_t)f) * C + pq.c0, t1 = ((size_t)pq.b1 * a.F + (size_t)f) * C + pq.c1;
  v4f row[R], th[R];
  if constexpr (IOF == 2) {
    const int16_t* Xh = reinterpret_cast<const int16_t*>(a.X);
    load_row_h<Bf16Fmt, CMODE, R>(Xh + o0, Xh + o1, C, has1, lane, row);
  } else {
    load_row<CMODE, R>(a.X + o0, a.X + o1, C, has1, lane, row);
  }
  v2f tt = {0.f, 0.f};
  if (!WANT_T) {
    if constexpr (IOF == 2) {
      const int16_t* th_in = reinterpret_cast<const int16_t*>(a.t_in);
      tt.x = Bf16Fmt::dec(th_in[t0]);
      tt.y = has1 ? Bf16Fmt::dec(th_in[t1]) : 0.f;
    } else {
      tt.x = a.t_in[t0];
      tt.y = has1 ? a.t_in[t1] : 0.f;
    }
  }
  PsyLane<R> pc;
  if (WANT_THR) pc = load_psy_lane<R>(a.psy.tab, lane, (uint32_t)(wave * WAVE_LDS_PSY));
  psy_stage<R, WANT_T, WANT_THR, SPREAD, IOF == 2>(row, lds, buf, pimg, pc, a.psy, lane, tt, th);
  if constexpr (IOF == 2) {
    if (WANT_T && lane == 0) {
      int16_t* t_h = reinterpret_cast<int16_t*>(a.t_out);
      const s2 e = Bf16Fmt::enc2(tt.x, tt.y);
      t_h[t0] = e.x;
      if (has1) t_h[t1] = e.y;
    }
    if (WANT_THR) {
      int16_t* th_h = reinterpret_cast<int16_t*>(a.thr);
      store_row_h<Bf16Fmt, CMODE, R>(th_h + o0, th_h + o1, C, has1, lane, th);
    }
  } else {
    if (WANT_T && lane == 0) {
      a.t_out[t0] = tt.x;
      if (has1) a.t_out[t1] = tt.y;
    }
    if (WANT_THR) store_row<CMODE, R>(a.thr + o0, a.thr + o1, C, has1, lane, th);
  }
}

}  // namespace

// the element-wise epilogues (EPI kernels) serve stereo float32 input at 8 points per lane (filters_n = 1024)
bool fast_epilogue_supported(const ac_mdct_plan* p, const ac_psy_plan* psy, int iof, int C) {
  // (the plain-bf16 matrix-core form of the spreading product would spill three registers here: it takes the un-fused path)
  return psy != nullptr && p->N == Geo<8>::FN && iof == 0 && C == 2 && psy->spread != 1;
}

template <int R, int IOF>
static void launch_fwd_R(const FwdArgs& a, bool psy, int spread, int C, unsigned grid, hipStream_t s) {
  constexpr bool PCM16 = IOF == 1;
  if constexpr (R == 8 && IOF == 0) {
    if (psy && C == 2 && (a.noisy || a.dbn)) {
      const dim3 blk(AC_WAVES_PSY * 64);
      if (spread == 2) hipLaunchKernelGGL((k_fwd_fast<R, 0, true, AC_WAVES_PSY, 0, 2, true>), dim3(grid), blk, 0, s, a);
      else hipLaunchKernelGGL((k_fwd_fast<R, 0, true, AC_WAVES_PSY, 0, 0, true>), dim3(grid), blk, 0, s, a);
      return;
    }
  }
  if constexpr (IOF == 2) {
    // bfloat16 tensors: stereo and mono kernels (other channel counts are served by the LDS-FFT tier, see ac_api_quant.hip)
    if (psy) {
      const dim3 blk(AC_WAVES_PSY * 64);
      if (C == 2) hipLaunchKernelGGL((k_fwd_fast<R, 0, true, AC_WAVES_PSY, 2>), dim3(grid), blk, 0, s, a);
      else if constexpr (R == 8) hipLaunchKernelGGL((k_fwd_fast<R, 2, true, AC_WAVES_PSY, 2>), dim3(grid), blk, 0, s, a);
      return;
    }
    const dim3 blk(AC_WAVES * 64);
    if (C == 2) hipLaunchKernelGGL((k_fwd_fast<R, 0, false, AC_WAVES, 2>), dim3(grid), blk, 0, s, a);
    else hipLaunchKernelGGL((k_fwd_fast<R, 2, false, AC_WAVES, 2>), dim3(grid), blk, 0, s, a);
    return;
  } else {
  if (psy) {
    const dim3 blk(AC_WAVES_PSY * 64);
    // the matrix-core forms of the spreading product serve the stereo kernels (float32 or 16-bit PCM input); the others
    // keep the f32 product
    if (C == 2 && spread == 1) hipLaunchKernelGGL((k_fwd_fast<R, 0, true, AC_WAVES_PSY, IOF, 1>), dim3(grid), blk, 0, s, a);
    else if (C == 2 && spread == 2) hipLaunchKernelGGL((k_fwd_fast<R, 0, true, AC_WAVES_PSY, IOF, 2>), dim3(grid), blk, 0, s, a);
    else if (C == 2) hipLaunchKernelGGL((k_fwd_fast<R, 0, true, AC_WAVES_PSY, IOF>), dim3(grid), blk, 0, s, a);
    else if (C == 1) {
      // (R = 16: the caller runs transform and masking model as two launches, see encode_fused in ac_api_encode.hip)
      if constexpr (R == 8) {
        if (spread == 1) hipLaunchKernelGGL((k_fwd_fast<R, 2, true, AC_WAVES_PSY, IOF, 1>), dim3(grid), blk, 0, s, a);
        else if (spread == 2) hipLaunchKernelGGL((k_fwd_fast<R, 2, true, AC_WAVES_PSY, IOF, 2>), dim3(grid), blk, 0, s, a);
        else hipLaunchKernelGGL((k_fwd_fast<R, 2, true, AC_WAVES_PSY, IOF>), dim3(grid), blk, 0, s, a);
      }
    } else {
      if constexpr (R == 8 || !PCM16) hipLaunchKernelGGL((k_fwd_fast<R, 1, true, AC_WAVES_PSY, IOF>), dim3(grid), blk, 0, s, a);
    }
    return;
  }
  const dim3 blk(AC_WAVES * 64);
  if (C == 2) hipLaunchKernelGGL((k_fwd_fast<R, 0, false, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a);
  else if (C == 1) hipLaunchKernelGGL((k_fwd_fast<R, 2, false, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a);
  else hipLaunchKernelGGL((k_fwd_fast<R, 1, false, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a);
  }
}

int launch_fwd_fast(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, int iof, float* X, float* t,
                    float* thr, float drown, const float* prev_block, int B, int Kin, int F, int C, hipStream_t s,
                    float* state_out, float* noisy, float* dbn, uint64_t seed) {
  if (B <= 0 || C <= 0 || F <= 0) return AC_OK;
  if (fast_mdct_frames_per_wave(p->N) > 1) {
    if (noisy || dbn || !fast_multi_serves(p, C, iof, Kin) || (psy && !(fast_multi_fuses(p, psy, C, iof, Kin) && t && thr))) {
      set_error("internal: no wave-level analysis kernel for filters_n = %d, %d channels, io format %d here", p->N, C, iof);
      return AC_EUNSUPPORTED;
    }
    return launch_fwd_multi(p, psy, x, iof, X, psy ? t : nullptr, psy ? thr : nullptr, drown, prev_block, state_out, B, Kin, F, C, s);
  }
  FwdArgs a;
  unsigned grid;
  const int st = prep_fwd_fast(p, psy, x, iof, X, t, thr, drown, prev_block, B, Kin, F, C, state_out, noisy, dbn, seed, a, grid);
  if (st) return st;
  const int spread = psy ? psy->spread : 0;
  if (p->N == Geo<8>::FN) {
    if (iof == 2) launch_fwd_R<8, 2>(a, psy != nullptr, spread, C, grid, s);
    else if (iof == 1) launch_fwd_R<8, 1>(a, psy != nullptr, spread, C, grid, s);
    else launch_fwd_R<8, 0>(a, psy != nullptr, spread, C, grid, s);
  } else if (iof == 2) launch_fwd_R<16, 2>(a, psy != nullptr, spread, C, grid, s);
  else if (iof == 1) launch_fwd_R<16, 1>(a, psy != nullptr, spread, C, grid, s);
  else launch_fwd_R<16, 0>(a, psy != nullptr, spread, C, grid, s);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

// ---- streaming duplex: analysis of one chunk and synthesis of another in one launch (k_duplex_fast) ----
// Served: float32, mono / stereo, filters_n 1024 / 2048, without the masking model or (1024, stereo) with the fused
// one in its f32 / split-bf16 spreading forms -- and only launches that leave the chip partly idle on their own: up to
// 256 wave tasks per CU over both halves (64 stereo streams in chunks of 256 blocks: 116 us per chunk against 124 for
// the chain; one stream: 11.6 against 18 -- a chunk's two dependent launches are latency there).  Beyond that each launch
// fills the chip by itself.  AC_DUPLEX_MAX_TASKS overrides the limit (tuning hook).
bool fast_duplex_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int B, int C, int k_fwd, int k_inv) {
  static const int off = [] { const char* e = getenv("AC_NO_DUPLEX"); return e ? atoi(e) : 0; }();   // tuning hook
  if (off || fast_mdct_frames_per_wave(p->N) != 1 || (C != 1 && C != 2) || k_fwd < 1 || k_inv < 1) return false;
  if (psy && !(p->N == Geo<8>::FN && C == 2 && psy->fast && psy->spread != 1)) return false;
  const long long pairs = (C == 2) ? B : (B + 1) / 2;
  static const long long max_tasks = [] { const char* e = getenv("AC_DUPLEX_MAX_TASKS"); return e ? atoll(e) : 0ll; }();
  // (the mono instantiations are compiled for two waves per SIMD: beyond latency-bound sizes the chain's kernels win)
  return pairs * ((long long)k_fwd + k_inv) <= (max_tasks > 0 ? max_tasks : (long long)p->cus * (C == 2 ? 256 : 8));
}

template <int R>
static void launch_duplex_R(const FwdArgs& fa, const InvArgs& ia, unsigned gf, unsigned gi, bool psy, int spread, int C,
                            hipStream_t s) {
  const dim3 grid(gf + gi), blk(AC_WAVES * 64);
  static_assert(AC_WAVES == AC_WAVES_PSY, "one workgroup shape for both halves");
  if constexpr (R == 8) {
    if (psy) {
      if (spread == 2) hipLaunchKernelGGL((k_duplex_fast<8, 0, true, AC_WAVES, 2>), grid, blk, 0, s, fa, ia, (int)gf);
      else hipLaunchKernelGGL((k_duplex_fast<8, 0, true, AC_WAVES, 0>), grid, blk, 0, s, fa, ia, (int)gf);
      return;
    }
  }
  if (C == 2) hipLaunchKernelGGL((k_duplex_fast<R, 0, false, AC_WAVES, 0>), grid, blk, 0, s, fa, ia, (int)gf);
  else hipLaunchKernelGGL((k_duplex_fast<R, 2, false, AC_WAVES, 0>), grid, blk, 0, s, fa, ia, (int)gf);
}

int launch_duplex_fast(const ac_mdct_plan* p, const ac_psy_plan* psy, const float* x, float* X, float* t, float* thr,
                       float drown, const float* prev_block, float* state_out, int k_fwd, const float* X_inv, float* x_inv,
                       const float* tail_in, float* tail_out, int k_inv, int B, int C, hipStream_t s) {
  if (!fast_duplex_serves(p, psy, B, C, k_fwd, k_inv)) {
    set_error("internal: the streaming duplex kernel does not serve this configuration");
    return AC_EUNSUPPORTED;
  }
  FwdArgs fa;
  InvArgs ia;
  unsigned gf, gi;
  int st = prep_fwd_fast(p, psy, x, 0, X, psy ? t : nullptr, psy ? thr : nullptr, drown, prev_block, B, k_fwd, k_fwd, C,
                         state_out, nullptr, nullptr, 0, fa, gf);
  if (!st) st = prep_inv_fast(p, X_inv, x_inv, 0, tail_in, tail_out, B, k_inv, k_inv, C, ia, gi);
  if (st) return st;
  const int spread = psy ? psy->spread : 0;
  if (p->N == Geo<8>::FN) launch_duplex_R<8>(fa, ia, gf, gi, psy != nullptr, spread, C, s);
  else launch_duplex_R<16>(fa, ia, gf, gi, false, 0, C, s);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

// ---- stand-alone tonality / threshold (k_psy_fast) ----
template <int R, int CMODE, int SPREAD>
static void launch_psy_thr(const PsyArgs& a, bool want_t, unsigned grid, hipStream_t s) {
  const dim3 blk(AC_WAVES * 64);
  if (want_t) hipLaunchKernelGGL((k_psy_fast<R, CMODE, true, true, AC_WAVES, SPREAD>), dim3(grid), blk, 0, s, a);
  else hipLaunchKernelGGL((k_psy_fast<R, CMODE, false, true, AC_WAVES, SPREAD>), dim3(grid), blk, 0, s, a);
}
template <int R, int CMODE>
static void launch_psy_bf16(const PsyArgs& a, bool want_t, bool want_thr, unsigned grid, hipStream_t s) {
  const dim3 blk(AC_WAVES * 64);
  if (want_t && !want_thr) hipLaunchKernelGGL((k_psy_fast<R, CMODE, true, false, AC_WAVES, 0, 2>), dim3(grid), blk, 0, s, a);
  else if (!want_t && want_thr) hipLaunchKernelGGL((k_psy_fast<R, CMODE, false, true, AC_WAVES, 0, 2>), dim3(grid), blk, 0, s, a);
  else if constexpr (R == 16 && CMODE == 2)   // (both in one pass: the second launch of the mono encode at 2048 only, see launch_psy_fast)
    if (want_t && want_thr) hipLaunchKernelGGL((k_psy_fast<R, CMODE, true, true, AC_WAVES, 0, 2>), dim3(grid), blk, 0, s, a);
}
template <int R, int CMODE>
static void launch_psy_R(const PsyArgs& a, bool want_t, bool want_thr, int spread, unsigned grid, hipStream_t s) {
  const dim3 blk(AC_WAVES * 64);
  if (CMODE == 0 && want_thr && spread == 1) return launch_psy_thr<R, 0, 1>(a, want_t, grid, s);
  if (CMODE == 0 && want_thr && spread == 2) return launch_psy_thr<R, 0, 2>(a, want_t, grid, s);
  if constexpr (CMODE == 2) {   // mono: the same two forms (two clips ride in the pair)
    if (want_thr && spread == 1) return launch_psy_thr<R, 2, 1>(a, want_t, grid, s);
    if (want_thr && spread == 2) return launch_psy_thr<R, 2, 2>(a, want_t, grid, s);
  }
  if (want_t && !want_thr) hipLaunchKernelGGL((k_psy_fast<R, CMODE, true, false, AC_WAVES>), dim3(grid), blk, 0, s, a);
  else if (!want_t && want_thr) hipLaunchKernelGGL((k_psy_fast<R, CMODE, false, true, AC_WAVES>), dim3(grid), blk, 0, s, a);
  else if (want_t && want_thr) hipLaunchKernelGGL((k_psy_fast<R, CMODE, true, true, AC_WAVES>), dim3(grid), blk, 0, s, a);
}

int launch_psy_fast(const ac_psy_plan* p, const float* X, const float* t_in, float* t_out, float* thr, float drown,
                    int B, int F, int C, hipStream_t s, int iof) {
  if (B <= 0 || C <= 0 || F <= 0) return AC_OK;
  PsyArgs a;
  a.X = X;
  a.t_in = t_in;
  a.t_out = t_out;
  a.thr = thr;
  a.psy = psy_params(p, drown);
  a.C = C;
  a.F = F;
  a.nsig = (long long)B * C;
  a.ntasks = ((C == 2) ? (long long)B : (a.nsig + 1) / 2) * F;
  unsigned grid;
  int st = grid_for(a.ntasks, AC_WAVES, &grid);
  if (st) return st;
  const bool want_t = (t_out != nullptr), want_thr = (thr != nullptr);
  const int cmode = (C == 2) ? 0 : (C == 1) ? 2 : 1;
  if (iof == 2 && C > 2) {
    set_error("internal: no wave-level masking-model kernel for bfloat16 tensors with %d channels", C);
    return AC_EUNSUPPORTED;
  }
  if (iof == 2 && want_t && want_thr && !(p->N == PsyGeo<16>::FN && cmode == 2)) {
    // (every other bfloat16 encode is one fused launch or calls tonality and threshold in turn: ac_encode_fused_typed)
    set_error("internal: no wave-level kernel for tonality and threshold of bfloat16 tensors in one pass at filters_n = %d, %d channels", p->N, C);
    return AC_EUNSUPPORTED;
  }
  if (iof == 2) {   // bfloat16 tensors: stereo and mono
    if (p->N == PsyGeo<8>::FN) {
      if (cmode == 0) launch_psy_bf16<8, 0>(a, want_t, want_thr, grid, s);
      else launch_psy_bf16<8, 2>(a, want_t, want_thr, grid, s);
    } else {
      if (cmode == 0) launch_psy_bf16<16, 0>(a, want_t, want_thr, grid, s);
      else launch_psy_bf16<16, 2>(a, want_t, want_thr, grid, s);
    }
    AC_HIP_CHECK(hipGetLastError());
    return AC_OK;
  }
  if (p->N == PsyGeo<8>::FN) {
    if (cmode == 0) launch_psy_R<8, 0>(a, want_t, want_thr, p->spread, grid, s);
    else if (cmode == 2) launch_psy_R<8, 2>(a, want_t, want_thr, p->spread, grid, s);
    else launch_psy_R<8, 1>(a, want_t, want_thr, p->spread, grid, s);
  } else {
    if (cmode == 0) launch_psy_R<16, 0>(a, want_t, want_thr, p->spread, grid, s);
    else if (cmode == 2) launch_psy_R<16, 2>(a, want_t, want_thr, p->spread, grid, s);
    else launch_psy_R<16, 1>(a, want_t, want_thr, p->spread, grid, s);
  }
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
