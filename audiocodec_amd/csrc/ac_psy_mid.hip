// Wave-level masking model for the configurations the fused epilogue of ac_fast_psy_dev.h does not serve: any even
// filter_bands_n up to 4096 (a frame is up to R = 1, 2, 4, 8, 16 or 32 granule registers per lane, the last ones partly filled
// when filter_bands_n is not a multiple of 128: 960, 576, 480 ...; above 512 the W_inv entries stay in global memory) with any Bark-band count up to 64 and any band layout (a bin may overlap several bands, bands may share
// bins freely) -- e.g. the models beside the several-frames-per-wave MDCT kernels (filters_n 256 / 512), where the
// O(N)-per-workgroup generic kernels ran at 0.5-0.8 TB/s.  gfx950 only.
//
// The per-frame arithmetic lives in ac_psy_mid_dev.h (the band walk) and ac_psy_runs_dev.h (the run-structured form), shared
// with the fused encodes; this file holds the two stand-alone kernels on strided rows, their row loader and their launchers.
// The table images are built in ac_psy_mid_plan.hip; the team form of more than two channels is ac_psy_runs_team_dev.h.
#include <algorithm>
#include <cstdlib>

#include "ac_psy_mid_launch.h"
#include "ac_psy_runs_team_dev.h"

namespace ac {
namespace {

using namespace mid;

struct MidArgs {
  const float* X;
  const float* t_in;
  float* t_out;
  float* thr;
  const uint32_t* img;   // ac_psy_plan::d_mid
  MidParams p;
  int C, F;
  int T;                 // frames per wave: workgroup g owns tasks [g nw T, (g + 1) nw T), wave w takes g nw T + w + nw t
  long long nsig, ntasks;
};

// rows of FB tasks of a wave: offsets, flags and the granules -- the loader and the threshold store of k_psy_runs.
// k_psy_mid below holds THE SAME CODE INLINE: a fix to the odd-channel or odd-batch handling here is a fix there too.  (Through
// RowSet every one of its 54 instances compiled to other instructions and 39 to other resources -- <32, 2, true, false> 150 for
// 192 VGPRs, <4, 2, true, true> 94 for 92, <2, 0, true, false> 69 for 60 SGPRs, <32, 1, false, true> 112 for 128 bytes of
// scratch -- which is where the change was to stop; k_psy_runs compiles to the same instructions either way.  DESIGN_LOG.md 15)
template <int R, int CMODE, int FB>
struct RowSet {
  bool ok[FB], has1[FB];
  size_t o0[FB], o1[FB], t0[FB], t1[FB];
  template <class INF>
  __device__ __forceinline__ void load(const float* X, int N, int C, int F, long long nsig, long long ntasks, long long task0, int tt, int T,
                                       int nw, int lane, INF in, v4f (&xq)[FB][R]) {
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
      const long long task = task0 + (long long)(tt + fb) * nw;
      ok[fb] = tt + fb < T && task < ntasks;
      const long long tk = ok[fb] ? task : task0 + (long long)tt * nw;   // (a frame past the end re-reads the group's first row)
      const size_t blk = (size_t)N * C;
      if (CMODE == 1) {
        // channels c, c + 1 of clip b (any channel count): rows strided by C, the pair's two values adjacent -- one 8-byte access
        // on the 4-byte grid per bin; the half-empty last pair of an odd count reads (c - 1, c) and keeps the second value.
        // The pairs of one frame are neighbouring tasks: the waves of a workgroup share the cache lines the pairs share.
        const int CP = (C + 1) / 2;
        const long long rest = tk / CP;
        const int c = 2 * (int)(tk - rest * CP), f = (int)(rest % F);
        const long long b = rest / F;
        has1[fb] = c + 1 < C;
        o0[fb] = ((size_t)b * F + (size_t)f) * blk + c;
        o1[fb] = o0[fb];
        t0[fb] = ((size_t)b * F + (size_t)f) * C + c;
        t1[fb] = t0[fb] + 1;
        const v2u* row = reinterpret_cast<const v2u*>(X + o0[fb] - (has1[fb] ? 0 : 1));
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const int q = 64 * i + lane;
          const v2u u = in(i) ? *reinterpret_cast<const v2u*>(reinterpret_cast<const float*>(row) + (size_t)(2 * q) * C) : v2u{0.f, 0.f};
          const v2u w = in(i) ? *reinterpret_cast<const v2u*>(reinterpret_cast<const float*>(row) + (size_t)(2 * q + 1) * C) : v2u{0.f, 0.f};
          xq[fb][i] = has1[fb] ? v4f{u.x, u.y, w.x, w.y} : v4f{u.y, u.y, w.y, w.y};
        }
        continue;
      }
      // the two signals of the wave: stereo = the two channels of clip p; mono = clips 2 p and 2 p + 1
      const int f = (int)(tk % F);
      const long long p = tk / F;
      has1[fb] = CMODE == 0 ? true : (2 * p + 1 < nsig);
      const long long b0 = CMODE == 0 ? p : 2 * p, b1 = CMODE == 0 ? p : (has1[fb] ? 2 * p + 1 : 2 * p);
      o0[fb] = ((size_t)b0 * F + (size_t)f) * blk;
      o1[fb] = ((size_t)b1 * F + (size_t)f) * blk;
      t0[fb] = ((size_t)b0 * F + (size_t)f) * C;
      t1[fb] = CMODE == 0 ? t0[fb] + 1 : ((size_t)b1 * F + (size_t)f) * C;
      // granule q = lane + 64 i: (X[2q], X[2q+1]) x (s0, s1); granules past the frame (q >= N/2) read as zero
      if (CMODE == 0) {
#pragma unroll
        for (int i = 0; i < R; ++i)
          xq[fb][i] = in(i) ? reinterpret_cast<const v4f*>(X + o0[fb])[64 * i + lane] : v4f{0.f, 0.f, 0.f, 0.f};
      } else {
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const v2f u = in(i) ? reinterpret_cast<const v2f*>(X + o0[fb])[64 * i + lane] : v2f{0.f, 0.f};
          // (no branch on has1: the half-empty last pair of an odd batch reads its one signal twice -- b1 above -- and
          // never stores the second; a conditional load would hold the wave at the join)
          const v2f w = in(i) ? reinterpret_cast<const v2f*>(X + o1[fb])[64 * i + lane] : v2f{0.f, 0.f};
          xq[fb][i] = v4f{u.x, w.x, u.y, w.y};
        }
      }
    }
  }
  __device__ __forceinline__ void store_thr(float* thr, int C, int fb, int i, int lane, const v4f& th) const {
    if (!ok[fb]) return;
    if (CMODE == 0) {
      __builtin_nontemporal_store(th, reinterpret_cast<v4f*>(thr + o0[fb]) + 64 * i + lane);
    } else if (CMODE == 1) {
      float* r0 = thr + o0[fb] + (size_t)(2 * (64 * i + lane)) * C;
      if (has1[fb]) {
        *reinterpret_cast<v2u*>(r0) = v2u{th.x, th.y};
        *reinterpret_cast<v2u*>(r0 + C) = v2u{th.z, th.w};
      } else {
        r0[0] = th.x;
        r0[C] = th.z;
      }
    } else {
      __builtin_nontemporal_store(v2f{th.x, th.z}, reinterpret_cast<v2f*>(thr + o0[fb]) + 64 * i + lane);
      if (has1[fb]) __builtin_nontemporal_store(v2f{th.y, th.w}, reinterpret_cast<v2f*>(thr + o1[fb]) + 64 * i + lane);
    }
  }
};

// One 64-lane wave per (frame, channel pair) as in k_psy_fast, FB frames at a time (their rows are loaded together: FB
// times the bytes in flight per wave, and the per-frame arithmetic of ac_psy_mid_dev.h interleaves the frames' dependent
// chains): rows move with coalesced 16-byte (stereo) or 8-byte (mono, two signals side by side) accesses.  All constant
// tables sit in one image copied to LDS per workgroup; a wave walks T frames so that the copy is paid once per 4 T frames.
// wave buffer: FB slots of [N] v2f intensities (c0, c1), the head of a slot reused for the frame's 64 G_j
template <int R, int CMODE, bool WANT_T, bool WANT_THR, int FB>
__global__ __launch_bounds__(256, (R >= 32 ? 1 : R >= 16 ? 2 : (WANT_THR && (FB > 1 || R >= 8)) ? 3 : 4)) void k_psy_mid(MidArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int N = a.p.N;
  const int SLOT = N >= 64 ? 8 * N : 512, WAVE_BYTES = FB * SLOT;   // (a slot also takes the frame's 64 G_j: 512 bytes)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint32_t* img = reinterpret_cast<uint32_t*>(smem);
  if (WANT_THR) {
    for (int i = threadIdx.x; i < a.p.lds_words / 4; i += blockDim.x)
      reinterpret_cast<uint4*>(img)[i] = reinterpret_cast<const uint4*>(a.img)[i];
    __syncthreads();
  }
  char* buf = smem + (size_t)a.p.lds_words * 4 + (size_t)wave * WAVE_BYTES;
  // the W_inv entries: in the LDS image, or (frames above 512 bins) read where the plan keeps them
  const uint4* wi = R >= AC_MID_WI_GLOBAL_R ? reinterpret_cast<const uint4*>(a.img + a.p.off_wi) : reinterpret_cast<const uint4*>(img + a.p.off_wi);
  const int C = a.C;
  const long long task0 = (long long)blockIdx.x * nw * a.T + wave;
  for (int tt = 0; tt < a.T && task0 + (long long)tt * nw < a.ntasks; tt += FB) {   // (no workgroup barrier inside)
    wave_sync();   // the previous group's reads of the wave's buffers are done
    // ---- RowSet::load, inline (see there: the comments too)
    auto in = [&](int i) { return in_frame<R>(a.p, i, lane); };
    bool ok[FB], has1[FB];
    size_t o0[FB], o1[FB], t0[FB], t1[FB];
    v4f xq[FB][R];
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
      const long long task = task0 + (long long)(tt + fb) * nw;
      ok[fb] = tt + fb < a.T && task < a.ntasks;
      const long long tk = ok[fb] ? task : task0 + (long long)tt * nw;
      const size_t blk = (size_t)N * C;
      if (CMODE == 1) {
        const int CP = (C + 1) / 2;
        const long long rest = tk / CP;
        const int c = 2 * (int)(tk - rest * CP), f = (int)(rest % a.F);
        const long long b = rest / a.F;
        has1[fb] = c + 1 < C;
        o0[fb] = ((size_t)b * a.F + (size_t)f) * blk + c;
        o1[fb] = o0[fb];
        t0[fb] = ((size_t)b * a.F + (size_t)f) * C + c;
        t1[fb] = t0[fb] + 1;
        const v2u* row = reinterpret_cast<const v2u*>(a.X + o0[fb] - (has1[fb] ? 0 : 1));
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const int q = 64 * i + lane;
          const v2u u = in(i) ? *reinterpret_cast<const v2u*>(reinterpret_cast<const float*>(row) + (size_t)(2 * q) * C) : v2u{0.f, 0.f};
          const v2u w = in(i) ? *reinterpret_cast<const v2u*>(reinterpret_cast<const float*>(row) + (size_t)(2 * q + 1) * C) : v2u{0.f, 0.f};
          xq[fb][i] = has1[fb] ? v4f{u.x, u.y, w.x, w.y} : v4f{u.y, u.y, w.y, w.y};
        }
        continue;
      }
      const int f = (int)(tk % a.F);
      const long long p = tk / a.F;
      has1[fb] = CMODE == 0 ? true : (2 * p + 1 < a.nsig);
      const long long b0 = CMODE == 0 ? p : 2 * p, b1 = CMODE == 0 ? p : (has1[fb] ? 2 * p + 1 : 2 * p);
      o0[fb] = ((size_t)b0 * a.F + (size_t)f) * blk;
      o1[fb] = ((size_t)b1 * a.F + (size_t)f) * blk;
      t0[fb] = ((size_t)b0 * a.F + (size_t)f) * C;
      t1[fb] = CMODE == 0 ? t0[fb] + 1 : ((size_t)b1 * a.F + (size_t)f) * C;
      if (CMODE == 0) {
#pragma unroll
        for (int i = 0; i < R; ++i)
          xq[fb][i] = in(i) ? reinterpret_cast<const v4f*>(a.X + o0[fb])[64 * i + lane] : v4f{0.f, 0.f, 0.f, 0.f};
      } else {
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const v2f u = in(i) ? reinterpret_cast<const v2f*>(a.X + o0[fb])[64 * i + lane] : v2f{0.f, 0.f};
          const v2f w = in(i) ? reinterpret_cast<const v2f*>(a.X + o1[fb])[64 * i + lane] : v2f{0.f, 0.f};
          xq[fb][i] = v4f{u.x, w.x, u.y, w.y};
        }
      }
    }
    v2f t[FB];
    if (WANT_T) {
      tonality_frames<R, FB>(xq, a.p, lane, t);
#pragma unroll
      for (int fb = 0; fb < FB; ++fb)
        if (ok[fb] && lane == 0) {
          a.t_out[t0[fb]] = t[fb].x;
          if (has1[fb]) a.t_out[t1[fb]] = t[fb].y;
        }
    } else {
#pragma unroll
      for (int fb = 0; fb < FB; ++fb) t[fb] = v2f{a.t_in[t0[fb]], has1[fb] ? a.t_in[t1[fb]] : 0.f};
    }
    if (!WANT_THR) continue;
    // ---- RowSet::store_thr, inline
    threshold_frames<R, FB>(xq, t, a.p, img, wi, buf, SLOT, lane, [&](int fb, int i, const v4f& th) {
      if (!ok[fb]) return;
      if (CMODE == 0) {
        __builtin_nontemporal_store(th, reinterpret_cast<v4f*>(a.thr + o0[fb]) + 64 * i + lane);
      } else if (CMODE == 1) {
        float* r0 = a.thr + o0[fb] + (size_t)(2 * (64 * i + lane)) * C;
        if (has1[fb]) {
          *reinterpret_cast<v2u*>(r0) = v2u{th.x, th.y};
          *reinterpret_cast<v2u*>(r0 + C) = v2u{th.z, th.w};
        } else {
          r0[0] = th.x;
          r0[C] = th.z;
        }
      } else {
        __builtin_nontemporal_store(v2f{th.x, th.z}, reinterpret_cast<v2f*>(a.thr + o0[fb]) + 64 * i + lane);
        if (has1[fb]) __builtin_nontemporal_store(v2f{th.y, th.w}, reinterpret_cast<v2f*>(a.thr + o1[fb]) + 64 * i + lane);
      }
    });
  }   // groups of frames of the wave
}

// the stand-alone kernel on the run-structured image: tasks, rows and the frame loop as in k_psy_mid; per wave FB slots of
// a.p.slot bytes behind the image
template <int R, int CMODE, bool WANT_T, bool WANT_THR, int FB>
__global__ __launch_bounds__(256, (R >= 32 ? 1 : R >= 16 ? 2 : 3)) void k_psy_runs(RunsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint32_t* img = reinterpret_cast<uint32_t*>(smem);
  const int slot = a.p.slot;
  char* buf = smem + (size_t)a.p.lds_words * 4 + (size_t)wave * FB * slot;
  constexpr bool IDX_REGS = R <= 8;   // (the launcher sizes lds_words to match)
  if (WANT_THR) {
    for (int i = threadIdx.x; i < a.p.lds_words / 4; i += blockDim.x)
      reinterpret_cast<uint4*>(img)[i] = reinterpret_cast<const uint4*>(a.img)[i];
    __syncthreads();
  }
  runs::RunsLane lc = {};
  runs::RegIdx<IDX_REGS ? R : 1> ridx = {};
  if (WANT_THR) {
    lc = runs::load_lane(img, lane);
    if (IDX_REGS) ridx.load(a.img, a.p, lane);
  }
  const long long task0 = (long long)blockIdx.x * nw * a.T + wave;
  for (int tt = 0; tt < a.T && task0 + (long long)tt * nw < a.ntasks; tt += FB) {   // (no workgroup barrier inside)
    wave_sync();   // the previous group's reads of the wave's slots are done
    RowSet<R, CMODE, FB> rs;
    v4f xq[FB][R];
    rs.load(a.X, a.p.N, a.C, a.F, a.nsig, a.ntasks, task0, tt, a.T, nw, lane, [&](int i) { return runs::in_frame<R>(a.p, i, lane); }, xq);
    v2f t[FB];
    runs::prep_frames<R, FB, WANT_T, WANT_THR>(xq, a.p, buf, slot, lane, t);
    if (WANT_T) {
#pragma unroll
      for (int fb = 0; fb < FB; ++fb)
        if (rs.ok[fb] && lane == 0) {
          a.t_out[rs.t0[fb]] = t[fb].x;
          if (rs.has1[fb]) a.t_out[rs.t1[fb]] = t[fb].y;
        }
    } else {
#pragma unroll
      for (int fb = 0; fb < FB; ++fb) t[fb] = v2f{a.t_in[rs.t0[fb]], rs.has1[fb] ? a.t_in[rs.t1[fb]] : 0.f};
    }
    if (!WANT_THR) continue;
    wave_sync();
    auto emit = [&](int fb, int i, const v4f& th) { rs.store_thr(a.thr, a.C, fb, i, lane, th); };
    if constexpr (IDX_REGS) runs::threshold_frames<R, FB, 0>(t, a.p, lc, img, buf, slot, lane, ridx, emit);
    else runs::threshold_frames<R, FB, 0>(t, a.p, lc, img, buf, slot, lane, runs::LdsIdx{img + runs::off_idx(a.p.lw, a.p.kb) + lane}, emit);
  }
}

// What both launches end in once the form has chosen nw waves per workgroup and `lds` bytes for them: frames per wave -- as
// many as keep every CU supplied with a few workgroups -- the grid, and the instance; family(Int<R>, Int<CMODE>, WANT_T,
// WANT_THR) names the kernel
template <class Args, class Family>
int launch_strided(const ac_psy_plan* p, Args& a, int nw, size_t lds, hipStream_t s, Family family) {
  const int R = mid_r(p->N), fb = psy_fb(R);
  a.T = psy_frames_per_wave(p, a.ntasks, nw, a.thr ? 8 : fb, fb);
  unsigned grid;
  const int st = grid_for(a.ntasks, nw * a.T, &grid);
  if (st) return st;
  return with_r_cmode(R, a.C, [&](auto r, auto cmode) {
    return launch_psy_outputs([=](auto want_t, auto want_thr) { return family(r, cmode, want_t, want_thr); }, grid, nw, lds, s, a);
  });
}

int launch_psy_runs(const ac_psy_plan* p, const float* X, const float* t_in, float* t_out, float* thr, float drown, int B, int F,
                    int C, hipStream_t s) {
  if (psy_runs_team_serves(p, X, thr, C)) return launch_psy_runs_team(p, X, t_in, t_out, thr, drown, B, F, C, s);
  const int R = mid_r(p->N), fb = psy_fb(R);
  RunsArgs a;
  fill_psy_args(a, X, t_in, t_out, thr, p->d_runs, B, F, C);
  a.p = runs_params(p, drown, R > 8);
  // waves per workgroup: the size that leaves the most waves resident (image + FB slots per wave; 160 KB of LDS per CU, the
  // kernels' register budget allows 12 / 8 / 4 waves per CU)
  const int wave_cap = R >= 32 ? 4 : R >= 16 ? 8 : 12;
  int nw = 4;
  {
    long best = -1;
    for (int w : {4, 3, 2, 1}) {
      const size_t b = (size_t)a.p.lds_words * 4 + (size_t)w * fb * a.p.slot;
      if (b > 160 * 1024) continue;
      const long res = std::min<long>((long)std::min<size_t>(8, 160 * 1024 / b) * w, wave_cap);
      if (res > best) {
        best = res;
        nw = w;
      }
    }
    if (best < 0) {
      set_error("internal: masking-model slots too large for LDS");
      return AC_EUNSUPPORTED;
    }
  }
  const size_t lds = thr ? (size_t)a.p.lds_words * 4 + (size_t)nw * fb * a.p.slot : 0;
  return launch_strided(p, a, nw, lds, s, [](auto r, auto cmode, auto want_t, auto want_thr) {
    return k_psy_runs<r(), cmode(), want_t(), want_thr(), psy_fb(r())>;
  });
}

}  // namespace

int launch_psy_mid(const ac_psy_plan* p, const float* X, const float* t_in, float* t_out, float* thr, float drown, int B,
                   int F, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || F <= 0) return AC_OK;
  static const bool no_runs = getenv("AC_NO_RUNS") != nullptr;   // (A/B hook: the band walk on a plan that has both forms)
  if (p->runs && !no_runs) return launch_psy_runs(p, X, t_in, t_out, thr, drown, B, F, C, s);
  // (the layout of the image was fixed when the plan was built: a launch only fills in arguments)
  const int R = mid_r(p->N), fb = psy_fb(R);
  MidArgs a;
  fill_psy_args(a, X, t_in, t_out, thr, p->d_mid, B, F, C);
  a.p = mid_params(p, drown);
  // four waves per workgroup when the image and the wave buffers fit three workgroups to a CU, else two; frames above
  // 1024 bins (32 KB of intensities per wave at 4096): the workgroup size that leaves the most waves resident
  int nw = 4;
  if (mid_lds_bytes(p->N, a.p.lds_words, nw, fb) > 53 * 1024) nw = 2;
  if (R >= AC_MID_WI_GLOBAL_R) {
    long best = 0;
    for (int w : {4, 2, 1}) {
      const size_t b = mid_lds_bytes(p->N, a.p.lds_words, w, fb);
      const long res = b > 160 * 1024 ? 0 : (long)std::min<size_t>(8, 160 * 1024 / b) * w;
      if (res > best) {
        best = res;
        nw = w;
      }
    }
  }
  const size_t lds = thr ? mid_lds_bytes(p->N, a.p.lds_words, nw, fb) : 0;
  if (lds > 160 * 1024) {
    set_error("internal: masking-model tables too large for LDS (%zu bytes)", lds);
    return AC_EUNSUPPORTED;
  }
  return launch_strided(p, a, nw, lds, s, [](auto r, auto cmode, auto want_t, auto want_thr) {
    return k_psy_mid<r(), cmode(), want_t(), want_thr(), psy_fb(r())>;
  });
}

}  // namespace ac
