// The several-frames-per-wave kernels of the wave-level tier (filters_n 512 ... 64): k_fwd_multi, k_inv_multi and their
// launch ladders.  Shared building blocks: ac_fast_dev.h.
#include <cstdlib>

#include "ac_fast.h"
#include "ac_fast_dev.h"
#include "ac_psy_mid_dev.h"
#include "ac_psy_runs_dev.h"

namespace ac {
namespace {

// ------------------------------------------------------------------------------------------------------
// Several short frames per wave: filters_n = 512, 256 (the reference's own test sizes,
// audiocodec/tests/test_mdctransformer.py:23) and 128.  A short frame keeps the wave-level scheme when NFR = 64 / LB
// frames share a wave, each on a group of LB consecutive lanes with eight complex points per lane:
//   filters_n = 512: NFR = 2 frames x 256 points on LB = 32 lanes;   256: NFR = 4 frames x 128 points on 16;
//   128: NFR = 8 frames x 64 points on 8 lanes (pass 2 below is then the identity: 64 = 8 x 8).
// With the frame index in the TOP lane bits (lane = l + LB f) the 8 LB-point FFT is 8 x (8 / NFR) x 8 with exactly the
// two LDS exchanges of the 512-point transform: element e = l + LB r; pass 1 over r (radix 8, twiddle W_{8 LB}^(l k0));
// exchange 1 hands lane (a = k0, m0) the eight values m0 + 8 e1 of row k0, and e1 = e1' + (8 / NFR) f, so pass 2 is NFR
// independent transforms of 8 / NFR points (one per frame, twiddle W_LB^(m0 k1')); exchange 2 and pass 3 (radix 8 over
// e0) are unchanged, and lane l + LB f ends up with the bins l + LB j of frame f: the layout the row loads / stores and
// the fold want, with LB in the place of 64.  Lane reversals stay inside a group: row_mirror DPP for LB = 16, row_mirror
// + two v_permlane16_swap per register pair for LB = 32 -- no LDS.  Table images have the Geo<8> layout, every entry
// replicated to the 64 lanes by the host (index r * 64 + lane as in the one-frame kernels).
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dft4(C2& x0, C2& x1, C2& x2, C2& x3) {
  const C2 t0 = cadd(x0, x2), t1 = csub(x0, x2), t2 = cadd(x1, x3), t3 = mul_mi(csub(x1, x3));
  x0 = cadd(t0, t2);
  x2 = csub(t0, t2);
  x1 = cadd(t1, t3);
  x3 = csub(t1, t3);
}
__device__ __forceinline__ void dft2(C2& x0, C2& x1) {
  const C2 s = cadd(x0, x1), d = csub(x0, x1);
  x0 = s;
  x1 = d;
}

template <int NFR>
__device__ __forceinline__ void fft_wave_multi(C2 (&z)[8], char* buf, gtab_t tab, const v2f (&p1)[8], int lane) {
  constexpr int Q2 = NFR >= 8 ? 1 : 8 / NFR;   // points of pass 2 per frame; 1: the pass is the identity, the exchanges remain
  static_assert(NFR == 2 || NFR == 4 || NFR == 8 || NFR == 16, "frames per wave");
  const int a = lane >> 3, m0 = lane & 7;
  if (NFR == 16) {   // two frames of four points each (see the 64-filter layout below)
    dft4(z[0], z[1], z[2], z[3]);
    dft4(z[4], z[5], z[6], z[7]);
#pragma unroll
    for (int k = 1; k < 8; ++k)
      if (k != 4) z[k] = cmul(z[k], p1[k]);
  } else {
    dft8(z);
#pragma unroll
    for (int k = 1; k < 8; ++k) z[k] = cmul(z[k], p1[k]);
  }
  C2 y[8];
  wave_sync();
  {
    char* w1 = buf + 16 * lane;
#pragma unroll
    for (int k = 0; k < 8; ++k) lds_put(w1 + 1152 * k, z[k]);
  }
  wave_sync();
  {
    const char* r1 = buf + 16 * (a * 72 + m0);
#pragma unroll
    for (int r = 0; r < 8; ++r) y[r] = lds_get(r1 + 128 * r);
  }
  if (NFR == 2) {
    dft4(y[0], y[1], y[2], y[3]);
    dft4(y[4], y[5], y[6], y[7]);
  } else if (NFR == 4) {
    dft2(y[0], y[1]);
    dft2(y[2], y[3]);
    dft2(y[4], y[5]);
    dft2(y[6], y[7]);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k)
    z[k] = (k % Q2 == 0) ? y[k] : cmul(y[k], reinterpret_cast<const v2f*>(tab + Geo<8>::I_P2)[k * 8 + m0]);
  wave_sync();
  {
    char* w2 = buf + 16 * (9 * a + m0);
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) lds_put(w2 + 16 * 72 * kk, z[kk]);
  }
  wave_sync();
  {
    const char* r2 = buf + 144 * lane;
#pragma unroll
    for (int r = 0; r < 8; ++r) y[r] = lds_get(r2 + 16 * r);
  }
  dft8(y);
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = y[j];
}

// lane reversal inside a group of LB lanes (lane -> lane ^ (LB - 1)), both halves of a (c0, c1) pair
template <int LB>
__device__ __forceinline__ v2f rev_group(v2f v) {
  unsigned a = __float_as_uint(v.x), b = __float_as_uint(v.y);
  if (LB == 32) {   // complement lane bit 4: v_permlane16_swap twice, the operands' roles exchanged in between
    const auto u = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    const auto w = __builtin_amdgcn_permlane16_swap(u[1], u[0], false, false);
    a = w[0];
    b = w[1];
  }
  constexpr int MIRROR = (LB == 4) ? 0x1b : (LB == 8) ? 0x141 : 0x140;   // quad_perm [3,2,1,0] / row_half_mirror / row_mirror
  return v2f{__uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)a, MIRROR, 0xf, 0xf, false)),
             __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)b, MIRROR, 0xf, 0xf, false))};
}
// out[i] = in[(OFS - i) mod 8] of the mirrored lane of the group
template <int LB, int OFS>
__device__ __forceinline__ void rev_exchange_g(const v2f (&in)[8], v2f (&out)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = rev_group<LB>(in[(OFS - i) & 7]);
}

// one natural-order row of a short frame: lane l of its group moves granules l + LB i, i = 0..7
// CMODE 0: two channels, 16-byte interleaved granules; CMODE 2: one channel, two signals side by side, 8-byte granules
template <int CMODE, int LB>
__device__ __forceinline__ void load_rowm(const float* r0, const float* r1, bool has1, int l, v4f (&v)[8]) {
  if (CMODE == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = reinterpret_cast<const v4f*>(r0)[LB * i + l];
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const v2f u = reinterpret_cast<const v2f*>(r0)[LB * i + l];
      v[i] = v4f{u.x, 0.f, u.y, 0.f};
    }
    if (has1) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const v2f w = reinterpret_cast<const v2f*>(r1)[LB * i + l];
        v[i].y = w.x;
        v[i].w = w.y;
      }
    }
  }
}
template <int CMODE, int LB>
__device__ __forceinline__ void store_rowm(float* r0, float* r1, bool has1, int l, const v4f (&v)[8]) {
  if (CMODE == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#if AC_NT_STORE
      __builtin_nontemporal_store(v[i], reinterpret_cast<v4f*>(r0) + LB * i + l);
#else
      reinterpret_cast<v4f*>(r0)[LB * i + l] = v[i];
#endif
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) reinterpret_cast<v2f*>(r0)[LB * i + l] = v2f{v[i].x, v[i].z};
    if (has1) {
#pragma unroll
      for (int i = 0; i < 8; ++i) reinterpret_cast<v2f*>(r1)[LB * i + l] = v2f{v[i].y, v[i].w};
    }
  }
}

// filters_n = 64: a frame is a 32-point transform = 4 x 8.  INPUT rows sit on 8 lanes x 4 registers, two frames in the
// register halves (lane = l8 + 8 g, register 4 fb + i4 holds granule l8 + 8 i4 of frame 2 g + fb); pass 1 is a radix-4
// over i4, the exchanges are the usual ones, pass 3 the radix-8 over l8, and the OUTPUT lands on 4 lanes x 8 registers
// (lane = l4 + 4 f, register j holds bin l4 + 4 j of frame f = 2 g + fb): the LB = 4 form of the layouts above.
template <int CMODE>
__device__ __forceinline__ void load_half(const float* r0, const float* r1, bool has1, int l8, v4f* v) {
  if (CMODE == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = reinterpret_cast<const v4f*>(r0)[8 * i + l8];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const v2f u = reinterpret_cast<const v2f*>(r0)[8 * i + l8];
      const v2f w = has1 ? reinterpret_cast<const v2f*>(r1)[8 * i + l8] : v2f{0.f, 0.f};
      v[i] = v4f{u.x, w.x, u.y, w.y};
    }
  }
}
template <int CMODE>
__device__ __forceinline__ void store_half(float* r0, float* r1, bool has1, int l8, const v4f* v) {
  if (CMODE == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) reinterpret_cast<v4f*>(r0)[8 * i + l8] = v[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      reinterpret_cast<v2f*>(r0)[8 * i + l8] = v2f{v[i].x, v[i].z};
      if (has1) reinterpret_cast<v2f*>(r1)[8 * i + l8] = v2f{v[i].y, v[i].w};
    }
  }
}

// the same movers for 16-bit PCM rows (x = pcm / 32768 on the way in, to_pcm16(x) on the way out)
template <int CMODE, int LB>
__device__ __forceinline__ void load_rowm(const int16_t* r0, const int16_t* r1, bool has1, int l, v4f (&v)[8]) {
  if (CMODE == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const s4 p = reinterpret_cast<const s4*>(r0)[LB * i + l];
      v[i] = v4f{Pcm16Fmt::dec(p.x), Pcm16Fmt::dec(p.y), Pcm16Fmt::dec(p.z), Pcm16Fmt::dec(p.w)};
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const s2 u = reinterpret_cast<const s2*>(r0)[LB * i + l];
      const s2 w = has1 ? reinterpret_cast<const s2*>(r1)[LB * i + l] : s2{0, 0};
      v[i] = v4f{Pcm16Fmt::dec(u.x), Pcm16Fmt::dec(w.x), Pcm16Fmt::dec(u.y), Pcm16Fmt::dec(w.y)};
    }
  }
}
template <int CMODE, int LB>
__device__ __forceinline__ void store_rowm(int16_t* r0, int16_t* r1, bool has1, int l, const v4f (&v)[8]) {
  if (CMODE == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const s2 lo = Pcm16Fmt::enc2(v[i].x, v[i].y), hi = Pcm16Fmt::enc2(v[i].z, v[i].w);
      reinterpret_cast<s4*>(r0)[LB * i + l] = s4{lo.x, lo.y, hi.x, hi.y};
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      reinterpret_cast<s2*>(r0)[LB * i + l] = Pcm16Fmt::enc2(v[i].x, v[i].z);
      if (has1) reinterpret_cast<s2*>(r1)[LB * i + l] = Pcm16Fmt::enc2(v[i].y, v[i].w);
    }
  }
}
template <int CMODE>
__device__ __forceinline__ void load_half(const int16_t* r0, const int16_t* r1, bool has1, int l8, v4f* v) {
  if (CMODE == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const s4 p = reinterpret_cast<const s4*>(r0)[8 * i + l8];
      v[i] = v4f{Pcm16Fmt::dec(p.x), Pcm16Fmt::dec(p.y), Pcm16Fmt::dec(p.z), Pcm16Fmt::dec(p.w)};
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const s2 u = reinterpret_cast<const s2*>(r0)[8 * i + l8];
      const s2 w = has1 ? reinterpret_cast<const s2*>(r1)[8 * i + l8] : s2{0, 0};
      v[i] = v4f{Pcm16Fmt::dec(u.x), Pcm16Fmt::dec(w.x), Pcm16Fmt::dec(u.y), Pcm16Fmt::dec(w.y)};
    }
  }
}

struct FwdMArgs {
  const void* x;     // [B, Kin*N, C]  float32, or 16-bit PCM (IOF 1)
  float* X;          // [B, F, N, C]
  const float* prev_block;   // [B, N, C] or null: block -1 of every signal (streaming analysis state)
  float* state_out;          // [B, N, C] or null: receives block Kin-1 (another buffer than prev_block)
  const float* tab;  // analysis image (Geo<8> layout, lane-replicated)
  int Kin, F, C;
  int cpp;           // chunks of NFR consecutive frames per signal pair: ceil(F / NFR)
  int T;             // chunks per wave: workgroup g owns chunks [g NW T, (g+1) NW T), wave w takes g NW T + w + NW t
  long long nsig, ntasks;   // B * C and npairs * cpp
  // fused masking model (PSY kernels): tonality [B, F, 1, C], threshold [B, F, N, C], the image of ac_psy_plan::d_runs
  float* t;
  float* thr;
  const uint32_t* psy_img;
  runs::RunsParams rp;
};

// LDS of the several-frames-per-wave analysis kernels: [NW wave buffers | table image | masking-model image (PSY)].
// The table images in global memory carry every entry replicated to the 64 lanes (index r * 64 + lane); the PSY kernels,
// short of LDS, keep one period of each row only -- TS = max(LB, 8) entries (8: the 64-filter kernels read their input-side
// tables by lane mod 8) -- and, at two frames per wave (filters_n = 512, where the masking model's image is largest), read
// the fold coefficients and the pre-twiddles from the (L2-resident) global image: 53.6 KB per workgroup, three to a CU.
template <int NFR, bool PSY> constexpr int multi_ts() { return PSY ? ((64 / NFR) > 8 ? (64 / NFR) : 8) : 64; }
template <int NFR, bool PSY> constexpr bool multi_pre_global() { return PSY && NFR == 2; }
template <int NFR, bool PSY> constexpr int multi_tab_bytes() {   // (PRE_GLOBAL: fold coefficients and pre-twiddles both stay in global memory)
  return PSY ? (128 + (multi_pre_global<NFR, PSY>() ? 1 : 3) * 16 * multi_ts<NFR, PSY>()) * 4 : Geo<8>::TAB_LDS;
}
// The fused masking model (ac_psy_runs_dev.h) works on FB frames side by side, each in a slot of its own: intensities,
// their partial sums, later G and the threshold entries.  multi_slot(): the largest slot build_runs lays out for
// filters_n = FN (all four levels), a compile-time stride so that a frame's displacement is an immediate of its LDS
// accesses.  The wave lays the spectra of one group of FB frames at a time straight into the slots (the lanes of the later
// groups keep theirs in registers meanwhile) and the intensities overwrite them: FB slots per wave, no staging area.
template <int NFR> constexpr int multi_slot() { return runs::runs_slot_max(1024 / NFR); }
template <int NFR> constexpr int multi_fb() { return (1024 / NFR) >= 512 ? 2 : 4; }
template <int NFR, bool PSY> constexpr int multi_wave_bytes() {
  if (!PSY) return WAVE_LDS;
  const int need = multi_fb<NFR>() * multi_slot<NFR>();
  return need > WAVE_LDS ? need : WAVE_LDS;
}

// analysis: the lanes of group f transform frame NFR c + f of the wave's signal pair (a group whose frame index is past
// the last frame idles); fold and twiddles as in k_fwd_fast with LB in the place of 64
// PSY: the masking model of ac_psy_mid_dev.h on the frames just transformed (the fused encode at filters_n 64 ... 512): the
// wave lays its NFR spectra out in natural order in its LDS buffer (8 KB: NFR frames x N bins x two signals), then walks
// them one frame at a time with all 64 lanes exactly as k_psy_mid does on a row loaded from HBM -- same device function on
// the same values, so X, tonality and threshold equal transform -> k_psy_mid bit for bit, and X is not read back from HBM.
// A frame's intensities overwrite its own slot, and so do its 64 G_j after them.
template <int NFR, int CMODE, int NW, int IOF = 0, bool FOLD4 = false, bool PSY = false>
__global__ __launch_bounds__(NW * 64, AC_WPE) void k_fwd_multi(FwdMArgs a) {
  using pcm_t = typename std::conditional<IOF == 1, int16_t, float>::type;   // (streaming state: float32 only, IOF 0)
  using G = Geo<8>;
  constexpr int LB = 64 / NFR;
  constexpr int TS = multi_ts<NFR, PSY>();                  // entries per register row of the LDS tables
  constexpr bool PRE_GLOBAL = multi_pre_global<NFR, PSY>();
  constexpr int TABB = multi_tab_bytes<NFR, PSY>();
  // (LDS offsets of the tables in floats: the global image's own when it is copied whole)
  constexpr int L_POST = PSY ? 128 : G::I_POST, L_COEF = PSY ? 128 + 16 * TS : G::I_COEF, L_PRE = PSY ? 128 + 32 * TS : G::I_PRE;
  constexpr int WSTR = multi_wave_bytes<NFR, PSY>();            // bytes of LDS per wave
  extern __shared__ __attribute__((aligned(16))) char lds[];   // NW * WSTR + TABB (+ the masking-model image)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if constexpr (PSY) {
    float* dst = reinterpret_cast<float*>(lds + NW * WSTR);
    for (int i = threadIdx.x; i < 128; i += NW * 64) dst[G::I_P2 + i] = a.tab[G::I_P2 + i];
    for (int i = threadIdx.x; i < 8 * TS; i += NW * 64) {     // one period of every row of POST / COEF / PRE
      const int src = (i / TS) * 64 + (i % TS);
      reinterpret_cast<v2f*>(dst + L_POST)[i] = reinterpret_cast<const v2f*>(a.tab + G::I_POST)[src];
      if (!PRE_GLOBAL) {
        reinterpret_cast<v2f*>(dst + L_COEF)[i] = reinterpret_cast<const v2f*>(a.tab + G::I_COEF)[src];
        reinterpret_cast<v2f*>(dst + L_PRE)[i] = reinterpret_cast<const v2f*>(a.tab + G::I_PRE)[src];
      }
    }
    uint4* pd = reinterpret_cast<uint4*>(lds + NW * WSTR + TABB);
    for (int i = threadIdx.x; i < a.rp.lds_words / 4; i += NW * 64) pd[i] = reinterpret_cast<const uint4*>(a.psy_img)[i];
    __syncthreads();
  } else {
    load_tables<NW, WAVE_LDS, G::I_LDS, 0>(lds, a.tab, nullptr);
  }
  char* buf = lds + wave * WSTR;
  gtab_t tab = reinterpret_cast<const float*>(lds + NW * WSTR);
  const uint32_t* pimg = reinterpret_cast<const uint32_t*>(lds + NW * WSTR + TABB);
  // masking model: constants of band / edge bin `lane`, the lane's per-bin entry offsets (registers: at most four words)
  constexpr int RPM = (1024 / NFR) >= 128 ? (1024 / NFR) / 128 : 1;
  runs::RegIdx<RPM> ridx = {};
  if constexpr (PSY) ridx.load(a.psy_img, a.rp, lane);
  const int tl = lane & (TS - 1);   // column of the lane in a table row
  // the fused kernels whose later groups of frames wait in registers for the model (NFR > FB) fetch the pass-1 twiddles per
  // chunk (L2-resident) instead of holding them across it: 14 registers less where the pressure peaks
  constexpr bool P1_PER_CHUNK = PSY && NFR > multi_fb<NFR>();
  v2f p1[8];
  if (!P1_PER_CHUNK) load_p1<8>(a.tab, lane, p1);
  const int f = lane / LB, l = lane & (LB - 1);
  const int C = a.C;
  const size_t blk = (size_t)(16 * LB) * C;   // floats per block / frame row over all channels
  long long task = (long long)blockIdx.x * NW * a.T + wave;
  long long pair = task / a.cpp;          // (one 64-bit division per wave; the task index then advances without)
  int c = (int)(task - pair * a.cpp);
  for (int t = 0; t < a.T && task < a.ntasks; ++t, task += NW, c += NW) {
    if (P1_PER_CHUNK) load_p1<8>(a.tab, (int)in_loop((uint32_t)lane), p1);
    while (c >= a.cpp) {
      c -= a.cpp;
      ++pair;
    }
    const Pair pq = make_pair<CMODE>(pair, C, a.nsig);
    // (tables read from global memory are fetched per chunk: hoisted out of the loop they would hold 32 registers)
    const uint32_t glane = PRE_GLOBAL ? in_loop((uint32_t)lane) : (uint32_t)lane;
    const int n = c * NFR + f;
    const bool frame_ok = n < a.F;
    const pcm_t* x0 = static_cast<const pcm_t*>(a.x) + row_off(pq.b0, a.Kin, 0, blk, pq.c0);
    const pcm_t* x1 = static_cast<const pcm_t*>(a.x) + row_off(pq.b1, a.Kin, 0, blk, pq.c1);
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    v4f cb[8], pb[8];
    // rows of frame m: the current block m and the block before it (streaming: block -1 is the stored state); a missing
    // block (before the first / after the last) is read from a neighbouring valid row and zeroed afterwards
    auto rows_of = [&](int m, const pcm_t*& c0p, const pcm_t*& c1p, const pcm_t*& p0p, const pcm_t*& p1p, bool& cur_ok,
                       bool& prv_ok) {
      const bool from_state = IOF == 0 && a.prev_block != nullptr && m == 0;
      cur_ok = m < a.Kin;
      prv_ok = (m >= 1 && m <= a.Kin) || from_state;
      const int bc = cur_ok ? m : a.Kin - 1, bp = (m >= 1 && m <= a.Kin) ? m - 1 : 0;
      c0p = x0 + (size_t)bc * blk;
      c1p = x1 + (size_t)bc * blk;
      p0p = x0 + (size_t)bp * blk;
      p1p = x1 + (size_t)bp * blk;
      if constexpr (IOF == 0) {
        if (from_state) {
          p0p = a.prev_block + row_off(pq.b0, 1, 0, blk, pq.c0);
          p1p = a.prev_block + row_off(pq.b1, 1, 0, blk, pq.c1);
        }
      }
    };
    C2 z[8];
    if (NFR == 16) {
      const int l8 = lane & 7, g = lane >> 3;
#pragma unroll
      for (int fb = 0; fb < 2; ++fb) {
        const int m = c * NFR + 2 * g + fb;
        const pcm_t *c0p, *c1p, *p0p, *p1p;
        bool cur_ok, prv_ok;
        rows_of(m, c0p, c1p, p0p, p1p, cur_ok, prv_ok);
        load_half<CMODE>(c0p, c1p, pq.has1, l8, cb + 4 * fb);
        load_half<CMODE>(p0p, p1p, pq.has1, l8, pb + 4 * fb);
        if constexpr (IOF == 0) {
          if (a.state_out && m == a.Kin - 1)   // streaming: the chunk's last block is the next chunk's block -1
            store_half<CMODE>(a.state_out + row_off(pq.b0, 1, 0, blk, pq.c0), a.state_out + row_off(pq.b1, 1, 0, blk, pq.c1),
                              pq.has1, l8, cb + 4 * fb);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          cb[4 * fb + i] = cur_ok ? cb[4 * fb + i] : zero;
          pb[4 * fb + i] = prv_ok ? pb[4 * fb + i] : zero;
        }
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int fb4 = r & 4, r4 = r & 3;
        const v4f& go_p = pb[fb4 + ((1 - r4) & 3)];
        const v4f& go_c = cb[fb4 + ((1 - r4) & 3)];
        const v2f xop = rev_group<8>(v2f{go_p.z, go_p.w}), xoc = rev_group<8>(v2f{go_c.z, go_c.w});
        const v4f& gp = pb[fb4 + ((r4 + 2) & 3)];
        const v4f& gc = cb[fb4 + ((r4 + 2) & 3)];
        const v2f xep = v2f{gp.x, gp.y}, xec = v2f{gc.x, gc.y};
        const v2f ab = (PRE_GLOBAL ? reinterpret_cast<const v2f*>(a.tab + G::I_COEF)[r * 64 + glane] : reinterpret_cast<const v2f*>(tab + L_COEF)[r * TS + tl]);
        const v2f carry = ab.y * xep + ab.x * xop;
        v2f cur;
        if constexpr (FOLD4) {   // a fold block that is not a rotation: its own two coefficients for the current block
          const v2f ce = reinterpret_cast<const v2f*>(a.tab + G::I_COEF2)[r * 64 + lane];
          cur = ce.x * xec + ce.y * xoc;
        } else {
          cur = (r4 < 2) ? (ab.y * xoc - ab.x * xec) : (ab.x * xec - ab.y * xoc);
        }
        const C2 v = (r4 < 2) ? C2{carry, cur} : C2{cur, carry};
        z[r] = cmul(v, PRE_GLOBAL ? reinterpret_cast<const v2f*>(a.tab + G::I_PRE)[r * 64 + glane]
                                   : reinterpret_cast<const v2f*>(tab + L_PRE)[r * TS + tl]);
      }
    } else {
      const pcm_t *c0p, *c1p, *p0p, *p1p;
      bool cur_ok, prv_ok;
      rows_of(n, c0p, c1p, p0p, p1p, cur_ok, prv_ok);
      load_rowm<CMODE, LB>(c0p, c1p, pq.has1, l, cb);
      load_rowm<CMODE, LB>(p0p, p1p, pq.has1, l, pb);
      if constexpr (IOF == 0) {
        if (a.state_out && n == a.Kin - 1)   // streaming: the chunk's last block is the next chunk's block -1
          store_rowm<CMODE, LB>(a.state_out + row_off(pq.b0, 1, 0, blk, pq.c0), a.state_out + row_off(pq.b1, 1, 0, blk, pq.c1),
                                pq.has1, l, cb);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        cb[i] = cur_ok ? cb[i] : zero;
        pb[i] = prv_ok ? pb[i] : zero;
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const v4f& go_p = pb[(3 - r) & 7];
        const v4f& go_c = cb[(3 - r) & 7];
        const v2f xop = rev_group<LB>(v2f{go_p.z, go_p.w}), xoc = rev_group<LB>(v2f{go_c.z, go_c.w});
        const v4f& gp = pb[(r + 4) & 7];
        const v4f& gc = cb[(r + 4) & 7];
        const v2f xep = v2f{gp.x, gp.y}, xec = v2f{gc.x, gc.y};
        const v2f ab = (PRE_GLOBAL ? reinterpret_cast<const v2f*>(a.tab + G::I_COEF)[r * 64 + glane] : reinterpret_cast<const v2f*>(tab + L_COEF)[r * TS + tl]);
        const v2f carry = ab.y * xep + ab.x * xop;
        v2f cur;
        if constexpr (FOLD4) {
          const v2f ce = reinterpret_cast<const v2f*>(a.tab + G::I_COEF2)[r * 64 + lane];
          cur = ce.x * xec + ce.y * xoc;
        } else {
          cur = (r < 4) ? (ab.y * xoc - ab.x * xec) : (ab.x * xec - ab.y * xoc);
        }
        const C2 v = (r < 4) ? C2{carry, cur} : C2{cur, carry};
        z[r] = cmul(v, PRE_GLOBAL ? reinterpret_cast<const v2f*>(a.tab + G::I_PRE)[r * 64 + glane]
                                   : reinterpret_cast<const v2f*>(tab + L_PRE)[r * TS + tl]);
      }
    }
    fft_wave_multi<NFR>(z, buf, tab, p1, lane);
    v4f row[8];
    {
      v2f xe[8], xo_in[8], xo[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const C2 r = cmul_negim(z[j], reinterpret_cast<const v2f*>(tab + L_POST)[j * TS + tl]);
        xe[j] = r.re;
        xo_in[j] = r.im;
      }
      rev_exchange_g<LB, 7>(xo_in, xo);
#pragma unroll
      for (int i = 0; i < 8; ++i) row[i] = v4f{xe[i].x, xe[i].y, xo[i].x, xo[i].y};
    }
    if (frame_ok) {
      const int nn = n;
      store_rowm<CMODE, LB>(a.X + row_off(pq.b0, a.F, nn, blk, pq.c0), a.X + row_off(pq.b1, a.F, nn, blk, pq.c1), pq.has1, l, row);
    }
    if constexpr (PSY) {
      constexpr int FN = 16 * LB;                      // filters_n
      constexpr int RP = RPM;                          // granule registers per lane when 64 lanes share one frame
      constexpr int FB = multi_fb<NFR>();              // frames side by side (ac_psy_runs_dev.h)
      constexpr int SLOT = multi_slot<NFR>();
      static_assert(NFR % FB == 0, "whole groups");
      const runs::RunsLane lc = runs::load_lane(pimg, lane);   // (per chunk: held across the FFT it would cost seven registers)
#pragma unroll 1
      for (int g0 = 0; g0 < NFR; g0 += FB) {
        if (c * NFR + g0 >= a.F) break;
        wave_sync();   // the FFT's (or the previous group's) accesses of the slots are done
        if (f >= g0 && f < g0 + FB) {
          char* fb = buf + (f - g0) * SLOT + 16 * l;   // granule q = l + LB i of the group's frame at byte 16 q of its slot
#pragma unroll
          for (int i = 0; i < 8; ++i) *reinterpret_cast<v4f*>(fb + 16 * LB * i) = row[i];
        }
        wave_sync();
        const char* ib = buf;
        constexpr int STG = SLOT;
        char* slots = buf;
        v4f xq[FB][RP];
        bool ok[FB];
        size_t o0[FB], o1[FB];
#pragma unroll
        for (int fb = 0; fb < FB; ++fb) {
          const int nn = c * NFR + g0 + fb;
          ok[fb] = nn < a.F;   // (a row past the last frame holds the zero spectrum of an idle group of lanes: computed, not stored)
          o0[fb] = row_off(pq.b0, a.F, ok[fb] ? nn : 0, blk, pq.c0);
          o1[fb] = row_off(pq.b1, a.F, ok[fb] ? nn : 0, blk, pq.c1);
#pragma unroll
          for (int i = 0; i < RP; ++i)
            xq[fb][i] = runs::in_frame<RP>(a.rp, i, lane) ? *reinterpret_cast<const v4f*>(ib + fb * STG + 16 * (64 * i + lane))
                                                          : v4f{0.f, 0.f, 0.f, 0.f};
        }
        v2f t[FB];
        runs::prep_frames<RP, FB, true, true>(xq, a.rp, slots, SLOT, lane, t);
#pragma unroll
        for (int fb = 0; fb < FB; ++fb)
          if (ok[fb] && lane == 0) {
            const int nn = c * NFR + g0 + fb;
            a.t[((size_t)pq.b0 * a.F + (size_t)nn) * C + pq.c0] = t[fb].x;
            if (pq.has1) a.t[((size_t)pq.b1 * a.F + (size_t)nn) * C + pq.c1] = t[fb].y;
          }
        wave_sync();
        runs::threshold_frames<RP, FB, FN>(t, a.rp, lc, pimg, slots, SLOT, lane, ridx, [&](int fb, int i, const v4f& th) {
          if (!ok[fb]) return;
          if (CMODE == 0) {
            __builtin_nontemporal_store(th, reinterpret_cast<v4f*>(a.thr + o0[fb]) + 64 * i + lane);
          } else {
            reinterpret_cast<v2f*>(a.thr + o0[fb])[64 * i + lane] = v2f{th.x, th.z};
            if (pq.has1) reinterpret_cast<v2f*>(a.thr + o1[fb])[64 * i + lane] = v2f{th.y, th.w};
          }
        });
        wave_sync();   // the group's reads of its slots are done before the next group's intensities (or the next chunk's FFT) land
      }
    }
  }
}

struct InvMArgs {
  const float* X;    // [B, Kp, N, C]
  void* x;           // [B, nblk*N, C]  float32, or 16-bit PCM (IOF 1)
  const float* tail_in;   // [B, C, N/2] or null: aliased half of the frame before frame 0 (streaming synthesis state)
  float* tail_out;        // [B, C, N/2] or null: receives the aliased half of frame nblk - 1
  const float* tab;  // analysis image; the synthesis image follows at Geo<8>::I_TOTAL floats
  int Kp, nblk, C;
  int cpp;           // chunks of NFR consecutive output blocks per signal pair: ceil(nblk / NFR)
  int spc;           // chunks per strip
  int nstrips;       // strips per signal pair
  long long nsig, ntasks;   // B * C and npairs * nstrips
};

// synthesis: a wave walks a strip of chunks; in a chunk the lanes of group f transform frame n = NFR c + f and finish
// output block n from it and the aliased half of frame n - 1, which the group below has (one shift by LB lanes through
// LDS); group 0 takes it from the chunk before (kept in registers), and a strip that does not start a signal begins with
// the DCT-IV of the chunk before it.  Unfold as in k_inv_fast.
template <int NFR, int CMODE, int NW, int IOF = 0, bool FOLD4 = false>
__global__ __launch_bounds__(NW * 64, AC_WPE) void k_inv_multi(InvMArgs a) {
  using pcm_t = typename std::conditional<IOF == 1, int16_t, float>::type;
  using G = Geo<8>;
  constexpr int LB = 64 / NFR;
  __shared__ __attribute__((aligned(16))) char lds[NW * WAVE_LDS + G::TAB_LDS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  load_tables<NW, WAVE_LDS, G::I_LDS, 0>(lds, a.tab + G::I_TOTAL, nullptr);
  char* buf = lds + wave * WAVE_LDS;
  gtab_t tab = reinterpret_cast<const float*>(lds + NW * WAVE_LDS);
  v2f p1[8];
  load_p1<8>(a.tab + G::I_TOTAL, lane, p1);
  const long long task = (long long)blockIdx.x * NW + wave;
  if (task >= a.ntasks) return;   // (no workgroup barrier below)
  const int f = lane / LB, l = lane & (LB - 1);
  const int C = a.C;
  const size_t blk = (size_t)(16 * LB) * C;
  const long long pair = task / a.nstrips;
  const int strip = (int)(task - pair * a.nstrips);
  const Pair pq = make_pair<CMODE>(pair, C, a.nsig);
  const int c0 = strip * a.spc, c1 = min(a.cpp, c0 + a.spc);
  const float* X0 = a.X + row_off(pq.b0, a.Kp, 0, blk, pq.c0);
  const float* X1 = a.X + row_off(pq.b1, a.Kp, 0, blk, pq.c1);
  const v4f zero = {0.f, 0.f, 0.f, 0.f};

  // DCT-IV of the frames of chunk c: (now, nxt) per output element k = l + LB j of the group's frame
  auto dct_chunk = [&](int c, v2f (&now)[8], v2f (&nxt)[8]) {
    v4f frm[8];
    v2f xo[8];
    if (NFR == 16) {   // input on 8 lanes x 4 registers, two frames in the register halves
      const int l8 = lane & 7, g = lane >> 3;
#pragma unroll
      for (int fb = 0; fb < 2; ++fb) {
        const int m = c * NFR + 2 * g + fb;
        const bool ok = m >= 0 && m < a.Kp;
        const int fr = ok ? m : 0;
        load_half<CMODE>(X0 + (size_t)fr * blk, X1 + (size_t)fr * blk, pq.has1, l8, frm + 4 * fb);
#pragma unroll
        for (int i = 0; i < 4; ++i) frm[4 * fb + i] = ok ? frm[4 * fb + i] : zero;
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const v4f& s = frm[(r & 4) + (3 - (r & 3))];
        xo[r] = rev_group<8>(v2f{s.z, s.w});
      }
    } else {
      const int n = c * NFR + f;
      const bool ok = n >= 0 && n < a.Kp;
      const int fr = ok ? n : 0;
      load_rowm<CMODE, LB>(X0 + (size_t)fr * blk, X1 + (size_t)fr * blk, pq.has1, l, frm);
#pragma unroll
      for (int i = 0; i < 8; ++i) frm[i] = ok ? frm[i] : zero;
      v2f xo_in[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) xo_in[q] = v2f{frm[q].z, frm[q].w};
      rev_exchange_g<LB, 7>(xo_in, xo);
    }
    C2 z[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const C2 v = {v2f{frm[r].x, frm[r].y}, xo[r]};
      z[r] = cmul(v, reinterpret_cast<const v2f*>(tab + G::I_PRE)[r * 64 + lane]);
    }
    fft_wave_multi<NFR>(z, buf, tab, p1, lane);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const C2 r = cmul_negim(z[j], reinterpret_cast<const v2f*>(tab + G::I_POST)[j * 64 + lane]);
      if (j < 4) {
        now[j] = r.re;
        nxt[j] = r.im;
      } else {
        now[j] = r.im;
        nxt[j] = r.re;
      }
    }
  };
  // every lane receives the value of the lane LB below (the lowest group: of the highest group)
  auto shift_up = [&](const v2f (&v)[8], v2f (&out)[8]) {
    wave_sync();
    {
      char* w = buf + 8 * ((lane + LB) & 63);
#pragma unroll
      for (int j = 0; j < 8; ++j) *reinterpret_cast<v2f*>(w + 512 * j) = v[j];
    }
    wave_sync();
    {
      const char* r = buf + 8 * lane;
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = *reinterpret_cast<const v2f*>(r + 512 * j);
    }
  };

  constexpr int FHs = 8 * LB;   // outputs per block half
  const size_t ts0 = ((size_t)pq.b0 * C + pq.c0) * FHs, ts1 = ((size_t)pq.b1 * C + pq.c1) * FHs;   // stream state rows
  v2f pend[8];   // in the lanes of group 0: the aliased half of the frame before the next chunk
#pragma unroll
  for (int j = 0; j < 8; ++j) pend[j] = v2f{0.f, 0.f};
  if (c0 == 0 && a.tail_in) {
#pragma unroll
    for (int j2 = 0; j2 < 8; ++j2) {
      const int k = l + LB * j2;
      const int j = (j2 < 4) ? (FHs - 1 - 2 * k) : (2 * k - FHs);
      pend[j2].x = a.tail_in[ts0 + j];
      pend[j2].y = pq.has1 ? a.tail_in[ts1 + j] : 0.f;
    }
  }
  if (c0 > 0) {
    v2f now[8], nxt[8];
    dct_chunk(c0 - 1, now, nxt);
    shift_up(nxt, pend);
  }
  for (int c = c0; c < c1; ++c) {
    v2f now[8], nxt[8], sh[8];
    dct_chunk(c, now, nxt);
    shift_up(nxt, sh);
    const int n = c * NFR + f;
    v4f row[8];
    {
      v2f xe[8], xo_in[8], xo[8];
#pragma unroll
      for (int j2 = 0; j2 < 8; ++j2) {
        const v2f cin = (f == 0) ? pend[j2] : sh[j2];
        const v2f ab = reinterpret_cast<const v2f*>(tab + G::I_COEF)[j2 * 64 + lane];
        const v2f o1 = ab.x * now[j2] + ab.y * cin;
        v2f o2;
        if constexpr (FOLD4) {   // F^-1 of a block that is not a rotation: (s3, s4) on their own
          const v2f cd = reinterpret_cast<const v2f*>(a.tab + G::I_TOTAL + G::I_COEF2)[j2 * 64 + lane];
          o2 = cd.x * now[j2] + cd.y * cin;
        } else {
          o2 = ab.y * now[j2] - ab.x * cin;
        }
        xe[(j2 + 4) & 7] = (j2 < 4) ? o2 : o1;
        xo_in[j2] = (j2 < 4) ? o1 : o2;
      }
      rev_exchange_g<LB, 3>(xo_in, xo);
#pragma unroll
      for (int i = 0; i < 8; ++i) row[i] = v4f{xe[i].x, xe[i].y, xo[i].x, xo[i].y};
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) pend[j] = sh[j];
    if (a.tail_out && n == a.nblk - 1) {   // streaming: the last frame's aliased half is the next chunk's state
#pragma unroll
      for (int j2 = 0; j2 < 8; ++j2) {
        const int k = l + LB * j2;
        const int j = (j2 < 4) ? (FHs - 1 - 2 * k) : (2 * k - FHs);
        a.tail_out[ts0 + j] = nxt[j2].x;
        if (pq.has1) a.tail_out[ts1 + j] = nxt[j2].y;
      }
    }
    if (n < a.nblk)
      store_rowm<CMODE, LB>(static_cast<pcm_t*>(a.x) + row_off(pq.b0, a.nblk, n, blk, pq.c0),
                            static_cast<pcm_t*>(a.x) + row_off(pq.b1, a.nblk, n, blk, pq.c1), pq.has1, l, row);
  }
}

}  // namespace

template <int NFR>
static int launch_fwd_multi_N(const FwdMArgs& a, int iof, bool fold4, bool psy, int C, unsigned grid, hipStream_t s) {
  const dim3 blk(AC_WAVES * 64);
  auto go = [&](auto kernel, size_t lds) -> int {
    if (lds > 64 * 1024)
      AC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3(grid), blk, lds, s, a);
    return AC_OK;
  };
  if (psy) {   // fused masking model: float32 tensors, rotation fold blocks (the caller checked)
    const size_t lds = (size_t)AC_WAVES * multi_wave_bytes<NFR, true>() + multi_tab_bytes<NFR, true>() + (size_t)a.rp.lds_words * 4;
    if (C == 2) return go(k_fwd_multi<NFR, 0, AC_WAVES, 0, false, true>, lds);
    return go(k_fwd_multi<NFR, 2, AC_WAVES, 0, false, true>, lds);
  }
  const size_t lds = (size_t)AC_WAVES * WAVE_LDS + Geo<8>::TAB_LDS;
  if (fold4) {
    if (C == 2) return go(k_fwd_multi<NFR, 0, AC_WAVES, 0, true>, lds);
    return go(k_fwd_multi<NFR, 2, AC_WAVES, 0, true>, lds);
  }
  if (iof == 1) {
    if (C == 2) return go(k_fwd_multi<NFR, 0, AC_WAVES, 1>, lds);
    return go(k_fwd_multi<NFR, 2, AC_WAVES, 1>, lds);
  }
  if (C == 2) return go(k_fwd_multi<NFR, 0, AC_WAVES>, lds);
  return go(k_fwd_multi<NFR, 2, AC_WAVES>, lds);
}
// psy (may be null): the plan of the masking model for general band layouts, fused into the launch (fast_multi_fuses())
int launch_fwd_multi(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, int iof, float* X, float* t, float* thr,
                            float drown, const float* prev_block, float* state_out, int B, int Kin, int F, int C, hipStream_t s) {
  const int nfr = fast_mdct_frames_per_wave(p->N);
  FwdMArgs a;
  a.x = x;
  a.X = X;
  a.prev_block = prev_block;
  a.state_out = state_out;
  a.tab = p->d_fast;
  a.Kin = Kin;
  a.F = F;
  a.C = C;
  a.cpp = (F + nfr - 1) / nfr;
  a.nsig = (long long)B * C;
  a.t = t;
  a.thr = thr;
  a.psy_img = psy ? psy->d_runs : nullptr;
  if (psy) a.rp = runs_params(psy, drown, false);
  else a.rp = runs::RunsParams{};
  const long long npairs = (C == 2) ? (long long)B : (a.nsig + 1) / 2;
  a.ntasks = npairs * a.cpp;
  // chunks per wave: the table copy (and the masking model's image) is paid once per workgroup
  static const int tper = [] { const char* e = getenv("AC_FWD_T"); return e ? atoi(e) : 4; }();
  static const int tper_psy = [] { const char* e = getenv("AC_FWD_T_PSY"); return e ? atoi(e) : 4; }();   // (2 ... 8 measure alike)
  int T = psy ? (tper_psy > 0 ? tper_psy : 4) : (tper > 0 ? tper : 4);
  while (T > 1 && a.ntasks < (long long)AC_WAVES * T * p->cus * 2) T >>= 1;
  a.T = T;
  unsigned grid;
  int st = grid_for(a.ntasks, AC_WAVES * T, &grid);
  if (st) return st;
  const bool f4 = p->fold4 != 0;
  if (nfr == 2) st = launch_fwd_multi_N<2>(a, iof, f4, psy != nullptr, C, grid, s);
  else if (nfr == 4) st = launch_fwd_multi_N<4>(a, iof, f4, psy != nullptr, C, grid, s);
  else if (nfr == 8) st = launch_fwd_multi_N<8>(a, iof, f4, psy != nullptr, C, grid, s);
  else st = launch_fwd_multi_N<16>(a, iof, f4, psy != nullptr, C, grid, s);
  if (st) return st;
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

template <int NFR>
static void launch_inv_multi_N(const InvMArgs& a, int iof, bool fold4, int C, unsigned grid, hipStream_t s) {
  const dim3 blk(AC_WAVES * 64);
  if (fold4) {
    if (C == 2) hipLaunchKernelGGL((k_inv_multi<NFR, 0, AC_WAVES, 0, true>), dim3(grid), blk, 0, s, a);
    else hipLaunchKernelGGL((k_inv_multi<NFR, 2, AC_WAVES, 0, true>), dim3(grid), blk, 0, s, a);
    return;
  }
  if (iof == 1) {
    if (C == 2) hipLaunchKernelGGL((k_inv_multi<NFR, 0, AC_WAVES, 1>), dim3(grid), blk, 0, s, a);
    else hipLaunchKernelGGL((k_inv_multi<NFR, 2, AC_WAVES, 1>), dim3(grid), blk, 0, s, a);
    return;
  }
  if (C == 2) hipLaunchKernelGGL((k_inv_multi<NFR, 0, AC_WAVES>), dim3(grid), blk, 0, s, a);
  else hipLaunchKernelGGL((k_inv_multi<NFR, 2, AC_WAVES>), dim3(grid), blk, 0, s, a);
}
int launch_inv_multi(const ac_mdct_plan* p, const float* X, void* x, int iof, const float* tail_in, float* tail_out,
                            int B, int Kp, int nblk, int C, hipStream_t s) {
  const int nfr = fast_mdct_frames_per_wave(p->N);
  InvMArgs a;
  a.X = X;
  a.x = x;
  a.tail_in = tail_in;
  a.tail_out = tail_out;
  a.tab = p->d_fast;
  a.Kp = Kp;
  a.nblk = nblk;
  a.C = C;
  a.cpp = (nblk + nfr - 1) / nfr;
  a.nsig = (long long)B * C;
  const long long npairs = (C == 2) ? (long long)B : (a.nsig + 1) / 2;
  // chunks per strip: every strip but a signal's first pays one more DCT-IV pass for the frame before it
  static const int spc_env = [] { const char* e = getenv("AC_SPC"); return e ? atoi(e) : 0; }();
  int spc = spc_env > 0 ? spc_env : 8;
  while (spc > 1 && npairs * ((a.cpp + spc - 1) / spc) < (long long)AC_WAVES * p->cus * 2) spc >>= 1;
  a.spc = spc;
  a.nstrips = (a.cpp + spc - 1) / spc;
  a.ntasks = npairs * a.nstrips;
  unsigned grid;
  const int st = grid_for(a.ntasks, AC_WAVES, &grid);
  if (st) return st;
  const bool f4 = p->fold4 != 0;
  if (nfr == 2) launch_inv_multi_N<2>(a, iof, f4, C, grid, s);
  else if (nfr == 4) launch_inv_multi_N<4>(a, iof, f4, C, grid, s);
  else if (nfr == 8) launch_inv_multi_N<8>(a, iof, f4, C, grid, s);
  else launch_inv_multi_N<16>(a, iof, f4, C, grid, s);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
