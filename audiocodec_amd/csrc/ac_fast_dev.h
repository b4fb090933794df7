// Wave-level kernels for filters_n = 1024 and 2048 on gfx950 (MI355X); the description below is for 1024
// (8 complex FFT points per lane), 2048 runs the same code with 16 (template parameter R).
//
// One 64-lane wavefront transforms one frame of two signals at a time (the two channels of a stereo clip, or two
// mono signals): both ride in the two halves of 64-bit register pairs (v2f = (s0, s1)), so twiddles, window
// coefficients, addresses and LDS traffic are shared.
//
// Data movement per frame, q = 64 i + lane being the 16-byte granule (x[2q], x[2q+1]) x (s0, s1) that lane `lane`
// loads / stores with one coalesced 16-byte access per i:
//   * analysis loads blocks n-1 and n of the PCM.  FFT element e = lane + 64 r needs, from each block, the even sample
//     of granule e + 256 (same lane, another register) and the odd sample of granule 767 - e (lane 63 - lane): only
//     the odd halves cross lanes, through one lane-reversal exchange in LDS (ds_write_b64 / ds_read_b64);
//   * window fold with two coefficients per element (Princen-Bradley windows: the 2x2 fold blocks are rotations);
//   * pre-twiddle -> 512-point complex FFT as three in-register radix-8 passes with two padded, conflict-free LDS
//     exchanges whose addresses are one per-lane base + an immediate -> post-twiddle; the output bin of
//     (lane, register k2) is lane + 64 k2, so the even coefficients X[2k] are already where the store wants
//     them and only the odd ones (X[N-1-2k]) take the lane-reversal exchange again;
//   * coalesced 16-byte stores of X; the psychoacoustic epilogue (tonality, Bark sums, spreading, threshold)
//     runs on the frame in registers; the band x band spreading product runs on the matrix cores by default
//     (spread_mfma: split-bf16 v_mfma_f32_4x4x4_16b_bf16) or as f32 multiply-adds (AC_SPREAD_F32);
//   * the same kernels take 16-bit PCM (IOF 1) or bfloat16 tensors (IOF 2): the conversion sits in the row loads / stores;
//   * synthesis carries the aliased half of a frame's DCT-IV in registers along a short strip of output blocks.
// Frames are dealt to waves in order, so the chip works on one contiguous window of every tensor (DESIGN_LOG.md section 9).
//
// Index maps and their bank behaviour are emulated lane by lane in tests/emulate_wave_fft.py.
// Reference formulas: mdctransformer.py:62-153 (closed forms in SURVEY.md App. A), psychoacoustic.py:102-210,301-331.
//
// This header: build parameters, table geometry, the wave FFT, lane reversals and row movement shared by every kernel
// family of the tier (ac_fast_fwd / _inv / _duplex / _psy / _multi .hip); the table images are built in ac_fast_plan.hip.
#pragma once
#include <type_traits>

#include "ac_internal.h"
#include "ac_quant_dev.h"

namespace ac {
namespace {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef const float* gtab_t;   // LDS-resident table image

// build parameters (set through CXXFLAGS, e.g. tools/build_variant.sh NAME -DAC_WPE=2): defined here and nowhere else, so
// that every object of the tier sees the same values
#ifndef AC_WAVES_PSY
#define AC_WAVES_PSY 4              // waves per workgroup, fused encode (LDS: three workgroups per CU)
#endif
#ifndef AC_WAVES
#define AC_WAVES 4                  // waves per workgroup, plain transform / inverse / stand-alone psycho
#endif
#ifndef AC_WPE
#define AC_WPE 3                    // waves per SIMD the register allocator must leave room for
#endif
#ifndef AC_NT_STORE
#define AC_NT_STORE 1               // 1: streaming (non-temporal) stores of the output rows (measured +4 % on both kernels)
#endif
constexpr int WAVE_LDS = 9216;      // bytes of LDS per wave: 576 x 16-byte elements (8 rows of 64 + 8 pad)
constexpr int S8_OFF = 8192;        // psycho: 128 chunk sums (8 bins each) behind the 8 KB intensity image
constexpr int ZERO_OFF = 9216;      // psycho: one zero slot (padding target of the gather lists)
constexpr int WAVE_LDS_PSY = 9232;
constexpr int MF_COPY_STRIDE = 288;               // bytes between the four shifted copies of the reversed bf16 prototype
constexpr int MF_TAB_BYTES = 4 * MF_COPY_STRIDE;  // one table (hi or lo parts)
constexpr float kEps = 1e-14f;      // _INTENSITY_EPS, psychoacoustic.py:56

// ---- geometry and mdct tables for R complex FFT points per lane: filters_n = 128 R (R = 8: 1024, R = 16: 2048).
// Two table images in ac_mdct_plan::d_fast (analysis at 0, synthesis at I_TOTAL floats); the kernel copies the first
// I_LDS floats of its image into LDS once per workgroup, so the frame loop touches HBM only for PCM / spectra.
template <int R>
struct Geo {
  static constexpr int FH = 64 * R;                 // complex FFT points per frame
  static constexpr int FN = 128 * R;                // filters_n
  static constexpr int I_P2 = 0;                    // [8][8]  float2  W64^(e0 k1)
  static constexpr int I_POST = I_P2 + 128;         // [R][64] float2  exp(-i pi k / N) * (1/(N sqrt 2) | 2 sqrt 2), k = lane + 64 j
  static constexpr int I_COEF = I_POST + 128 * R;   // [R][64] float2  fold (A, B)(e) | unfold (a, b)(k)
  static constexpr int I_PRE = I_COEF + 128 * R;    // [R][64] float2  exp(-i pi (e + 1/4) / N), e = lane + 64 r
  static constexpr int I_P1 = I_PRE + 128 * R;      // [R][64] float2  W_{64R}^(lane k0), pass-1 twiddles
  // the other two coefficients of a fold block that is not a rotation (float32-precomputed or rectangular windows; FOLD4
  // kernels read them from global memory: the image is L2-resident): analysis (cE, cO)(e) | synthesis (s3, s4)(k)
  static constexpr int I_COEF2 = I_P1 + 128 * R;    // [R][64] float2
  static constexpr int I_TOTAL = I_COEF2 + 128 * R; // floats per image in global memory
  // R = 8 holds the seven pass-1 twiddles of a lane in registers (LDS is the scarcer resource: 3 workgroups per CU);
  // R = 16 reads its fifteen from LDS (registers are: 64 for the frame alone)
  static constexpr bool P1_IN_REGS = (R == 8);
  static constexpr int I_LDS = P1_IN_REGS ? I_P1 : I_COEF2;   // floats that live in LDS (R = 8: 12 800 bytes)
  // a kernel short of LDS leaves the pre-twiddles out as well (I_LDS_NOPRE floats) and forms them as
  // PRE[e] = POST[e] * (exp(-i pi / (4 N)) / scale): four more packed multiply-adds per element
  static constexpr int I_LDS_NOPRE = I_PRE;
  static constexpr int TAB_LDS = I_LDS * 4;
};
// waves per SIMD the register allocator must leave room for: the strided any-channel-count variants (CMODE 1) and the
// 2048-filter kernels get the larger budget
template <int R, int CMODE, bool PSY = false, int SPREAD = 0>
constexpr int wpe() { return (R == 8 && (CMODE == 0 || (CMODE == 2 && !PSY))) ? AC_WPE : 2; }


typedef short v4s __attribute__((ext_vector_type(4)));
typedef __bf16 v2b __attribute__((ext_vector_type(2)));

struct C2 {   // one complex value for both channels of the pair
  v2f re, im;
};

__device__ __forceinline__ void wave_sync() {
  // LDS operations of one wave execute in order; this only pins the compiler's ordering of
  // cross-lane communication through LDS
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ C2 cmul(const C2& x, const v2f w) {
  C2 r;
  r.re = x.re * w.x - x.im * w.y;
  r.im = x.re * w.y + x.im * w.x;
  return r;
}
// (re, -im) of x * w: the sign rides on the operand modifiers of the multiply-add instead of a separate negation
__device__ __forceinline__ C2 cmul_negim(const C2& x, const v2f w) {
  C2 r;
  r.re = x.re * w.x - x.im * w.y;
  r.im = (-x.re) * w.y - x.im * w.x;
  return r;
}
__device__ __forceinline__ C2 cadd(const C2& a, const C2& b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ C2 csub(const C2& a, const C2& b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ C2 mul_mi(const C2& a) { return {a.im, -a.re}; }   // a * (-i)

// 8-point DFT (forward sign) of the eight registers, outputs in natural order
__device__ __forceinline__ void dft8(C2 (&x)[8]) {
  constexpr float R = 0.70710678118654752440f;
  C2 a0 = cadd(x[0], x[4]), a4 = csub(x[0], x[4]);
  C2 a1 = cadd(x[1], x[5]), a5 = csub(x[1], x[5]);
  C2 a2 = cadd(x[2], x[6]), a6 = csub(x[2], x[6]);
  C2 a3 = cadd(x[3], x[7]), a7 = csub(x[3], x[7]);
  a5 = {(a5.re + a5.im) * R, (a5.im - a5.re) * R};     // * W8^1
  a6 = mul_mi(a6);                                      // * W8^2
  a7 = {(a7.im - a7.re) * R, -(a7.re + a7.im) * R};    // * W8^3
  {
    C2 c0 = cadd(a0, a2), c2 = csub(a0, a2), c1 = cadd(a1, a3), c3 = mul_mi(csub(a1, a3));
    x[0] = cadd(c0, c1);
    x[4] = csub(c0, c1);
    x[2] = cadd(c2, c3);
    x[6] = csub(c2, c3);
  }
  {
    C2 c0 = cadd(a4, a6), c2 = csub(a4, a6), c1 = cadd(a5, a7), c3 = mul_mi(csub(a5, a7));
    x[1] = cadd(c0, c1);
    x[5] = csub(c0, c1);
    x[3] = cadd(c2, c3);
    x[7] = csub(c2, c3);
  }
}

__device__ __forceinline__ void lds_put(char* p, const C2& v) {
  *reinterpret_cast<v4f*>(p) = v4f{v.re.x, v.re.y, v.im.x, v.im.y};
}
__device__ __forceinline__ C2 lds_get(const char* p) {
  const v4f t = *reinterpret_cast<const v4f*>(p);
  return {v2f{t.x, t.y}, v2f{t.z, t.w}};
}

// 16-point DFT (forward sign): two 8-point DFTs of the even / odd registers and one radix-2 stage
__device__ __forceinline__ void dft16(C2 (&x)[16]) {
  C2 e[8], o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    e[i] = x[2 * i];
    o[i] = x[2 * i + 1];
  }
  dft8(e);
  dft8(o);
  constexpr float c1 = 0.92387953251128675613f, s1 = 0.38268343236508977173f, R2 = 0.70710678118654752440f;
  const v2f w[8] = {v2f{1.f, 0.f}, v2f{c1, -s1}, v2f{R2, -R2}, v2f{s1, -c1},
                    v2f{0.f, -1.f}, v2f{-s1, -c1}, v2f{-R2, -R2}, v2f{-c1, -s1}};   // W16^k
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const C2 t = (k == 0) ? o[0] : (k == 4) ? mul_mi(o[4]) : cmul(o[k], w[k]);
    x[k] = cadd(e[k], t);
    x[k + 8] = csub(e[k], t);
  }
}
__device__ __forceinline__ void dft_regs(C2 (&x)[8]) { dft8(x); }
__device__ __forceinline__ void dft_regs(C2 (&x)[16]) { dft16(x); }

// 64R-point FFT of z[r] = element (lane + 64 r); result z[j] = bin lane + 64 j.
// Element index e = e0 + 8 e1 + 64 r (lane = e0 + 8 e1), bin k = k0 + R (k1 + 8 k2), k0 = 8 beta + kappa.
//   pass 1 over r -> k0 (radix R in registers), twiddle W_{64R}^(lane k0);
//   per batch beta of eight k0: exchange 1: row kappa (72 elements of 16 B: 64 + 8 pad), column lane;
//     lane (a = kappa, m0 = e0) reads e1 = 0..7 at a 72 + 8 e1 + m0;  pass 2 over e1 -> k1, twiddle W64^(e0 k1);
//   per half h of the k1 (k1 = (64/R) h + kk): exchange 2: element (k0, kk, e0) at 9 (k0 + R kk) + e0;
//     lane k0 + R kk reads its 8 consecutive e0;  pass 3 over e0 -> k2;  bin = lane + 64 (h + (R/8) k2).
// Every exchange address is one per-lane base + an immediate, and every access is bank-conflict-free under the
// gfx950 lane-group rules (tests/emulate_wave_fft.py emulates the maps for R = 8 and 16).
template <int R>
__device__ __forceinline__ void fft_wave(C2 (&z)[R], char* buf, gtab_t tab, const v2f (&p1)[R], int lane) {
  constexpr int NB = R / 8;      // batches of eight 64-point FFTs
  constexpr int Q = 64 / R;      // k1 values per exchange-2 half
  const int a = lane >> 3, m0 = lane & 7;
  dft_regs(z);
#pragma unroll
  for (int k = 1; k < R; ++k)
    z[k] = cmul(z[k], Geo<R>::P1_IN_REGS ? p1[k] : reinterpret_cast<const v2f*>(tab + Geo<R>::I_P1)[k * 64 + lane]);
#pragma unroll
  for (int beta = 0; beta < NB; ++beta) {
    C2 y[8];
    wave_sync();
    {
      char* w1 = buf + 16 * lane;
#pragma unroll
      for (int k = 0; k < 8; ++k) lds_put(w1 + 1152 * k, z[8 * beta + k]);
    }
    wave_sync();
    {
      const char* r1 = buf + 16 * (a * 72 + m0);
#pragma unroll
      for (int r = 0; r < 8; ++r) y[r] = lds_get(r1 + 128 * r);
    }
    dft8(y);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      z[8 * beta + k] = (k == 0) ? y[0] : cmul(y[k], reinterpret_cast<const v2f*>(tab + Geo<R>::I_P2)[k * 8 + m0]);
  }
  C2 out[R];
#pragma unroll
  for (int h = 0; h < NB; ++h) {
    C2 y[8];
    wave_sync();
    {
      char* w2 = buf + 16 * (9 * a + m0);
#pragma unroll
      for (int beta = 0; beta < NB; ++beta)
#pragma unroll
        for (int kk = 0; kk < Q; ++kk) lds_put(w2 + 16 * (72 * beta + 9 * R * kk), z[8 * beta + Q * h + kk]);
    }
    wave_sync();
    {
      const char* r2 = buf + 144 * lane;
#pragma unroll
      for (int r = 0; r < 8; ++r) y[r] = lds_get(r2 + 16 * r);
    }
    dft8(y);
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) out[h + NB * k2] = y[k2];
  }
#pragma unroll
  for (int j = 0; j < R; ++j) z[j] = out[j];
}

// the lane's pass-1 twiddles W_{64R}^(lane k), k = 1..R-1, from the image in global memory
template <int R>
__device__ __forceinline__ void load_p1(const float* __restrict__ image, int lane, v2f (&p1)[R]) {
  p1[0] = v2f{1.f, 0.f};
#pragma unroll
  for (int k = 1; k < R; ++k)
    p1[k] = Geo<R>::P1_IN_REGS ? reinterpret_cast<const v2f*>(image + Geo<R>::I_P1)[k * 64 + lane] : v2f{0.f, 0.f};
}

// lane-reversal exchange of R (c0, c1) pairs: afterwards out[i] = in[(OFS - i) mod R] of lane 63 - lane
template <int OFS, int R>
__device__ __forceinline__ void rev_exchange(char* buf, int lane, const v2f (&in)[R], v2f (&out)[R]) {
  wave_sync();
  {
    char* w = buf + 8 * (63 - lane);
#pragma unroll
    for (int c = 0; c < R; ++c) *reinterpret_cast<v2f*>(w + 512 * c) = in[c];
  }
  wave_sync();
  {
    const char* r = buf + 8 * lane;
#pragma unroll
    for (int i = 0; i < R; ++i) out[i] = *reinterpret_cast<const v2f*>(r + 512 * ((OFS - i) & (R - 1)));
  }
}

// ---- the two signals a wave transforms side by side, and global <-> register movement of one natural-order row ----
// CMODE 0: exactly two channels: the pair is (clip b, channels 0 and 1), rows are interleaved 16-byte vectors.
// CMODE 1: any channel count: signals s = b C + c are paired in order, (2p, 2p+1), across clip boundaries when C is
//          odd (mono: two clips per wave), so no half of the packed registers idles except in one last odd pair;
//          rows are read with stride C from one base pointer per signal.
// CMODE 2: exactly one channel: as CMODE 1 with the two samples of a granule read / written as one 8-byte vector.
struct Pair {
  long long b0, b1;   // clips of the two signals
  int c0, c1;         // their channels
  bool has1;          // false: the second slot is the padding of an odd signal count
};
template <int CMODE>
__device__ __forceinline__ Pair make_pair(long long p, int C, long long nsig) {
  Pair q;
  if (CMODE == 0) {
    q.b0 = q.b1 = p;
    q.c0 = 0;
    q.c1 = 1;
    q.has1 = true;
  } else if (CMODE == 2) {   // one channel: signal = clip (no 64-bit divisions on the scalar unit)
    const long long s0 = 2 * p, s1 = s0 + 1;
    q.has1 = s1 < nsig;
    q.b0 = s0;
    q.b1 = q.has1 ? s1 : s0;
    q.c0 = q.c1 = 0;
  } else {
    const long long s0 = 2 * p, s1 = s0 + 1;
    q.has1 = s1 < nsig;
    q.b0 = s0 / C;
    q.c0 = (int)(s0 % C);
    q.b1 = q.has1 ? s1 / C : q.b0;
    q.c1 = q.has1 ? (int)(s1 % C) : q.c0;
  }
  return q;
}
// row of signal slot i of a [clips, rows_per_clip, N, C] tensor (floats per row over all channels = blk)
__device__ __forceinline__ size_t row_off(long long b, long long rows_per_clip, long long row, size_t blk, int c) {
  return ((size_t)b * (size_t)rows_per_clip + (size_t)row) * blk + (size_t)c;
}

template <int CMODE, int R = 8>
__device__ __forceinline__ void load_row(const float* __restrict__ r0, const float* __restrict__ r1, int C, bool has1,
                                         int lane, v4f (&v)[R]) {
  if (CMODE == 0) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int q = 64 * i + lane;
      v[i] = reinterpret_cast<const v4f*>(r0)[q];
    }
  } else if (CMODE == 2) {
    // one wave-uniform branch for the second signal (only the last pair of an odd signal count lacks it)
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const v2f u = reinterpret_cast<const v2f*>(r0)[64 * i + lane];
      v[i] = v4f{u.x, 0.f, u.y, 0.f};
    }
    if (has1) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const v2f w = reinterpret_cast<const v2f*>(r1)[64 * i + lane];
        v[i].y = w.x;
        v[i].w = w.y;
      }
    }
  } else {
    // uniform base per register + two 32-bit lane offsets shared by all registers (keeps the addresses out of VGPRs)
    const int off = 2 * lane * C;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const size_t step = (size_t)(128 * i) * C;
      v[i] = v4f{r0[step + off], 0.f, r0[step + off + C], 0.f};
    }
    if (has1) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const size_t step = (size_t)(128 * i) * C;
        v[i].y = r1[step + off];
        v[i].w = r1[step + off + C];
      }
    }
  }
}

template <int CMODE, int R = 8, bool NTS = (AC_NT_STORE != 0)>
__device__ __forceinline__ void store_row(float* __restrict__ r0, float* __restrict__ r1, int C, bool has1, int lane,
                                          const v4f (&v)[R]) {
  if (CMODE == 0) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int q = 64 * i + lane;
      if (NTS) __builtin_nontemporal_store(v[i], reinterpret_cast<v4f*>(r0) + q);
      else reinterpret_cast<v4f*>(r0)[q] = v[i];
    }
  } else if (CMODE == 2) {
#pragma unroll
    for (int i = 0; i < R; ++i) reinterpret_cast<v2f*>(r0)[64 * i + lane] = v2f{v[i].x, v[i].z};
    if (has1) {
#pragma unroll
      for (int i = 0; i < R; ++i) reinterpret_cast<v2f*>(r1)[64 * i + lane] = v2f{v[i].y, v[i].w};
    }
  } else {
    const int off = 2 * lane * C;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const size_t step = (size_t)(128 * i) * C;
      r0[step + off] = v[i].x;
      r0[step + off + C] = v[i].z;
    }
    if (has1) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const size_t step = (size_t)(128 * i) * C;
        r1[step + off] = v[i].y;
        r1[step + off + C] = v[i].w;
      }
    }
  }
}

// ---- the same rows in 2-byte storage: 16-bit PCM (x = pcm / 32768; pcm = to_pcm16(x), ac_internal.h) or bfloat16 ------
typedef short s4 __attribute__((ext_vector_type(4)));
typedef short s2 __attribute__((ext_vector_type(2)));
constexpr float kPcmScale = 1.0f / 32768.0f;
struct Pcm16Fmt {
  static __device__ __forceinline__ float dec(short h) { return (float)h * kPcmScale; }
  static __device__ __forceinline__ s2 enc2(float a, float b) { return s2{to_pcm16(a), to_pcm16(b)}; }
};
struct Bf16Fmt {   // storage = the upper half of the float32 pattern; stores round to nearest even (v_cvt_pk_bf16_f32)
  static __device__ __forceinline__ float dec(short h) { return __uint_as_float((uint32_t)(uint16_t)h << 16); }
  static __device__ __forceinline__ s2 enc2(float a, float b) {
    return __builtin_bit_cast(s2, __builtin_convertvector(v2f{a, b}, v2b));
  }
};

template <typename FMT, int CMODE, int R>
__device__ __forceinline__ void load_row_h(const int16_t* __restrict__ r0, const int16_t* __restrict__ r1, int C,
                                           bool has1, int lane, v4f (&v)[R]) {
  if (CMODE == 0) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const s4 p = reinterpret_cast<const s4*>(r0)[64 * i + lane];
      v[i] = v4f{FMT::dec(p.x), FMT::dec(p.y), FMT::dec(p.z), FMT::dec(p.w)};
    }
  } else if (CMODE == 2) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const s2 u = reinterpret_cast<const s2*>(r0)[64 * i + lane];
      v[i] = v4f{FMT::dec(u.x), 0.f, FMT::dec(u.y), 0.f};
    }
    if (has1) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const s2 w = reinterpret_cast<const s2*>(r1)[64 * i + lane];
        v[i].y = FMT::dec(w.x);
        v[i].w = FMT::dec(w.y);
      }
    }
  } else {
    const int off = 2 * lane * C;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const size_t step = (size_t)(128 * i) * C;
      v[i] = v4f{FMT::dec(r0[step + off]), 0.f, FMT::dec(r0[step + off + C]), 0.f};
    }
    if (has1) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const size_t step = (size_t)(128 * i) * C;
        v[i].y = FMT::dec(r1[step + off]);
        v[i].w = FMT::dec(r1[step + off + C]);
      }
    }
  }
}

template <typename FMT, int CMODE, int R>
__device__ __forceinline__ void store_row_h(int16_t* __restrict__ r0, int16_t* __restrict__ r1, int C, bool has1,
                                            int lane, const v4f (&v)[R]) {
  if (CMODE == 0) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const s2 lo = FMT::enc2(v[i].x, v[i].y), hi = FMT::enc2(v[i].z, v[i].w);
      reinterpret_cast<s4*>(r0)[64 * i + lane] = s4{lo.x, lo.y, hi.x, hi.y};
    }
  } else if (CMODE == 2) {
#pragma unroll
    for (int i = 0; i < R; ++i) reinterpret_cast<s2*>(r0)[64 * i + lane] = FMT::enc2(v[i].x, v[i].z);
    if (has1) {
#pragma unroll
      for (int i = 0; i < R; ++i) reinterpret_cast<s2*>(r1)[64 * i + lane] = FMT::enc2(v[i].y, v[i].w);
    }
  } else {
    const int off = 2 * lane * C;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const size_t step = (size_t)(128 * i) * C;
      const s2 e = FMT::enc2(v[i].x, v[i].z);
      r0[step + off] = e.x;
      r0[step + off + C] = e.y;
    }
    if (has1) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const size_t step = (size_t)(128 * i) * C;
        const s2 e = FMT::enc2(v[i].y, v[i].w);
        r1[step + off] = e.x;
        r1[step + off + C] = e.y;
      }
    }
  }
}
// ---- a row of quantised spectra (ac_quant.hip): int16 codes and int8 scale factors, dequantised where the frame is used
// -- X^ = fp32(code * step(sf)), the product ac_dequantize forms (ac_quant_dev.h).  A granule holds the raw codes and
// scale factors of (2q, s0), (2q, s1), (2q+1, s0), (2q+1, s1) -- the element order of load_row -- so a prefetch of the next
// frame only issues loads.  bw[i] packs the bands of bins 2q (low half) and 2q+1, q = 64 i + lane: frame-invariant, held in
// registers for the whole strip.  sf0 / sf1 address the frame's scale-factor row [M, C] at the signal's channel.
struct QGran {
  s4 code;
  uint32_t sfw;   // four scale-factor bytes, same order
};
template <int CMODE, int R>
__device__ __forceinline__ void load_row_q(const int16_t* __restrict__ r0, const int16_t* __restrict__ r1,
                                           const int8_t* __restrict__ sf0, const int8_t* __restrict__ sf1,
                                           const uint32_t (&bw)[R], bool has1, int lane, QGran (&g)[R]) {
  static_assert(CMODE == 0 || CMODE == 2, "quantised spectra: mono / stereo");
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int q = 64 * i + lane;
    const int j0 = (int)(bw[i] & 0xffffu), j1 = (int)(bw[i] >> 16);
    if (CMODE == 0) {   // [M][2]: the two channels' scale factors of a band are one 16-bit word
      g[i].code = reinterpret_cast<const s4*>(r0)[q];
      g[i].sfw = (uint32_t)*reinterpret_cast<const uint16_t*>(sf0 + 2 * j0) |
                 ((uint32_t)*reinterpret_cast<const uint16_t*>(sf0 + 2 * j1) << 16);
    } else {
      const s2 u = reinterpret_cast<const s2*>(r0)[q];
      g[i].code = s4{u.x, 0, u.y, 0};
      g[i].sfw = (uint32_t)(uint8_t)sf0[j0] | ((uint32_t)(uint8_t)sf0[j1] << 16);
    }
  }
  if (CMODE == 2 && has1) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const s2 w = reinterpret_cast<const s2*>(r1)[64 * i + lane];
      g[i].code.y = w.x;
      g[i].code.w = w.y;
      g[i].sfw |= ((uint32_t)(uint8_t)sf1[bw[i] & 0xffffu] << 8) | ((uint32_t)(uint8_t)sf1[bw[i] >> 16] << 24);
    }
  }
}
template <int R>
__device__ __forceinline__ void dequant_frame(const QGran (&g)[R], v4f (&v)[R]) {
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const uint32_t w = g[i].sfw;
    v[i] = v4f{dequant(g[i].code.x, (int8_t)(w & 0xff)), dequant(g[i].code.y, (int8_t)((w >> 8) & 0xff)),
               dequant(g[i].code.z, (int8_t)((w >> 16) & 0xff)), dequant(g[i].code.w, (int8_t)(w >> 24))};
  }
}

// IOF: 0 = float32 tensors; 1 = 16-bit PCM on the PCM side (spectra float32); 2 = bfloat16 tensors throughout
template <int IOF> struct RowFmt { using type = Pcm16Fmt; };
template <> struct RowFmt<2> { using type = Bf16Fmt; };

// wave-wide sum, result uniform (scalar register): xor butterflies inside each row of 16 lanes, then the two
// row broadcasts of the DPP unit; no LDS traffic
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {   // v + v[lane permuted by a DPP pattern] on the enabled rows
  const int iv = __builtin_bit_cast(int, v);
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, iv, CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum(float v) {
  v = dpp_add<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]  (lane ^ 1)
  v = dpp_add<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]  (lane ^ 2)
  v = dpp_add<0x141, 0xf>(v);   // row_half_mirror      (other quad of the 8)
  v = dpp_add<0x140, 0xf>(v);   // row_mirror           (other half of the 16): every lane holds its row's sum
  v = dpp_add<0x142, 0xa>(v);   // row_bcast15 into rows 1, 3: row 1 = r0 + r1, row 3 = r2 + r3
  v = dpp_add<0x143, 0xc>(v);   // row_bcast31 into rows 2, 3: row 3 = total
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

__device__ __forceinline__ float fast_log2(float x) { return __builtin_amdgcn_logf(x); }     // v_log_f32
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }    // v_exp_f32
__device__ __forceinline__ v2f log2v(v2f x) { return v2f{fast_log2(x.x), fast_log2(x.y)}; }
__device__ __forceinline__ v2f exp2v(v2f x) { return v2f{fast_exp2(x.x), fast_exp2(x.y)}; }
__device__ __forceinline__ v2f maxv(v2f a, float b) { return v2f{fmaxf(a.x, b), fmaxf(a.y, b)}; }

// keeps the unpacking of a loop-invariant word inside the loop (hoisted, the 16 addresses would cost 16 registers)
__device__ __forceinline__ uint32_t in_loop(uint32_t w) {
  asm volatile("" : "+v"(w));
  return w;
}

// copies the table image (and the psy image) into the workgroup's LDS behind the wave buffers; every thread takes part
template <int NW, int WSTRIDE, int TABF, int PSYW, int PSY_TOTAL = 0, int MFB = 0>
__device__ __forceinline__ void load_tables(char* lds, const float* __restrict__ image, const uint32_t* psy_tab) {
  if (image) {
    v4f* dst = reinterpret_cast<v4f*>(lds + NW * WSTRIDE);
    const v4f* src = reinterpret_cast<const v4f*>(image);
    for (int i = threadIdx.x; i < TABF / 4; i += NW * 64) dst[i] = src[i];
  }
  if (psy_tab) {
    uint4* pd = reinterpret_cast<uint4*>(lds + NW * WSTRIDE + (image ? TABF * 4 : 0));
    const uint4* ps = reinterpret_cast<const uint4*>(psy_tab);
    for (int i = threadIdx.x; i < PSYW / 4; i += NW * 64) pd[i] = ps[i];
    if (MFB > 0) {   // the bf16 tiles of spread_mfma, behind the psy image
      const uint4* ms = reinterpret_cast<const uint4*>(psy_tab + PSY_TOTAL);
      for (int i = threadIdx.x; i < MFB / 16; i += NW * 64) pd[PSYW / 4 + i] = ms[i];
    }
  }
  __syncthreads();
}

}  // namespace
}  // namespace ac
