// Device building blocks of the LDS-FFT tier, shared by its run-time forms (ac_mdct_generic.hip) and by the 16-byte kernels with the
// size and the plan known at compile time (ac_wave_v.h and the translation units that instantiate them): the complex pair
// arithmetic, the Stockham passes and the DCT-IV around them, the LDS padding and the LDS sizes per frame.  gfx950 only.
#pragma once
#include "ac_internal.h"

namespace ac {

constexpr int kThreads = 256;
extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];

// ------------------------------------------------------------------------------------------------
// Middle tier: any filters_n from 16 to 4096 whose half is 5-smooth (2^a 3^b 5^c: the powers of two, and the 120 / 240 /
// 480 / 960 and 192 / 576 families of the speech and music codecs) that the wave-level kernels do not serve, with any
// window, the rectangular one included.  Same O(N) fold / unfold as above, the DCT-IV as an N/2-point complex FFT in LDS
// (mixed-radix Stockham -- radix 4 while it divides, then 2, 3, 5 -- fp32), one group of threads per (signal, frame).
// ------------------------------------------------------------------------------------------------
// Two channels of a clip ride side by side (c0, c0 + 1; the last one alone when C is odd): every value is a float2
// over the pair, a complex value a cpair.
__device__ __forceinline__ float2 cis_neg(const float* __restrict__ ctab, int idx, int N) {
  // exp(-i pi idx / (4 N)), 0 <= idx < 8 N, from ctab[i] = cos(pi i / (4 N)):  sin(x) = cos(x - pi/2)
  const int s = idx - 2 * N;
  return make_float2(ctab[idx], -ctab[s < 0 ? -s : s]);
}
struct alignas(16) cpair {   // (16-byte aligned: one ds_read_b128 / ds_write_b128 per value)
  float2 re, im;   // (c0, c1)
};
// (the two channels of a pair as one 2-vector: the compiler then emits packed v_pk_fma_f32 / v_pk_add_f32 / v_pk_mul_f32 --
// half the vector-ALU instructions of the same arithmetic written on .x / .y)
typedef float pk2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pk2 pk(float2 v) { return pk2{v.x, v.y}; }
__device__ __forceinline__ float2 unpk(pk2 v) { return make_float2(v.x, v.y); }
__device__ __forceinline__ cpair cmulw(cpair a, float2 w) {
  const pk2 re = pk(a.re), im = pk(a.im);
  cpair r;
  r.re = unpk(re * w.x - im * w.y);
  r.im = unpk(re * w.y + im * w.x);
  return r;
}
__device__ __forceinline__ float2 ld2(const float* p, int C, bool has1) {   // the pair's two samples at one index
  if (C == 2) return *reinterpret_cast<const float2*>(p);                     // stereo: one 8-byte access
  return make_float2(p[0], has1 ? p[1] : 0.f);
}
__device__ __forceinline__ void st2(float* p, float2 v, int C, bool has1) {
  if (C == 2) {
    *reinterpret_cast<float2*>(p) = v;
    return;
  }
  p[0] = v.x;
  if (has1) p[1] = v.y;
}
// bfloat16 storage: the stereo pair is one 4-byte access
typedef bf16_t bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 ld2(const bf16_t* p, int C, bool has1) {
  if (C == 2) {
    const f2v v = __builtin_convertvector(*reinterpret_cast<const bf16x2_t*>(p), f2v);
    return make_float2(v.x, v.y);
  }
  return make_float2((float)p[0], has1 ? (float)p[1] : 0.f);
}
__device__ __forceinline__ void st2(bf16_t* p, float2 v, int C, bool has1) {
  if (C == 2) {
    *reinterpret_cast<bf16x2_t*>(p) = __builtin_convertvector(f2v{v.x, v.y}, bf16x2_t);
    return;
  }
  p[0] = (bf16_t)v.x;
  if (has1) p[1] = (bf16_t)v.y;
}
// float16 storage (MDCTransformer(compute_dtype=float16): mdctransformer.py:327-344 up-casts such tensors to float32 inside
// the DCT-IV; here all the arithmetic is float32)
typedef f16_t f16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 ld2(const f16_t* p, int C, bool has1) {
  if (C == 2) {
    const f2v v = __builtin_convertvector(*reinterpret_cast<const f16x2_t*>(p), f2v);
    return make_float2(v.x, v.y);
  }
  return make_float2((float)p[0], has1 ? (float)p[1] : 0.f);
}
__device__ __forceinline__ void st2(f16_t* p, float2 v, int C, bool has1) {
  if (C == 2) {
    *reinterpret_cast<f16x2_t*>(p) = __builtin_convertvector(f2v{v.x, v.y}, f16x2_t);
    return;
  }
  p[0] = (f16_t)v.x;
  if (has1) p[1] = (f16_t)v.y;
}

__device__ __forceinline__ cpair cadd(cpair a, cpair b) { return {unpk(pk(a.re) + pk(b.re)), unpk(pk(a.im) + pk(b.im))}; }
__device__ __forceinline__ cpair csub(cpair a, cpair b) { return {unpk(pk(a.re) - pk(b.re)), unpk(pk(a.im) - pk(b.im))}; }
__device__ __forceinline__ cpair cscale(cpair a, float s) { return {unpk(pk(a.re) * s), unpk(pk(a.im) * s)}; }
__device__ __forceinline__ cpair cmul_mi(cpair a) {   // a * (-i)
  return {a.im, unpk(-pk(a.re))};
}
// radix of the next Stockham pass over what is left of the transform length (4 while it divides, then 2, 3, 5)
static inline __host__ __device__ int next_radix(int rem) { return rem % 4 == 0 ? 4 : rem % 2 == 0 ? 2 : rem % 3 == 0 ? 3 : 5; }

// v[N] (LDS, float2 per entry) -> y[k] = sum_m v[m] cos(pi/N (m + 1/2)(k + 1/2)) written back into v;
// A, B: N/2 cpairs each (LDS), tw[k] = exp(-2 pi i k / (N/2)), k < N/2.  Executed by a group of nt threads (tid = index
// inside the group); every group of the workgroup runs it at the same time on its own buffers (the barriers are
// workgroup-wide).  Stockham autosort, decimation in time: a pass of radix r joins r transforms of length L into one of
// length r L -- butterfly j = (p, q), q < L: x_s = src[q + L (p + s m)] W_{rL}^{q s}, m = H / (r L);
// dst[q + L (r p + t)] = sum_s x_s w_r^{s t}.
// B may BE v (the analysis kernel at filters_n > 2048, where a third buffer would leave one workgroup per CU): the
// pre-twiddled input then goes through registers into the buffer from which the passes end in A, so that the last step
// reads A and writes v.
// (ALIAS is a template parameter, not a run-time test: the staging registers of the aliased form cost the other one
// a third of its speed when both share a body)
constexpr int kAliasPerThread = 8;   // N/2 values over 256 threads, N <= 4096
template <bool ALIAS = false>
__device__ void dct4_lds(float2* v, cpair* A, cpair* B, const float* __restrict__ ctab, const float2* __restrict__ tw,
                         int N, int tid, int nt) {
  const int H = N >> 1;
  cpair* src = A;
  cpair* dst = B;
  if constexpr (ALIAS) {
    int passes = 0;
    for (int rem0 = H; rem0 > 1; rem0 /= next_radix(rem0)) ++passes;
    if (passes & 1) {   // an odd number of passes starts in B (= v) and ends in A
      src = B;
      dst = A;
    }
    cpair held[kAliasPerThread];
#pragma unroll
    for (int i = 0; i < kAliasPerThread; ++i) {
      const int n = tid + i * nt;
      if (n < H) {
        cpair t;
        t.re = v[2 * n];
        t.im = v[N - 1 - 2 * n];
        held[i] = cmulw(t, cis_neg(ctab, 4 * n + 1, N));
      }
    }
    __syncthreads();   // every value of v has been read: its bytes may now serve as B
#pragma unroll
    for (int i = 0; i < kAliasPerThread; ++i) {
      const int n = tid + i * nt;
      if (n < H) src[n] = held[i];
    }
  } else {
    for (int n = tid; n < H; n += nt) {
      cpair t;
      t.re = v[2 * n];
      t.im = v[N - 1 - 2 * n];
      A[n] = cmulw(t, cis_neg(ctab, 4 * n + 1, N));   // exp(-i pi (n + 1/4) / N)
    }
  }
  __syncthreads();
  int rem = H;
  for (int L = 1; L < H;) {
    const int r = next_radix(rem);
    const int m = H / (r * L);   // exp(-2 pi i q s / (r L)) = exp(-2 pi i (q s m) / H) = tw[q s m]
    for (int j = tid; j < H / r; j += nt) {
      const int p = j / L, q = j - p * L;
      const cpair* in = src + q + L * p;
      cpair* out = dst + q + L * r * p;
      const cpair x0 = in[0];
      if (r == 4) {
        const cpair x1 = cmulw(in[L * m], tw[q * m]), x2 = cmulw(in[2 * L * m], tw[2 * q * m]);
        const cpair x3 = cmulw(in[3 * L * m], tw[3 * q * m]);
        const cpair t0 = cadd(x0, x2), t1 = csub(x0, x2), t2 = cadd(x1, x3), t3 = cmul_mi(csub(x1, x3));
        out[0] = cadd(t0, t2);
        out[L] = cadd(t1, t3);
        out[2 * L] = csub(t0, t2);
        out[3 * L] = csub(t1, t3);
      } else if (r == 2) {
        const cpair x1 = cmulw(in[L * m], tw[q * m]);
        out[0] = cadd(x0, x1);
        out[L] = csub(x0, x1);
      } else if (r == 3) {
        const cpair x1 = cmulw(in[L * m], tw[q * m]), x2 = cmulw(in[2 * L * m], tw[2 * q * m]);
        const cpair sm = cadd(x1, x2), m1 = csub(x0, cscale(sm, 0.5f));
        const cpair m2 = cscale(cmul_mi(csub(x1, x2)), 0.86602540378443865f);   // -i sin(2 pi / 3) (x1 - x2)
        out[0] = cadd(x0, sm);
        out[L] = cadd(m1, m2);
        out[2 * L] = csub(m1, m2);
      } else {   // 5
        const cpair x1 = cmulw(in[L * m], tw[q * m]), x2 = cmulw(in[2 * L * m], tw[2 * q * m]);
        const cpair x3 = cmulw(in[3 * L * m], tw[3 * q * m]), x4 = cmulw(in[4 * L * m], tw[4 * q * m]);
        const cpair a1 = cadd(x1, x4), a2 = cadd(x2, x3), b1 = csub(x1, x4), b2 = csub(x2, x3);
        constexpr float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;   // cos(2 pi / 5), cos(4 pi / 5)
        constexpr float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;    // sin(2 pi / 5), sin(4 pi / 5)
        const cpair e1 = cadd(x0, cadd(cscale(a1, c1), cscale(a2, c2))), e2 = cadd(x0, cadd(cscale(a1, c2), cscale(a2, c1)));
        const cpair d1 = cmul_mi(cadd(cscale(b1, s1), cscale(b2, s2))), d2 = cmul_mi(csub(cscale(b1, s2), cscale(b2, s1)));
        out[0] = cadd(x0, cadd(a1, a2));
        out[L] = cadd(e1, d1);
        out[2 * L] = cadd(e2, d2);
        out[3 * L] = csub(e2, d2);
        out[4 * L] = csub(e1, d1);
      }
    }
    __syncthreads();
    cpair* t = src;
    src = dst;
    dst = t;
    L *= r;
    rem /= r;
  }
  for (int k = tid; k < H; k += nt) {
    const cpair r = cmulw(src[k], cis_neg(ctab, 4 * k, N));   // exp(-i pi k / N)
    v[2 * k] = r.re;
    v[N - 1 - 2 * k] = make_float2(-r.im.x, -r.im.y);
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// The same transform with one group of <= 64 lanes INSIDE ONE WAVE per frame (filters_n <= 2048): no workgroup barrier
// anywhere in a frame (LDS operations of a wave execute in order; wave_sync only pins the compiler), two or three radix
// stages per LDS round trip -- a pass has a super-radix R = R1 R2 <= 16 (16 = 4 x 4, 15 = 3 x 5, 12 = 4 x 3, 10 = 2 x 5,
// 9 = 3 x 3, 8 = 4 x 2, 6 = 2 x 3, or a plain 5 / 4 / 3 / 2), computed in registers with compile-time inner twiddles, so
// filters_n = 960 takes 3 round trips instead of 5, 480 two -- and padded buffers: element i of a buffer lives at
// i + (i >> 4), which spreads the stride-R writes of the first pass (and every other power-of-two stride) over the banks.
// The fold buffer shares the bytes of the second FFT buffer: 17 N bytes of LDS per frame, 9 frames resident per CU at
// filters_n = 960 (the three-buffer workgroup form above: 6).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// one 16-byte element of padding per 2^ps elements: ps = 4, but 2 at the two sizes where a survey of ps = 2 ... 5 over every
// instance (B = 64 stereo) found another value faster on a second look (120: 0.106 / 0.095 -> 0.089 / 0.087 ms, 36: +5 %;
// four other sizes of the first pass were noise)
#define AC_PAD_SHIFT 4
static inline __host__ __device__ constexpr int pad_shift_ct(int N) { return N == 120 || N == 36 ? 2 : AC_PAD_SHIFT; }
__device__ __forceinline__ int pad16(int i, int ps = AC_PAD_SHIFT) { return i + (i >> ps); }
static inline __host__ __device__ constexpr int padded_len(int n, int ps = AC_PAD_SHIFT) { return n + (n >> ps) + 1; }

// compile-time cos / sin of 2 pi e / R (Taylor series on the angle reduced to [-pi, pi])
constexpr double c_series(double x, bool sine) {
  double term = sine ? x : 1.0, sum = term;
  for (int k = 1; k < 16; ++k) {
    const double a = sine ? 2.0 * k : 2.0 * k - 1.0;
    term *= -x * x / (a * (a + 1.0));
    sum += term;
  }
  return sum;
}
constexpr double c_angle(int e, int R) {
  const int m = ((e % R) + R) % R;
  const double a = 6.283185307179586476925 * (double)m / (double)R;
  return a > 3.14159265358979323846 ? a - 6.283185307179586476925 : a;
}
template <int E, int R> struct Wc {   // exp(-2 pi i E / R)
  static constexpr float re = (float)c_series(c_angle(E, R), false);
  static constexpr float im = (float)(-c_series(c_angle(E, R), true));
};

// small DFTs (forward sign) on R cpairs in natural order, in place
template <int R> __device__ __forceinline__ void dft_small(cpair* a);
template <> __device__ __forceinline__ void dft_small<1>(cpair*) {}
template <> __device__ __forceinline__ void dft_small<2>(cpair* a) {
  const cpair s = cadd(a[0], a[1]), d = csub(a[0], a[1]);
  a[0] = s;
  a[1] = d;
}
template <> __device__ __forceinline__ void dft_small<3>(cpair* a) {
  const cpair sm = cadd(a[1], a[2]), m1 = csub(a[0], cscale(sm, 0.5f));
  const cpair m2 = cscale(cmul_mi(csub(a[1], a[2])), 0.86602540378443865f);   // -i sin(2 pi / 3) (x1 - x2)
  a[0] = cadd(a[0], sm);
  a[1] = cadd(m1, m2);
  a[2] = csub(m1, m2);
}
template <> __device__ __forceinline__ void dft_small<4>(cpair* a) {
  const cpair t0 = cadd(a[0], a[2]), t1 = csub(a[0], a[2]), t2 = cadd(a[1], a[3]), t3 = cmul_mi(csub(a[1], a[3]));
  a[0] = cadd(t0, t2);
  a[1] = cadd(t1, t3);
  a[2] = csub(t0, t2);
  a[3] = csub(t1, t3);
}
template <> __device__ __forceinline__ void dft_small<5>(cpair* a) {
  const cpair a1 = cadd(a[1], a[4]), a2 = cadd(a[2], a[3]), b1 = csub(a[1], a[4]), b2 = csub(a[2], a[3]);
  constexpr float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;   // cos(2 pi / 5), cos(4 pi / 5)
  constexpr float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;    // sin(2 pi / 5), sin(4 pi / 5)
  const cpair e1 = cadd(a[0], cadd(cscale(a1, c1), cscale(a2, c2))), e2 = cadd(a[0], cadd(cscale(a1, c2), cscale(a2, c1)));
  const cpair d1 = cmul_mi(cadd(cscale(b1, s1), cscale(b2, s2))), d2 = cmul_mi(csub(cscale(b1, s2), cscale(b2, s1)));
  a[0] = cadd(a[0], cadd(a1, a2));
  a[1] = cadd(e1, d1);
  a[2] = cadd(e2, d2);
  a[3] = csub(e2, d2);
  a[4] = csub(e1, d1);
}
// inner twiddles W_R^(n2 k1) of the two-stage form, applied row by row with compile-time constants
template <int R1, int R2, int N2, int K1>
struct TwRow {
  static __device__ __forceinline__ void run(cpair* g) {   // g[k1], k1 = 0 .. R1 - 1, for a fixed n2 = N2
    TwRow<R1, R2, N2, K1 - 1>::run(g);
    if constexpr (K1 > 0 && N2 > 0) g[K1] = cmulw(g[K1], make_float2(Wc<N2 * K1, R1 * R2>::re, Wc<N2 * K1, R1 * R2>::im));
  }
};
template <int R1, int R2, int N2>
struct TwRow<R1, R2, N2, -1> {
  static __device__ __forceinline__ void run(cpair*) {}
};
template <int R1, int R2, int N2>
struct Stage1 {   // for n2 = 0 .. N2: DFT_R1 over n1 of x[n1 R2 + n2] (fetched by `load`), times W_R^(n2 k1) -> y[k1 R2 + n2]
  template <class LOAD>
  static __device__ __forceinline__ void run(const LOAD& load, cpair* y) {
    Stage1<R1, R2, N2 - 1>::run(load, y);
    cpair g[R1];
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) g[n1] = load(n1 * R2 + N2);
    dft_small<R1>(g);
    TwRow<R1, R2, N2, R1 - 1>::run(g);
#pragma unroll
    for (int k1 = 0; k1 < R1; ++k1) y[k1 * R2 + N2] = g[k1];
  }
};
template <int R1, int R2>
struct Stage1<R1, R2, -1> {
  template <class LOAD>
  static __device__ __forceinline__ void run(const LOAD&, cpair*) {}
};

// one Stockham pass of super-radix R = R1 R2 joining R transforms of length L (see dct4_lds), by the nt <= 64 lanes of a group
// inside one wave; src / dst padded (pad16).  The R-point DFT runs in registers as R2 DFTs of R1 points (inputs fetched column
// by column), compile-time inner twiddles, R1 DFTs of R2 points (outputs stored row by row):  n = n1 R2 + n2,  k = k1 + R1 k2.
// first: the inputs are the folded frame v itself, element n = v[2 n] + i v[N - 1 - 2 n], times the pre-twiddle
// exp(-i pi (n + 1/4) / N) (no separate pre-twiddle round trip); last_to_v: the outputs go to v in their final form,
// y[2 k] = Re, y[N - 1 - 2 k] = -Im of out[k] exp(-i pi k / N) (no separate post-twiddle round trip).
struct WaveTabs {
  const float2* tw;    // exp(-2 pi i k / (N/2))
  const float2* pre;   // exp(-i pi (n + 1/4) / N)
  const float2* post;  // exp(-i pi k / N)
};
template <int R1, int R2, bool first, bool last_to_v, bool CT = false>
__device__ __forceinline__ void wave_pass(const cpair* __restrict__ src, cpair* __restrict__ dst, float2* v, int N, int L, int H,
                                          const WaveTabs& tb, int tid, int nt, int ps = AC_PAD_SHIFT, int ps_dst = -1) {
  if (ps_dst < 0) ps_dst = ps;   // (ps: the padding of src; ps_dst: of dst, when the two buffers are padded differently)
  constexpr int R = R1 * R2;
  const int m = H / (R * L), nb = H / R;
  const unsigned invL = 0xFFFFFFFFu / (unsigned)L + 1u;   // j / L for j < 2^16 as a multiply-high
  auto butterfly = [&](int j) {
    const int p = L == 1 ? j : (int)__umulhi((unsigned)j, invL), q = j - p * L;
    const int base = q + L * p, tq = q * m, ob = q + L * R * p, Lm = L * m;
    auto load = [&](int s2) {
      const int n = base + Lm * s2;
      if constexpr (first) {   // (L = 1, q = 0: no pass twiddle)
        cpair t;
        t.re = v[2 * n];
        t.im = v[N - 1 - 2 * n];
        return cmulw(t, tb.pre[n]);
      } else {
        const cpair x = src[pad16(n, ps)];
        return s2 > 0 ? cmulw(x, tb.tw[tq * s2]) : x;
      }
    };
    auto store = [&](int t, const cpair& val) {
      const int k = ob + L * t;
      if constexpr (last_to_v) {
        const cpair r = cmulw(val, tb.post[k]);
        v[2 * k] = r.re;
        v[N - 1 - 2 * k] = make_float2(-r.im.x, -r.im.y);
      } else {
        dst[pad16(k, ps_dst)] = val;
      }
    };
    if constexpr (R2 == 1) {
      cpair g[R1];
#pragma unroll
      for (int n1 = 0; n1 < R1; ++n1) g[n1] = load(n1);
      dft_small<R1>(g);
#pragma unroll
      for (int t = 0; t < R1; ++t) store(t, g[t]);
    } else {
      cpair y[R];
      Stage1<R1, R2, R2 - 1>::run(load, y);
#pragma unroll
      for (int k1 = 0; k1 < R1; ++k1) {
        cpair h[R2];
#pragma unroll
        for (int n2 = 0; n2 < R2; ++n2) h[n2] = y[k1 * R2 + n2];
        dft_small<R2>(h);
#pragma unroll
        for (int k2 = 0; k2 < R2; ++k2) store(k1 + R1 * k2, h[k2]);
      }
    }
  };
  if constexpr (CT) {   // N and nt are compile-time constants of the caller: the rounds unroll, the strides fold
    const int rounds = (nb + nt - 1) / nt;
#pragma unroll
    for (int rd = 0; rd < rounds; ++rd) {
      const int j = tid + rd * nt;
      if (j < nb) butterfly(j);
    }
  } else {
    for (int j = tid; j < nb; j += nt) butterfly(j);
  }
}

// the super-radices of a size, chosen on the host (lds_wave_plan): their product is N / 2.  The run-time form takes super-radices
// up to 10 (16 / 15 / 12 take two passes off some sizes but push the kernels past 256 registers); compile-time plans may name them.
struct WavePlan {
  int n;
  unsigned char r[6];
  int nt;   // lanes per frame (a power of two <= 64; 64 / nt frames share a wave)
};

// v[N] (LDS, float2 per entry; its bytes are ALSO buffer Bp) -> DCT-IV written back into v, as dct4_lds.  Ap, Bp: padded_len(N/2)
// cpairs each.  Called by all the lanes of a wave; tid = lane inside its group of nt.
// Buffers: pass 1 reads v (pre-twiddle fused) and writes Ap; the passes then alternate Ap -> Bp -> Ap ...  An even number of
// passes ends with a pass that reads Ap and writes v in final form (post-twiddle fused: v's bytes are Bp's, free by then); an
// odd number ends in Ap, and a separate post-twiddle step writes v.
static __device__ void dct4_wave(float2* v, cpair* Ap, cpair* Bp, const WaveTabs& tb, int N, int tid, int nt, const WavePlan& wp) {
  const int H = N >> 1;
  const bool even = (wp.n & 1) == 0;
  cpair* src = Bp;   // (unused by the first pass)
  cpair* dst = Ap;
  int L = 1;
  for (int ps = 0; ps < wp.n; ++ps) {
    const int r = wp.r[ps];
    const bool first = ps == 0, lastv = even && ps == wp.n - 1;
#define AC_WAVE_PASS(A, B)                                                                   \
  if (first) wave_pass<A, B, true, false>(src, dst, v, N, L, H, tb, tid, nt);                \
  else if (lastv) wave_pass<A, B, false, true>(src, dst, v, N, L, H, tb, tid, nt);           \
  else wave_pass<A, B, false, false>(src, dst, v, N, L, H, tb, tid, nt);                     \
  break
    switch (r) {
      case 10: AC_WAVE_PASS(2, 5);
      case 9: AC_WAVE_PASS(3, 3);
      case 8: AC_WAVE_PASS(4, 2);
      case 6: AC_WAVE_PASS(2, 3);
      case 5: AC_WAVE_PASS(5, 1);
      case 4: AC_WAVE_PASS(4, 1);
      case 3: AC_WAVE_PASS(3, 1);
      default: AC_WAVE_PASS(2, 1);
    }
#undef AC_WAVE_PASS
    wave_sync_lds();
    cpair* t = (ps == 0) ? Bp : src;   // after pass 1 the data is in Ap and Bp (= v, read out) is free
    src = dst;
    dst = t;
    L *= r;
  }
  if (!even) {
    for (int k = tid; k < H; k += nt) {
      const cpair r = cmulw(src[pad16(k)], tb.post[k]);   // src == Ap here
      v[2 * k] = r.re;
      v[N - 1 - 2 * k] = make_float2(-r.im.x, -r.im.y);
    }
    wave_sync_lds();
  }
}

// the same with the size, the lanes per frame and the super-radices known at compile time (R3 / R2 = 0: three / two passes):
// strides, rounds and buffer offsets fold into immediates
template <int R> struct RadixSplit { static constexpr int A = R, B = 1; };
template <> struct RadixSplit<16> { static constexpr int A = 4, B = 4; };
template <> struct RadixSplit<15> { static constexpr int A = 3, B = 5; };
template <> struct RadixSplit<12> { static constexpr int A = 4, B = 3; };
template <> struct RadixSplit<10> { static constexpr int A = 2, B = 5; };
template <> struct RadixSplit<9> { static constexpr int A = 3, B = 3; };
template <> struct RadixSplit<8> { static constexpr int A = 4, B = 2; };
template <> struct RadixSplit<6> { static constexpr int A = 2, B = 3; };
template <int NC, int NTC, int R0, int R1, int R2, int R3>
__device__ __forceinline__ void dct4_wave_ct(float2* v, cpair* Ap, cpair* Bp, const WaveTabs& tb, int tid) {
  constexpr int H = NC / 2, NP = 1 + (R1 > 0) + (R2 > 0) + (R3 > 0);
  static_assert(R0 * (R1 ? R1 : 1) * (R2 ? R2 : 1) * (R3 ? R3 : 1) == H, "the super-radices multiply to N / 2");
  constexpr bool even = (NP & 1) == 0;
  constexpr int PS = pad_shift_ct(NC);
  // The first pass writes its outputs R0 elements apart from lane to lane.  One element of padding per 16 spreads a stride
  // that is a multiple of four over the banks; a stride of 5, 6, 9 or 10 elements already visits all sixteen 16-byte bank
  // groups in eight consecutive lanes, and the padding only folds them onto each other (filters_n = 960, R0 = 10: lanes
  // 0 .. 7 land on groups 0, 10, 5, 15, 10, 5, 15, 10).  So buffer A -- the first pass's target -- is padded only where the
  // first radix asks for it; buffer B (and the later passes' writes: runs of R0 consecutive elements) keeps the padding.
  // Measured (128 stereo clips of 10 s, base -> this): filters_n 600 transform 0.249 -> 0.212 ms, 540 0.244 -> 0.216, 648
  // 0.218 -> 0.200, 360 inverse 0.220 -> 0.202, the other sizes of 32 and 64 lanes per frame within the noise; the frames
  // of 8 and 16 lanes (108, 160) lost 8-15 % on the inverse and keep the padding.  LDS bank-conflict cycles at 960: 35 % of
  // the LDS-active cycles -> 26 %.
  constexpr int PSA = (R0 % 4 == 0 || PS != AC_PAD_SHIFT || NTC < 32) ? PS : 30, PSB = PS;
  // pass 1: v -> Ap; then Ap -> Bp -> Ap ...; an even count ends in v (= Bp's bytes) in final form
  wave_pass<RadixSplit<R0>::A, RadixSplit<R0>::B, true, false, true>(Bp, Ap, v, NC, 1, H, tb, tid, NTC, PSB, PSA);
  wave_sync_lds();
  if constexpr (NP >= 2) {
    wave_pass<RadixSplit<R1>::A, RadixSplit<R1>::B, false, NP == 2, true>(Ap, Bp, v, NC, R0, H, tb, tid, NTC, PSA, PSB);
    wave_sync_lds();
  }
  if constexpr (NP >= 3) {
    wave_pass<RadixSplit<R2>::A, RadixSplit<R2>::B, false, false, true>(Bp, Ap, v, NC, R0 * R1, H, tb, tid, NTC, PSB, PSA);
    wave_sync_lds();
  }
  if constexpr (NP >= 4) {
    wave_pass<RadixSplit<R3>::A, RadixSplit<R3>::B, false, true, true>(Ap, Bp, v, NC, R0 * R1 * R2, H, tb, tid, NTC, PSA, PSB);
    wave_sync_lds();
  }
  if constexpr (!even) {
#pragma unroll
    for (int rd = 0; rd < (H + NTC - 1) / NTC; ++rd) {
      const int k = tid + rd * NTC;
      if (k < H) {
        const cpair r = cmulw(Ap[pad16(k, PSA)], tb.post[k]);
        v[2 * k] = r.re;
        v[NC - 1 - 2 * k] = make_float2(-r.im.x, -r.im.y);
      }
    }
    wave_sync_lds();
  }
}

// ---- the same passes for a frame dealt to NTC = 128 / 256 lanes (two / four waves: filters_n above 1024), IN PLACE in one
// padded buffer that shares the bytes of v: a pass loads and transforms all its butterflies in registers (one or two per
// lane), the group synchronises, then the outputs go back.  8.5 N bytes of LDS per frame; the pre-twiddles are formed from
// the post-twiddle table (exp(-i pi (n + 1/4) / N) = post[n] exp(-i pi / (4 N))): two tables beside the frame, so that
// filters_n = 4096 keeps two workgroups (eight waves) per CU.
template <int NTC>
__device__ __forceinline__ void group_sync() {
  if constexpr (NTC > 64) __syncthreads();
  else wave_sync_lds();
}
template <int NC, int NTC, int L, int R, bool first, bool last_to_v>
__device__ __forceinline__ void group_pass(cpair* buf, float2* v, const WaveTabs& tb, float2 pre0, int tid) {
  constexpr int R1 = RadixSplit<R>::A, R2 = RadixSplit<R>::B;
  constexpr int H = NC / 2, m = H / (R * L), nb = H / R, Lm = L * m, rounds = (nb + NTC - 1) / NTC, PS = pad_shift_ct(NC);
  cpair out[rounds][R];
#pragma unroll
  for (int rd = 0; rd < rounds; ++rd) {
    const int j = tid + rd * NTC;
    if (j < nb) {
      const int p = j / L, q = j - p * L;
      const int base = q + L * p, tq = q * m;
      auto load = [&](int s2) {
        const int n = base + Lm * s2;
        if constexpr (first) {
          cpair t;
          t.re = v[2 * n];
          t.im = v[NC - 1 - 2 * n];
          const float2 w = tb.post[n];
          return cmulw(t, make_float2(w.x * pre0.x - w.y * pre0.y, w.x * pre0.y + w.y * pre0.x));
        } else {
          const cpair x = buf[pad16(n, PS)];
          return s2 > 0 ? cmulw(x, tb.tw[tq * s2]) : x;
        }
      };
      if constexpr (R2 == 1) {
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) out[rd][n1] = load(n1);
        dft_small<R1>(out[rd]);
      } else {
        cpair y[R];
        Stage1<R1, R2, R2 - 1>::run(load, y);
#pragma unroll
        for (int k1 = 0; k1 < R1; ++k1) {
          cpair h[R2];
#pragma unroll
          for (int n2 = 0; n2 < R2; ++n2) h[n2] = y[k1 * R2 + n2];
          dft_small<R2>(h);
#pragma unroll
          for (int k2 = 0; k2 < R2; ++k2) out[rd][k1 + R1 * k2] = h[k2];
        }
      }
    }
  }
  group_sync<NTC>();
#pragma unroll
  for (int rd = 0; rd < rounds; ++rd) {
    const int j = tid + rd * NTC;
    if (j < nb) {
      const int p = j / L, q = j - p * L, ob = q + L * R * p;
#pragma unroll
      for (int t = 0; t < R; ++t) {
        const int k = ob + L * t;
        if constexpr (last_to_v) {
          const cpair r = cmulw(out[rd][t], tb.post[k]);
          v[2 * k] = r.re;
          v[NC - 1 - 2 * k] = make_float2(-r.im.x, -r.im.y);
        } else {
          buf[pad16(k, PS)] = out[rd][t];
        }
      }
    }
  }
  group_sync<NTC>();
}
template <int NC, int NTC, int R0, int R1, int R2, int R3>
__device__ __forceinline__ void dct4_group_ct(float2* v, cpair* buf, const WaveTabs& tb, float2 pre0, int tid) {
  constexpr int H = NC / 2, NP = 1 + (R1 > 0) + (R2 > 0) + (R3 > 0);
  static_assert(R0 * (R1 ? R1 : 1) * (R2 ? R2 : 1) * (R3 ? R3 : 1) == H, "the super-radices multiply to N / 2");
  static_assert(NP >= 2, "at least two passes (the first reads v, the last writes it)");
  group_pass<NC, NTC, 1, R0, true, false>(buf, v, tb, pre0, tid);
  group_pass<NC, NTC, R0, R1, false, NP == 2>(buf, v, tb, pre0, tid);
  if constexpr (NP >= 3) group_pass<NC, NTC, R0 * R1, R2, false, NP == 3>(buf, v, tb, pre0, tid);
  if constexpr (NP >= 4) group_pass<NC, NTC, R0 * R1 * R2, R3, false, true>(buf, v, tb, pre0, tid);
}

// LDS floats per frame of the wave form: Bp (= v) and Ap, padded; of the in-place form above: one buffer
// a frame on several waves is transformed in place in one buffer.  Frames inside a wave keep two buffers: in place, with half
// the LDS per frame and twice the frames resident, the tier ran within +-3 % of the two-buffer form at every size measured
// (B = 256 stereo, 20 sizes 24 ... 1024: 960 0.467 / 0.479 -> 0.461 / 0.456 ms, 600 0.420 -> 0.462, 720 0.447 -> 0.428): with 9
// or 18 frames resident the kernels run at the rate of a device copy of the same tensors (0.38 ms), so residency is not the limit.
static inline __host__ __device__ constexpr bool wave_in_place(int ntc) { return ntc > 64; }
static inline __host__ __device__ constexpr int wave_floats_per_group(int N, int ps = AC_PAD_SHIFT) { return 2 * 4 * padded_len(N / 2, ps); }
static inline __host__ __device__ constexpr int group_floats_per_frame(int N, int ps = AC_PAD_SHIFT) { return 4 * padded_len(N / 2, ps); }

// the FFT's twiddles exp(-2 pi i k / (N/2)), k < N/2, once per workgroup into LDS (every thread takes part; the caller
// synchronises before the first use)
__device__ __forceinline__ void fill_twiddles(float2* tw, const float* __restrict__ ctab, int N) {
  for (int k = threadIdx.x; k < N / 2; k += kThreads) tw[k] = cis_neg(ctab, 16 * k, N);   // exp(-i pi (16 k) / (4 N))
}

// threads per group: a power of two (a workgroup holds kThreads / nt groups) near the N/8 butterflies of a radix-4
// stage, at least one wave
static inline __host__ __device__ int lds_group_threads(int N) {
  int nt = 64;
  while (nt < kThreads && nt < N / 8) nt <<= 1;
  return nt;
}

// LDS floats per group of the analysis kernel: v [N float2] + A + B; beyond filters_n 2048 B shares v's bytes (measured:
// N = 4096 0.679 -> 0.495 ms, two workgroups per CU instead of one; at smaller sizes the third buffer is faster)
constexpr int kLdsAliasAbove = 2048;
static inline __host__ __device__ int lds_fwd_floats_per_group(int N) { return N > kLdsAliasAbove ? 4 * N : 6 * N; }

}  // namespace ac
