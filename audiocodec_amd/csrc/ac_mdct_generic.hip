// The filter bank below the wave-level FFT kernels (ac_fast_*.hip): any even N, any channel count, in float32, float64 and on
// bfloat16 / float16 tensors.  The generic kernels are an O(N^2) direct DCT-IV: the path for the sizes nothing else covers and an
// independent on-device cross-check for the rest.  Also here: the run-time forms of the LDS-FFT middle tier (the 16-byte kernels
// with compile-time plans are instantiated in ac_wave_*.hip) and the dispatch between the tiers, with the host plan and geometry
// helpers of ac_wave_v.h.  gfx950 only.
#include <algorithm>
#include <cstdlib>

#include "ac_generic_dev.h"
#include "ac_wave_v.h"

namespace ac {

// ------------------------------------------------------------------------------------------------
// analysis: fold (mdctransformer.py:118,349-368 in closed form) + DCT-IV (:311-347) + scale (:125)
// one workgroup per (signal = b*C + c, frame n)
// ------------------------------------------------------------------------------------------------
template <typename TIO, typename TC = typename Compute<TIO>::type>
static __global__ __launch_bounds__(kThreads) void k_fwd_generic(const TIO* __restrict__ x, TIO* __restrict__ X,
                                                          const TIO* __restrict__ prev_block,
                                                          const TC* __restrict__ coef,
                                                          const TC* __restrict__ ctab, int Kin, int F, int C,
                                                          int N) {
  TC* v = reinterpret_cast<TC*>(smem_raw);  // [N]
  const int h = N >> 1;
  const long long wg = blockIdx.x;
  const int n = (int)(wg % F);
  const long long sig = wg / F;
  const int c = (int)(sig % C);
  const long long b = sig / C;
  const TC* a1 = coef;
  const TC* a2 = coef + h;
  const TC* a3 = coef + 2 * h;
  const TC* a4 = coef + 3 * h;

  const bool has_cur = n < Kin;
  const TIO* xc = x + ((size_t)b * Kin + (size_t)n) * N * C + c;              // block n
  const TIO* xp = nullptr;                                                     // block n-1
  if (n >= 1) xp = x + ((size_t)b * Kin + (size_t)(n - 1)) * N * C + c;
  else if (prev_block) xp = prev_block + (size_t)b * N * C + c;

  for (int j = threadIdx.x; j < h; j += kThreads) {
    TC vc = 0, vp = 0;
    if (has_cur) vc = a1[j] * ldv(xc + (size_t)j * C) + a2[j] * ldv(xc + (size_t)(N - 1 - j) * C);
    if (xp) vp = a3[j] * ldv(xp + (size_t)(h - 1 - j) * C) + a4[j] * ldv(xp + (size_t)(h + j) * C);
    v[h + j] = vc;
    v[j] = vp;
  }
  __syncthreads();

  const unsigned mod = 8u * (unsigned)N;
  const double scale = 1.0 / ((double)N * 1.4142135623730951);   // 1/sqrt(4N) * sqrt(2/N)
  TIO* Xo = X + (((size_t)b * F + (size_t)n) * N) * C + c;
  for (int k = threadIdx.x; k < N; k += kThreads) {
    const unsigned step = (unsigned)((2ull * (2ull * k + 1ull)) % mod);
    unsigned idx = (unsigned)((2ull * k + 1ull) % mod);   // (2m+1)(2k+1) at m = 0
    double acc = 0.0;
    for (int m = 0; m < N; ++m) {
      acc += (double)v[m] * (double)ctab[idx];
      idx += step;
      if (idx >= mod) idx -= mod;
    }
    stv(Xo + (size_t)k * C, (TC)(acc * scale));
  }
}

// ------------------------------------------------------------------------------------------------
// synthesis: scale (mdctransformer.py:145) + DCT-IV + unfold/overlap-add (:148 in closed form)
// one workgroup per (signal, output block n); block n = nblk only writes the new stream state
// ------------------------------------------------------------------------------------------------
template <typename TIO, typename TC = typename Compute<TIO>::type>
static __global__ __launch_bounds__(kThreads) void k_inv_generic(const TIO* __restrict__ X, TIO* __restrict__ x,
                                                          const TC* __restrict__ tail_in,
                                                          TC* __restrict__ tail_out,
                                                          const TC* __restrict__ coef,
                                                          const TC* __restrict__ ctab, int Kp, int nblk,
                                                          int nwg_per_sig, int C, int N) {
  TC* Xn = reinterpret_cast<TC*>(smem_raw);   // [N] frame n
  TC* Xm = Xn + N;                            // [N] frame n-1
  const int h = N >> 1;
  const long long wg = blockIdx.x;
  const int n = (int)(wg % nwg_per_sig);
  const long long sig = wg / nwg_per_sig;
  const int c = (int)(sig % C);
  const long long b = sig / C;
  const TC* s1 = coef + 4 * h;
  const TC* s2 = coef + 5 * h;
  const TC* s3 = coef + 6 * h;
  const TC* s4 = coef + 7 * h;

  const bool has_n = n < Kp && n < nblk;   // the virtual state block (n == nblk) has no current frame
  const bool has_m = n >= 1;
  for (int k = threadIdx.x; k < N; k += kThreads) {
    Xn[k] = has_n ? (TC)ldv(X + (((size_t)b * Kp + (size_t)n) * N + k) * C + c) : (TC)0;
    Xm[k] = has_m ? (TC)ldv(X + (((size_t)b * Kp + (size_t)(n - 1)) * N + k) * C + c) : (TC)0;
  }
  __syncthreads();

  const unsigned mod = 8u * (unsigned)N;
  const double scale = 2.0 * 1.4142135623730951;   // sqrt(4N) * sqrt(2/N)
  for (int j = threadIdx.x; j < h; j += kThreads) {
    double a = 0.0, bb = 0.0;
    if (has_n) {   // u_n[h-1-j]
      const unsigned long long mm = 2ull * (unsigned)(h - 1 - j) + 1ull;
      const unsigned step = (unsigned)((2ull * mm) % mod);
      unsigned idx = (unsigned)(mm % mod);
      for (int k = 0; k < N; ++k) {
        a += (double)Xn[k] * (double)ctab[idx];
        idx += step;
        if (idx >= mod) idx -= mod;
      }
      a *= scale;
    }
    if (has_m) {   // u_{n-1}[h+j]
      const unsigned long long mm = 2ull * (unsigned)(h + j) + 1ull;
      const unsigned step = (unsigned)((2ull * mm) % mod);
      unsigned idx = (unsigned)(mm % mod);
      for (int k = 0; k < N; ++k) {
        bb += (double)Xm[k] * (double)ctab[idx];
        idx += step;
        if (idx >= mod) idx -= mod;
      }
      bb *= scale;
    } else if (tail_in) {
      bb = (double)tail_in[((size_t)b * C + c) * h + j];
    }
    if (n < nblk) {
      TIO* xo = x + (((size_t)b * nblk + (size_t)n) * N) * C + c;
      stv(xo + (size_t)j * C, (TC)((double)s1[j] * a + (double)s2[j] * bb));
      stv(xo + (size_t)(N - 1 - j) * C, (TC)((double)s3[j] * a + (double)s4[j] * bb));
    } else if (tail_out) {
      tail_out[((size_t)b * C + c) * h + j] = (TC)bb;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Middle tier: any filters_n from 16 to 4096 whose half is 5-smooth (2^a 3^b 5^c: the powers of two, and the 120 / 240 /
// 480 / 960 and 192 / 576 families of the speech and music codecs) that the wave-level kernels do not serve, with any
// window, the rectangular one included.  Same O(N) fold / unfold as above, the DCT-IV as an N/2-point complex FFT in LDS
// (mixed-radix Stockham -- radix 4 while it divides, then 2, 3, 5 -- fp32), one group of threads per (signal, frame); the
// FFT itself is in ac_lds_fft_dev.h.
// ------------------------------------------------------------------------------------------------
// one group per (clip, channel pair, frame); ALIAS: the form for filters_n > 2048 (a kernel of its own: see dct4_lds)
template <typename TIO, bool ALIAS = false>
static __global__ __launch_bounds__(kThreads) void k_fwd_lds(const TIO* __restrict__ x, TIO* __restrict__ X,
                                                      const TIO* __restrict__ prev_block,
                                                      const float* __restrict__ coef,
                                                      const float* __restrict__ ctab, int Kin, int F, int C, int CP,
                                                      int N, long long ntasks) {
  float* smem = reinterpret_cast<float*>(smem_raw);
  const int nt = lds_group_threads(N), grp = threadIdx.x / nt, tid = threadIdx.x - grp * nt;
  const int per = ALIAS ? 4 * N : 6 * N;                   // (= lds_fwd_floats_per_group(N)) second FFT buffer aliased to v or not
  float2* tw = reinterpret_cast<float2*>(smem + (size_t)(kThreads / nt) * per);   // [N/2] behind the groups' buffers
  fill_twiddles(tw, ctab, N);
  float* base = smem + (size_t)grp * per;
  float2* v = reinterpret_cast<float2*>(base);             // [N]
  cpair* A = reinterpret_cast<cpair*>(base + 2 * N);       // [N/2]
  cpair* Bf = ALIAS ? reinterpret_cast<cpair*>(base) : reinterpret_cast<cpair*>(base + 4 * N);   // [N/2]
  const int h = N >> 1;
  const long long task_raw = (long long)blockIdx.x * (kThreads / nt) + grp;
  const bool valid = task_raw < ntasks;
  const long long wg = valid ? task_raw : ntasks - 1;      // idle groups of the last workgroup only join the barriers
  const int n = (int)(wg % F);
  const long long sig = wg / F;
  const int c = 2 * (int)(sig % CP);
  const bool has1 = c + 1 < C;
  const long long b = sig / CP;
  const float* a1 = coef;
  const float* a2 = coef + h;
  const float* a3 = coef + 2 * h;
  const float* a4 = coef + 3 * h;
  const bool has_cur = n < Kin;
  const TIO* xc = x + ((size_t)b * Kin + (size_t)n) * N * C + c;
  const TIO* xp = nullptr;
  if (n >= 1) xp = x + ((size_t)b * Kin + (size_t)(n - 1)) * N * C + c;
  else if (prev_block) xp = prev_block + (size_t)b * N * C + c;
  for (int j = tid; j < h; j += nt) {
    float2 vc = make_float2(0.f, 0.f), vp = make_float2(0.f, 0.f);
    if (has_cur) {
      const float2 p = ld2(xc + (size_t)j * C, C, has1), q = ld2(xc + (size_t)(N - 1 - j) * C, C, has1);
      vc = make_float2(a1[j] * p.x + a2[j] * q.x, a1[j] * p.y + a2[j] * q.y);
    }
    if (xp) {
      const float2 p = ld2(xp + (size_t)(h - 1 - j) * C, C, has1), q = ld2(xp + (size_t)(h + j) * C, C, has1);
      vp = make_float2(a3[j] * p.x + a4[j] * q.x, a3[j] * p.y + a4[j] * q.y);
    }
    v[h + j] = vc;
    v[j] = vp;
  }
  __syncthreads();
  dct4_lds<ALIAS>(v, A, Bf, ctab, tw, N, tid, nt);
  if (!valid) return;
  const float scale = (float)(1.0 / ((double)N * 1.4142135623730951));   // 1/sqrt(4N) * sqrt(2/N)
  TIO* Xo = X + (((size_t)b * F + (size_t)n) * N) * C + c;
  for (int k = tid; k < N; k += nt) st2(Xo + (size_t)k * C, make_float2(v[k].x * scale, v[k].y * scale), C, has1);
}

// one group per (clip, channel pair, strip of `seg` output blocks): the aliased half of the previous frame's DCT-IV
// stays in LDS along the strip, so a strip of T blocks costs T + 1 transforms; the block index nblk (one past the
// last) only writes the new stream state.  Every group runs the same number of transforms (barriers are workgroup-wide).
template <typename TIO>
static __global__ __launch_bounds__(kThreads) void k_inv_lds(const TIO* __restrict__ X, TIO* __restrict__ x,
                                                      const float* __restrict__ tail_in, float* __restrict__ tail_out,
                                                      const float* __restrict__ coef, const float* __restrict__ ctab,
                                                      int Kp, int nblk, int seg, int nseg, int C, int CP, int N,
                                                      long long ntasks) {
  float* smem = reinterpret_cast<float*>(smem_raw);
  const int nt = lds_group_threads(N), grp = threadIdx.x / nt, tid = threadIdx.x - grp * nt;
  float2* tw = reinterpret_cast<float2*>(smem + (size_t)(kThreads / nt) * 7 * N);   // [N/2] behind the groups' buffers
  fill_twiddles(tw, ctab, N);
  float* base = smem + (size_t)grp * 7 * N;
  float2* v = reinterpret_cast<float2*>(base);             // [N]
  cpair* A = reinterpret_cast<cpair*>(base + 2 * N);       // [N/2]
  cpair* Bf = reinterpret_cast<cpair*>(base + 4 * N);      // [N/2]
  float2* um = reinterpret_cast<float2*>(base + 6 * N);    // [N/2]  u_{n-1}[h + j]
  const int h = N >> 1;
  const long long task_raw = (long long)blockIdx.x * (kThreads / nt) + grp;
  const bool valid = task_raw < ntasks;
  const long long wg = valid ? task_raw : ntasks - 1;
  const int sgm = (int)(wg % nseg);
  const long long sig = wg / nseg;
  const int c = 2 * (int)(sig % CP);
  const bool has1 = c + 1 < C;
  const long long b = sig / CP;
  const float* s1 = coef + 4 * h;
  const float* s2 = coef + 5 * h;
  const float* s3 = coef + 6 * h;
  const float* s4 = coef + 7 * h;
  const float scale = 2.0f * 1.4142135623730951f;   // sqrt(4N) * sqrt(2/N)
  const int nlast = nblk + (tail_out ? 1 : 0);      // blocks incl. the virtual state block
  const int n0 = sgm * seg;
  const size_t ts = ((size_t)b * C + c) * h;        // stream state rows of the pair: ts, ts + h
  // aliased half before the strip: frame n0 - 1, the stream state, or zero
  {
    const bool halo = n0 >= 1;
    const TIO* Xi = X + (((size_t)b * Kp + (size_t)(halo ? n0 - 1 : 0)) * N) * C + c;
    for (int k = tid; k < N; k += nt) v[k] = halo ? ld2(Xi + (size_t)k * C, C, has1) : make_float2(0.f, 0.f);
    __syncthreads();
    dct4_lds(v, A, Bf, ctab, tw, N, tid, nt);
    for (int j = tid; j < h; j += nt) {
      if (halo) um[j] = make_float2(v[h + j].x * scale, v[h + j].y * scale);
      else um[j] = tail_in ? make_float2(tail_in[ts + j], has1 ? tail_in[ts + h + j] : 0.f) : make_float2(0.f, 0.f);
    }
    __syncthreads();
  }
  for (int t = 0; t < seg; ++t) {
    const int n = n0 + t;
    const bool live = valid && n < nlast;    // this group still has a block to write
    const bool has_n = n < Kp && n < nblk;   // the virtual state block (n == nblk) has no current frame
    {
      const TIO* Xi = X + (((size_t)b * Kp + (size_t)(has_n ? n : 0)) * N) * C + c;
      for (int k = tid; k < N; k += nt) v[k] = has_n ? ld2(Xi + (size_t)k * C, C, has1) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    dct4_lds(v, A, Bf, ctab, tw, N, tid, nt);
    if (live) {
      for (int j = tid; j < h; j += nt) {
        const float2 a = make_float2(v[h - 1 - j].x * scale, v[h - 1 - j].y * scale);   // u_n[h-1-j]
        const float2 bb = um[j];                                                        // u_{n-1}[h+j]
        if (n < nblk) {
          TIO* xo = x + (((size_t)b * nblk + (size_t)n) * N) * C + c;
          st2(xo + (size_t)j * C, make_float2(s1[j] * a.x + s2[j] * bb.x, s1[j] * a.y + s2[j] * bb.y), C, has1);
          st2(xo + (size_t)(N - 1 - j) * C, make_float2(s3[j] * a.x + s4[j] * bb.x, s3[j] * a.y + s4[j] * bb.y), C, has1);
        } else if (tail_out) {
          tail_out[ts + j] = bb.x;
          if (has1) tail_out[ts + h + j] = bb.y;
        }
      }
    }
    __syncthreads();
    for (int j = tid; j < h; j += nt) um[j] = make_float2(v[h + j].x * scale, v[h + j].y * scale);
    __syncthreads();
  }
}

// ---- the wave form of the two kernels above (filters_n <= 2048): a group of wp.nt lanes inside one wave per frame / strip,
// several tasks per group so that the twiddle table is built once per workgroup; no workgroup barrier after that
template <typename TIO>
static __global__ __launch_bounds__(kThreads, 2) void k_fwd_wave(const TIO* __restrict__ x, TIO* __restrict__ X,
                                                       const TIO* __restrict__ prev_block, const float* __restrict__ coef,
                                                       const float* __restrict__ ctab, int Kin, int F, int C, int CP, int N,
                                                       long long ntasks, int T, WavePlan wp) {
  float* smem = reinterpret_cast<float*>(smem_raw);
  const int nt = wp.nt, gpw = (int)blockDim.x / nt, grp = threadIdx.x / nt, tid = threadIdx.x - grp * nt;
  const int per = wave_floats_per_group(N), h = N >> 1;
  float2* tw = reinterpret_cast<float2*>(smem + (size_t)gpw * per);   // three tables of N/2 behind the groups' buffers
  for (int k = threadIdx.x; k < h; k += blockDim.x) {
    tw[k] = cis_neg(ctab, 16 * k, N);            // exp(-2 pi i k / (N/2))
    tw[h + k] = cis_neg(ctab, 4 * k + 1, N);     // exp(-i pi (k + 1/4) / N)
    tw[2 * h + k] = cis_neg(ctab, 4 * k, N);     // exp(-i pi k / N)
  }
  __syncthreads();
  const WaveTabs tb = {tw, tw + h, tw + 2 * h};
  float* base = smem + (size_t)grp * per;
  float2* v = reinterpret_cast<float2*>(base);                                   // [N], sharing the bytes of Bp
  cpair* Bp = reinterpret_cast<cpair*>(base);
  cpair* Ap = reinterpret_cast<cpair*>(base + 4 * padded_len(h));
  const float *a1 = coef, *a2 = coef + h, *a3 = coef + 2 * h, *a4 = coef + 3 * h;
  const float scale = (float)(1.0 / ((double)N * 1.4142135623730951));   // 1/sqrt(4N) * sqrt(2/N)
  for (int t = 0; t < T; ++t) {
    const long long wg = ((long long)blockIdx.x * T + t) * gpw + grp;
    if (wg >= ntasks) return;
    const int n = (int)(wg % F);
    const long long sig = wg / F;
    const int c = 2 * (int)(sig % CP);
    const bool has1 = c + 1 < C;
    const long long b = sig / CP;
    const bool has_cur = n < Kin;
    const TIO* xc = x + ((size_t)b * Kin + (size_t)n) * N * C + c;
    const TIO* xp = nullptr;
    if (n >= 1) xp = x + ((size_t)b * Kin + (size_t)(n - 1)) * N * C + c;
    else if (prev_block) xp = prev_block + (size_t)b * N * C + c;
    // the frame's PCM in batches of eight steps: all the loads of a batch are in flight together (a wave that waits for
    // each step's loads in turn keeps a few hundred bytes in flight, and the tier ran at a quarter of the memory rate)
    for (int j0 = tid; j0 < h; j0 += 8 * nt) {
      float2 pc[8], qc[8], pp[8], qp[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int j = j0 + i * nt;
        pc[i] = qc[i] = pp[i] = qp[i] = make_float2(0.f, 0.f);
        if (j < h) {
          if (has_cur) {
            pc[i] = ld2(xc + (size_t)j * C, C, has1);
            qc[i] = ld2(xc + (size_t)(N - 1 - j) * C, C, has1);
          }
          if (xp) {
            pp[i] = ld2(xp + (size_t)(h - 1 - j) * C, C, has1);
            qp[i] = ld2(xp + (size_t)(h + j) * C, C, has1);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int j = j0 + i * nt;
        if (j < h) {
          v[h + j] = make_float2(a1[j] * pc[i].x + a2[j] * qc[i].x, a1[j] * pc[i].y + a2[j] * qc[i].y);
          v[j] = make_float2(a3[j] * pp[i].x + a4[j] * qp[i].x, a3[j] * pp[i].y + a4[j] * qp[i].y);
        }
      }
    }
    wave_sync_lds();
    dct4_wave(v, Ap, Bp, tb, N, tid, nt, wp);
    TIO* Xo = X + (((size_t)b * F + (size_t)n) * N) * C + c;
    for (int k = tid; k < N; k += nt) st2(Xo + (size_t)k * C, make_float2(v[k].x * scale, v[k].y * scale), C, has1);
    wave_sync_lds();   // v is read out before the next task folds into it
  }
}

template <typename TIO>
static __global__ __launch_bounds__(kThreads, 2) void k_inv_wave(const TIO* __restrict__ X, TIO* __restrict__ x,
                                                       const float* __restrict__ tail_in, float* __restrict__ tail_out,
                                                       const float* __restrict__ coef, const float* __restrict__ ctab,
                                                       int Kp, int nblk, int seg, int nseg, int C, int CP, int N,
                                                       long long ntasks, WavePlan wp) {
  float* smem = reinterpret_cast<float*>(smem_raw);
  const int nt = wp.nt, gpw = (int)blockDim.x / nt, grp = threadIdx.x / nt, tid = threadIdx.x - grp * nt;
  const int h = N >> 1, per = wave_floats_per_group(N) + N;   // + um [N/2] float2
  float2* tw = reinterpret_cast<float2*>(smem + (size_t)gpw * per);
  for (int k = threadIdx.x; k < h; k += blockDim.x) {
    tw[k] = cis_neg(ctab, 16 * k, N);
    tw[h + k] = cis_neg(ctab, 4 * k + 1, N);
    tw[2 * h + k] = cis_neg(ctab, 4 * k, N);
  }
  __syncthreads();
  const WaveTabs tb = {tw, tw + h, tw + 2 * h};
  float* base = smem + (size_t)grp * per;
  float2* v = reinterpret_cast<float2*>(base);
  cpair* Bp = reinterpret_cast<cpair*>(base);
  cpair* Ap = reinterpret_cast<cpair*>(base + 4 * padded_len(h));
  float2* um = reinterpret_cast<float2*>(base + wave_floats_per_group(N));   // u_{n-1}[h + j]
  const long long wg = (long long)blockIdx.x * gpw + grp;
  if (wg >= ntasks) return;
  const int sgm = (int)(wg % nseg);
  const long long sig = wg / nseg;
  const int c = 2 * (int)(sig % CP);
  const bool has1 = c + 1 < C;
  const long long b = sig / CP;
  const float *s1 = coef + 4 * h, *s2 = coef + 5 * h, *s3 = coef + 6 * h, *s4 = coef + 7 * h;
  const float scale = 2.0f * 1.4142135623730951f;   // sqrt(4N) * sqrt(2/N)
  const int nlast = nblk + (tail_out ? 1 : 0);      // blocks incl. the virtual state block
  const int n0 = sgm * seg;
  const size_t ts = ((size_t)b * C + c) * h;        // stream state rows of the pair: ts, ts + h
  // aliased half before the strip: the stream state or zero for a signal's first strip, else frame n0 - 1 (step t = -1 of
  // the loop below: one call site of the transform)
  if (n0 == 0) {
    for (int j = tid; j < h; j += nt)
      um[j] = tail_in ? make_float2(tail_in[ts + j], has1 ? tail_in[ts + h + j] : 0.f) : make_float2(0.f, 0.f);
    wave_sync_lds();
  }
  for (int t = (n0 >= 1 ? -1 : 0); t < seg; ++t) {
    const int n = n0 + t;
    if (t >= 0 && n >= nlast) break;         // nothing left to write
    const bool has_n = t < 0 || (n < Kp && n < nblk);   // the virtual state block (n == nblk) has no current frame
    {
      const TIO* Xi = X + (((size_t)b * Kp + (size_t)(has_n ? n : 0)) * N) * C + c;
      for (int k0 = tid; k0 < N; k0 += 16 * nt) {   // sixteen loads in flight per lane (see k_fwd_wave)
        float2 r[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int k = k0 + i * nt;
          r[i] = (has_n && k < N) ? ld2(Xi + (size_t)k * C, C, has1) : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int k = k0 + i * nt;
          if (k < N) v[k] = r[i];
        }
      }
    }
    wave_sync_lds();
    if (has_n) dct4_wave(v, Ap, Bp, tb, N, tid, nt, wp);   // (the DCT-IV of a zero frame is zero)
    if (t >= 0) {
      for (int j = tid; j < h; j += nt) {
        const float2 a = make_float2(v[h - 1 - j].x * scale, v[h - 1 - j].y * scale);   // u_n[h-1-j]
        const float2 bb = um[j];                                                        // u_{n-1}[h+j]
        if (n < nblk) {
          TIO* xo = x + (((size_t)b * nblk + (size_t)n) * N) * C + c;
          st2(xo + (size_t)j * C, make_float2(s1[j] * a.x + s2[j] * bb.x, s1[j] * a.y + s2[j] * bb.y), C, has1);
          st2(xo + (size_t)(N - 1 - j) * C, make_float2(s3[j] * a.x + s4[j] * bb.x, s3[j] * a.y + s4[j] * bb.y), C, has1);
        } else if (tail_out) {
          tail_out[ts + j] = bb.x;
          if (has1) tail_out[ts + h + j] = bb.y;
        }
      }
      wave_sync_lds();
    }
    for (int j = tid; j < h; j += nt) um[j] = make_float2(v[h + j].x * scale, v[h + j].y * scale);
    wave_sync_lds();
  }
}

// ------------------------------------------------------------------------------------------------
// tier rules and launchers
// ------------------------------------------------------------------------------------------------
// even, from 16 to 4096, half of it 5-smooth (8 N floats of LDS <= 128 KB of the CU's 160 KB): the LDS-FFT middle tier applies
static bool lds_fft_ok(int N) {
  if (N < 16 || N > 4096 || (N & 1)) return false;
  int h = N / 2;
  for (int r : {2, 3, 5})
    while (h % r == 0) h /= r;
  return h == 1;
}

int check_grid(long long n) {
  if (n <= 0) return 1;
  if (n > 2147483647ll) {
    set_error("problem too large for one launch (%lld workgroups)", n);
    return AC_EINVAL;
  }
  return 0;
}

// ---- the wave form of the LDS-FFT tier (filters_n <= 2048) ------------------------------------------------------------
#ifndef AC_LDS_WAVE_MAX
#define AC_LDS_WAVE_MAX 2048   // (0: the workgroup form everywhere, for A/B measurements)
#endif
// Which of the two forms serves a size is measured, not derived (profiles/r3/lds_fft_tier_sizes.txt, B = 64
// stereo, 10 s, same process).  float32 stereo rows with filters_n % 4 == 0 up to 1024 take the 16-byte wave kernels wherever
// the tier applies (every such size at 2.2 - 6.0 TB/s; the workgroup form 1.3 - 2.0).  Other layouts (mono, more channels,
// bfloat16) run the 8-byte wave kernels where they measured faster: the analysis up to filters_n = 1024 except where a frame
// gets 16 lanes and three passes (N / 2 from 97 to 127), the synthesis up to 1536.  AC_LDS_WAVE_MAX (tuning hook; 0: the
// workgroup form everywhere) caps both.
static bool lds_wave_vec_shape(int N, int C, bool f32) {
  return f32 && C >= 1 && N % 4 == 0 && (N <= 1024 || lds_wave_ct_size(N));   // (above 1024: the in-place instances only)
}
static int lds_wave_max() {
  static const int wave_max = [] { const char* e = getenv("AC_LDS_WAVE_MAX"); return e ? atoi(e) : AC_LDS_WAVE_MAX; }();
  return wave_max;
}
static bool lds_wave_ok(int N, bool synthesis, int C, bool f32) {
  const int wave_max = lds_wave_max();
  if (wave_max <= 0) return false;
  if (lds_wave_vec_shape(N, C, f32) && (lds_fft_ok(N) || lds_wave_ct_size(N))) return true;   // (instances reach 8192, the tier's other forms 4096)
  if (!lds_fft_ok(N) || N > wave_max) return false;
  const int H = N / 2;
  return synthesis ? N <= 1536 : (N <= 1024 && !(H > 96 && H < 128));
}

// the table itself is AC_WAVE_CT_SIZES (ac_wave_v.h)
bool lds_wave_ct_size(int N) {
#define AC_WAVE_CT(NC, NTC, R0, R1, R2, R3) \
  if (N == NC) return true;
  AC_WAVE_CT_SIZES
#undef AC_WAVE_CT
  return false;
}
bool wave_ct_off() {
  static const int off = [] { const char* e = getenv("AC_LDS_WAVE_NOCT"); return e ? atoi(e) : 0; }();   // (A/B measurements)
  return off != 0;
}
// super-radices of N / 2 (a pass of radix r runs (N / 2) / r butterflies of r points in registers): the factorisation with
// the least estimated work -- every pass costs a round trip through LDS, a butterfly ~ r (log2 r + 3) operations, and the
// butterflies of a pass are dealt to nt lanes
WavePlan lds_wave_plan(int N, bool groups) {
  const int H = N / 2;
  WavePlan best{};
#define AC_WAVE_CT(NC, NTC, R0, R1, R2, R3)                                \
  if (N == NC && (groups || NTC <= 64)) {                                  \
    best.n = 1 + (R1 > 0) + (R2 > 0) + (R3 > 0);                           \
    best.r[0] = R0, best.r[1] = R1, best.r[2] = R2, best.r[3] = R3;        \
    best.nt = NTC;                                                         \
    return best;                                                           \
  }
  AC_WAVE_CT_SIZES
#undef AC_WAVE_CT
  int nt = 4;
  while (nt < 64 && nt < H / 8) nt <<= 1;
  best.nt = nt;
  static const int cand[] = {10, 9, 8, 6, 5, 4, 3, 2};   // (the super-radices of dct4_wave's run-time form)
  double best_cost = 1e300;
  int cur[6];
  auto cost_of = [&](int n) {
    double c = 0;
    for (int i = 0; i < n; ++i) {
      const int r = cur[i], nb = H / r;
      int lg = 0;
      while ((1 << lg) < r) ++lg;
      c += (double)((nb + nt - 1) / nt) * r * (lg + 3) + 24.0;
    }
    return c;
  };
  // depth-first over non-increasing factor sequences (the largest radix first: its pass has the stride-r writes the padding absorbs)
  struct Rec {
    static void go(int rem, int depth, int maxr, int* cur, const int* cand, double& best_cost, WavePlan& best,
                   const decltype(cost_of)& cost) {
      if (rem == 1) {
        const double c = cost(depth);
        if (c < best_cost) {
          best_cost = c;
          best.n = depth;
          for (int i = 0; i < depth; ++i) best.r[i] = (unsigned char)cur[i];
        }
        return;
      }
      if (depth == 6) return;
      for (int i = 0; i < 8; ++i) {
        const int r = cand[i];
        if (r > maxr || rem % r) continue;
        cur[depth] = r;
        go(rem / r, depth + 1, r, cur, cand, best_cost, best, cost);
      }
    }
  };
  Rec::go(H, 0, 10, cur, cand, best_cost, best, cost_of);
  return best;
}
// waves per workgroup that leave the most waves resident per CU (160 KB of LDS)
static int lds_wave_block(int N, const WavePlan& wp, int extra_floats, size_t* lds_bytes, int ps = AC_PAD_SHIFT) {
  int best_w = 1;
  long best_res = 0;
  for (int w = 1; w <= 4; ++w) {
    const size_t lds = ((size_t)(64 / wp.nt) * w * (wave_floats_per_group(N, ps) + extra_floats) + 3 * N) * sizeof(float);
    const long res = (long)std::min<size_t>(8, 160 * 1024 / std::max<size_t>(lds, 1)) * w;
    if (lds <= 160 * 1024 && res >= best_res) {
      best_res = res;
      best_w = w;
    }
  }
  *lds_bytes = ((size_t)(64 / wp.nt) * best_w * (wave_floats_per_group(N, ps) + extra_floats) + 3 * N) * sizeof(float);   // + the three tables
  return best_w;
}

// the 16-byte kernels serve float32 stereo rows whose lanes cover a frame's sample pairs in four steps
bool lds_wave_vec_ok(const ac_mdct_plan* p, const WavePlan& wp, int C) {
  static const int off = [] { const char* e = getenv("AC_LDS_WAVE_NOVEC"); return e ? atoi(e) : 0; }();   // (A/B measurements)
  return !off && lds_wave_vec_shape(p->N, C, true) && p->d_coefv && p->N / 4 <= kWaveVSteps * wp.nt && !(wp.nt > 64 && wave_ct_off());
}
// which rows a complex pair carries (RowPair): by channel count (the C ABI takes 16-byte aligned tensors; a pointer that is
// not -- an internal caller's -- gets the 4-byte layout)
int wave_v_layout(int C, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* q : ptrs) bits |= reinterpret_cast<uintptr_t>(q);
  if (C == 2 && !(bits & 15)) return 0;
  if (C == 1) return (bits & 7) ? -1 : 1;   // (a mono tensor off the 8-byte grid: the 8-byte kernels of the run-time forms)
  return 2;
}
// waves per workgroup, frames per workgroup and LDS bytes of the 16-byte kernels: the wave form packs frames as lds_wave_block
// says; a frame on more than one wave (in place) is a workgroup of its own with two tables behind its buffer
void wave_v_geometry(int N, const WavePlan& wp, int* w, int* gpw, size_t* lds) {
  const int ps = (lds_wave_ct_size(N) && !wave_ct_off()) ? pad_shift_ct(N) : AC_PAD_SHIFT;   // (as the kernel that will run pads)
  if (wave_in_place(wp.nt)) {
    *w = wp.nt / 64;
    *gpw = 1;
    *lds = ((size_t)group_floats_per_frame(N, ps) + 2 * (size_t)N) * sizeof(float);
  } else {
    *w = lds_wave_block(N, wp, 0, lds, ps);
    *gpw = *w * (64 / wp.nt);
  }
}
// frames per strip of the 16-byte kernels: a strip pays `extra` frames' worth of work before its first frame (the block /
// the transform before it), a launch runs in rounds of as many workgroups as are resident; the least rounds x (frames + extra)
int wave_strip(long long pairs, int per_sig, int gpw, int w, size_t lds, int cus, double extra) {
  static const int forced = [] { const char* e = getenv("AC_LDS_WAVE_STRIP"); return e ? atoi(e) : 0; }();   // (A/B measurements, tests)
  if (forced > 0) return std::min(forced, std::max(per_sig, 1));
  const int t_max = 32;
  const long resident = (long)cus * std::max<long>(1, std::min<long>(160 * 1024 / (long)std::max<size_t>(lds, 1), 8 / w));
  static const int cand[] = {32, 24, 16, 12, 8, 6, 4, 3, 2, 1};
  int best = 1;
  double best_cost = 1e300;
  for (int seg : cand) {
    if (seg > t_max && seg > 1) continue;
    const int len = std::min(seg, per_sig);
    const long long wgs = (pairs * ((per_sig + len - 1) / len) + gpw - 1) / gpw;
    const double rounds = wgs <= 4 * resident ? (double)((wgs + resident - 1) / resident) : (double)wgs / (double)resident;
    const double cost = rounds * (len + extra);
    if (cost < best_cost) {
      best_cost = cost;
      best = len;
    }
  }
  return best;
}


// returned by launch_fwd_wave / launch_inv_wave when the tensors at hand are not for the 16-byte kernels (rows off the 16-byte
// grid, tuning hooks) and the size is past the 8-byte wave kernels' range: the caller goes on to the next tier
constexpr int kWaveDeclined = -12345;
static bool wave_8_byte_range(int N) { return lds_fft_ok(N) && N <= lds_wave_max(); }
template <typename TIO>
static int launch_fwd_wave(const ac_mdct_plan* p, const TIO* x, TIO* X, const TIO* prev_block, int B, int Kin, int F, int C,
                           hipStream_t s) {
  const WavePlan wp0 = lds_wave_plan(p->N);
  if constexpr (std::is_same<TIO, float>::value)
    if (lds_wave_vec_ok(p, wp0, C)) {
      const int lay = wave_v_layout(C, {x, X, prev_block});
      if (lay >= 0) return lay == 0 ? launch_fwd_wave_stereo(p, x, X, prev_block, B, Kin, F, s)
             : lay == 1 ? launch_fwd_wave_mono(p, x, X, prev_block, B, Kin, F, s)
                        : [&] {   // whole cache lines where the shape has a team form, the strided channel pairs elsewhere
                            const int st = launch_fwd_wave_team(p, x, X, prev_block, B, Kin, F, C, s);
                            return st != kTeamDeclined ? st : launch_fwd_wave_strided(p, x, X, prev_block, B, Kin, F, C, s);
                          }();
    }
  if (!wave_8_byte_range(p->N)) return kWaveDeclined;
  const WavePlan wp = lds_wave_plan(p->N, false);
  size_t lds = 0;
  const int w = lds_wave_block(p->N, wp, 0, &lds);
  const int CP = (C + 1) / 2, gpw = w * (64 / wp.nt);
  const long long ntasks = (long long)B * CP * F;
  int T = 4;
  while (T > 1 && ntasks < (long long)gpw * T * p->cus * 4) T >>= 1;
  const int st = allow_lds(k_fwd_wave<TIO>, lds);
  if (st) return st;
  const long long g = (ntasks + (long long)gpw * T - 1) / ((long long)gpw * T);
  const int st2 = check_grid(g);
  if (st2) return st2 < 0 ? st2 : AC_OK;
  hipLaunchKernelGGL(k_fwd_wave<TIO>, dim3((unsigned)g), dim3(64 * w), lds, s, x, X, prev_block, p->d_coef, p->d_ctab, Kin, F, C,
                     CP, p->N, ntasks, T, wp);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}
template <typename TIO>
static int launch_inv_wave(const ac_mdct_plan* p, const TIO* X, TIO* x, const float* tail_in, float* tail_out, int B, int Kp,
                           int nblk, int C, hipStream_t s) {
  const WavePlan wp0 = lds_wave_plan(p->N);
  if constexpr (std::is_same<TIO, float>::value)
    if (lds_wave_vec_ok(p, wp0, C)) {
      const int lay = wave_v_layout(C, {X, x});
      if (lay >= 0) return lay == 0 ? launch_inv_wave_stereo(p, X, x, tail_in, tail_out, B, Kp, nblk, s)
             : lay == 1 ? launch_inv_wave_mono(p, X, x, tail_in, tail_out, B, Kp, nblk, s)
                        : [&] {
                            const int st = launch_inv_wave_team(p, X, x, tail_in, tail_out, B, Kp, nblk, C, s);
                            return st != kTeamDeclined ? st : launch_inv_wave_strided(p, X, x, tail_in, tail_out, B, Kp, nblk, C, s);
                          }();
    }
  if (!wave_8_byte_range(p->N)) return kWaveDeclined;
  const WavePlan wp = lds_wave_plan(p->N, false);
  size_t lds = 0;
  const int w = lds_wave_block(p->N, wp, p->N, &lds);
  const int per_sig = nblk + (tail_out ? 1 : 0);
  const int CP = (C + 1) / 2, gpw = w * (64 / wp.nt);
  // blocks per strip: every strip but a signal's first pays one more transform for the frame before it
  int seg = 8;
  while (seg > 1 && (long long)B * CP * ((per_sig + seg - 1) / seg) < (long long)gpw * p->cus * 4) seg >>= 1;
  const int nseg = (per_sig + seg - 1) / seg;
  const long long ntasks = (long long)B * CP * nseg;
  const int st = allow_lds(k_inv_wave<TIO>, lds);
  if (st) return st;
  const long long g = (ntasks + gpw - 1) / gpw;
  const int st2 = check_grid(g);
  if (st2) return st2 < 0 ? st2 : AC_OK;
  hipLaunchKernelGGL(k_inv_wave<TIO>, dim3((unsigned)g), dim3(64 * w), lds, s, X, x, tail_in, tail_out, p->d_coef, p->d_ctab, Kp,
                     nblk, seg, nseg, C, CP, p->N, ntasks, wp);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

// 16-bit PCM at the boundary on the instances of AC_WAVE_PCM_SIZES (mono / stereo): AC_EUNSUPPORTED elsewhere
static bool wave_pcm_size(int N) {
#define AC_WAVE_CT(NC, NTC, R0, R1, R2, R3) \
  if (N == NC) return true;
  AC_WAVE_PCM_SIZES
#undef AC_WAVE_CT
  return false;
}
bool lds_fft_serves_pcm16(const ac_mdct_plan* p, int C) {
  return !g_force_generic && !wave_ct_off() && p->d_coefv && (C == 1 || C == 2) && wave_pcm_size(p->N);
}
int launch_fwd_lds_pcm16(const ac_mdct_plan* p, const int16_t* x, float* X, int B, int K, int C, hipStream_t s) {
  return C == 2 ? launch_fwd_wave_stereo_pcm16(p, x, X, B, K, K + 1, s) : launch_fwd_wave_mono_pcm16(p, x, X, B, K, K + 1, s);
}
int launch_inv_lds_pcm16(const ac_mdct_plan* p, const float* X, int16_t* x, int B, int Kp, int C, hipStream_t s) {
  return C == 2 ? launch_inv_wave_stereo_pcm16(p, X, x, B, Kp, Kp + 1, s) : launch_inv_wave_mono_pcm16(p, X, x, B, Kp, Kp + 1, s);
}

// which LDS-FFT form serves float32 tensors of C channels at this plan's size: 2 = a compile-time instance of the 16-byte
// kernels, 1 = the run-time forms of the tier, 0 = none (the O(N^2) kernels)
int lds_fft_tier_of(const ac_mdct_plan* p, int C) {
  if (g_force_generic) return 0;
  if (lds_wave_ok(p->N, false, C, true) && lds_wave_vec_ok(p, lds_wave_plan(p->N), C)) return lds_wave_ct_size(p->N) && !wave_ct_off() ? 2 : 1;
  return lds_fft_ok(p->N) ? 1 : 0;
}

// ---- the dispatch below the wave-level kernels, for every storage type TIO the filter bank admits: the 16-byte / 8-byte wave
// kernels, then the workgroup form of the LDS-FFT tier, then the O(N^2) kernels.  The LDS-FFT tier is float32 arithmetic;
// float64 tensors have the O(N^2) kernels only, in fp64 on the fp64 tables.  The streaming state (prev_block; tail_in, tail_out
// in the arithmetic type) may be null.
template <typename TC>
static const TC* coef_of(const ac_mdct_plan* p) {
  if constexpr (std::is_same<TC, double>::value) return p->d_coef64;
  else return p->d_coef;
}
template <typename TC>
static const TC* ctab_of(const ac_mdct_plan* p) {
  if constexpr (std::is_same<TC, double>::value) return p->d_ctab64;
  else return p->d_ctab;
}
// the O(N^2) kernels hold one frame (synthesis: two) of TC in at most 64 KB of LDS
template <typename TC>
static int require_generic_lds(size_t lds, int N) {
  if constexpr (std::is_same<TC, double>::value)
    AC_REQUIRE(lds <= 64 * 1024, "filters_n = %d too large for the float64 kernel", N);
  else
    AC_REQUIRE(lds <= 64 * 1024, "filters_n = %d too large for the generic kernel", N);
  return AC_OK;
}

template <typename TIO>
static int launch_fwd_T(const ac_mdct_plan* p, const TIO* x, TIO* X, const TIO* prev_block, int B, int Kin, int F, int C,
                        hipStream_t s) {
  using TC = typename Compute<TIO>::type;
  const long long nwg = (long long)B * C * F;
  const int st = check_grid(nwg);
  if (st) return st < 0 ? st : AC_OK;
  if constexpr (std::is_same<TC, float>::value) {
    if (lds_wave_ok(p->N, false, C, std::is_same<TIO, float>::value) && !g_force_generic) {
      const int r = launch_fwd_wave<TIO>(p, x, X, prev_block, B, Kin, F, C, s);
      if (r != kWaveDeclined) return r;
    }
    if (lds_fft_ok(p->N) && !g_force_generic) {
      const int CP = (C + 1) / 2, gpw = kThreads / lds_group_threads(p->N);
      const long long ntasks = (long long)B * CP * F;
      const size_t lds2 = ((size_t)gpw * lds_fwd_floats_per_group(p->N) + p->N) * sizeof(float);
      const bool alias = lds_fwd_floats_per_group(p->N) == 4 * p->N;
      const int st2 = alias ? allow_lds(k_fwd_lds<TIO, true>, lds2) : allow_lds(k_fwd_lds<TIO, false>, lds2);
      if (st2) return st2;
      const dim3 grid((unsigned)((ntasks + gpw - 1) / gpw));
      if (alias)
        hipLaunchKernelGGL((k_fwd_lds<TIO, true>), grid, dim3(kThreads), lds2, s, x, X, prev_block, p->d_coef, p->d_ctab, Kin, F,
                           C, CP, p->N, ntasks);
      else
        hipLaunchKernelGGL((k_fwd_lds<TIO, false>), grid, dim3(kThreads), lds2, s, x, X, prev_block, p->d_coef, p->d_ctab, Kin, F,
                           C, CP, p->N, ntasks);
      AC_HIP_CHECK(hipGetLastError());
      return AC_OK;
    }
  }
  const size_t lds = (size_t)p->N * sizeof(TC);
  const int st3 = require_generic_lds<TC>(lds, p->N);
  if (st3) return st3;
  hipLaunchKernelGGL((k_fwd_generic<TIO, TC>), dim3((unsigned)nwg), dim3(kThreads), lds, s, x, X, prev_block, coef_of<TC>(p),
                     ctab_of<TC>(p), Kin, F, C, p->N);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

template <typename TIO, typename TC = typename Compute<TIO>::type>
static int launch_inv_T(const ac_mdct_plan* p, const TIO* X, TIO* x, const TC* tail_in, TC* tail_out, int B, int Kp, int nblk,
                        int C, hipStream_t s) {
  const int per_sig = nblk + (tail_out ? 1 : 0);   // blocks incl. the virtual state block
  const long long nwg = (long long)B * C * per_sig;
  const int st = check_grid(nwg);
  if (st) return st < 0 ? st : AC_OK;
  if constexpr (std::is_same<TC, float>::value) {
    if (lds_wave_ok(p->N, true, C, std::is_same<TIO, float>::value) && !g_force_generic) {
      const int r = launch_inv_wave<TIO>(p, X, x, tail_in, tail_out, B, Kp, nblk, C, s);
      if (r != kWaveDeclined) return r;
    }
    if (lds_fft_ok(p->N) && !g_force_generic) {
      const int seg = 8, CP = (C + 1) / 2, gpw = kThreads / lds_group_threads(p->N);
      const int nseg = (per_sig + seg - 1) / seg;
      const long long ntasks = (long long)B * CP * nseg;
      const size_t lds2 = ((size_t)gpw * 7 * p->N + p->N) * sizeof(float);
      const int st2 = allow_lds(k_inv_lds<TIO>, lds2);
      if (st2) return st2;
      hipLaunchKernelGGL(k_inv_lds<TIO>, dim3((unsigned)((ntasks + gpw - 1) / gpw)), dim3(kThreads), lds2, s, X, x, tail_in,
                         tail_out, p->d_coef, p->d_ctab, Kp, nblk, seg, nseg, C, CP, p->N, ntasks);
      AC_HIP_CHECK(hipGetLastError());
      return AC_OK;
    }
  }
  const size_t lds = 2 * (size_t)p->N * sizeof(TC);
  const int st3 = require_generic_lds<TC>(lds, p->N);
  if (st3) return st3;
  hipLaunchKernelGGL((k_inv_generic<TIO, TC>), dim3((unsigned)nwg), dim3(kThreads), lds, s, X, x, tail_in, tail_out, coef_of<TC>(p),
                     ctab_of<TC>(p), Kp, nblk, per_sig, C, p->N);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

// ---- the entry points of the unit (ac_internal.h): tensors of `dtype`, one of the four the filter bank admits
template <typename F>
static int with_mdct_dtype(int dtype, F&& f) {
  return with_dtype<float, double, f16_t, bf16_t>(dtype, f);
}
int launch_fwd_typed(const ac_mdct_plan* p, const void* x, void* X, const void* prev_block, int dtype, int B, int Kin, int F, int C,
                     hipStream_t s) {
  return with_mdct_dtype(dtype, [&](auto tag) {
    using TIO = typename decltype(tag)::type;
    return launch_fwd_T(p, (const TIO*)x, (TIO*)X, (const TIO*)prev_block, B, Kin, F, C, s);
  });
}
int launch_inv_typed(const ac_mdct_plan* p, const void* X, void* x, const void* tail_in, void* tail_out, int dtype, int B, int Kp,
                     int nblk, int C, hipStream_t s) {
  return with_mdct_dtype(dtype, [&](auto tag) {
    using TIO = typename decltype(tag)::type;
    using TC = typename Compute<TIO>::type;
    return launch_inv_T(p, (const TIO*)X, (TIO*)x, (const TC*)tail_in, (TC*)tail_out, B, Kp, nblk, C, s);
  });
}

}  // namespace ac
