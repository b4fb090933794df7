// The 16-byte kernels of the LDS-FFT tier (k_fwd_wave_v / k_inv_wave_v), the table of the sizes with compile-time instances,
// and the launch templates that pick an instance.  Each row layout instantiates them in a translation unit of its own
// (ac_wave_stereo.hip, ac_wave_mono.hip, ac_wave_strided.hip); the team form (ac_wave_team.hip) and the fused encode
// (ac_wave_enc.hip) build on the same pieces.  The host plan and geometry helpers declared here are defined once, with the
// dispatch, in ac_mdct_generic.hip.  gfx950 only.
#pragma once
#include <initializer_list>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

#include "ac_lds_fft_dev.h"

namespace ac {

// ---- the 16-byte kernels of the tier (float32, N % 4 == 0, N <= 16 nt): wide accesses and every PCM block read ONCE.
// A lane owns the sample pairs j = 2 i, 2 i + 1 (i = tid + s nt, s < 4) and their mirrors N - 1 - j.  Block n enters frame n
// through (a1, a2) (second half of the fold) and frame n + 1 through (a3, a4) (first half): with j' = h - 1 - j the second
// is  v[h - 1 - j] = a3[h - 1 - j] x[j] + a4[h - 1 - j] x[N - 1 - j],  i.e. the SAME two samples the lane already holds, so
// it is formed at once and carried in registers to the next frame of the strip.  coefv (ac_mdct_plan::d_coefv) holds the
// coefficients in that order, 16 bytes per lane and step.  The next block's loads are issued before the transform of the
// current frame and land while it runs.
// The two rows a complex pair carries through the transform (LAY): 0 the channels of a stereo signal (one 16-byte access
// per two samples); 1 two mono signals b, b + 1 (8 bytes each; the last pair of an odd batch is half empty); 2 the channels
// c, c + 1 of three or more channels (8-byte accesses on the 4-byte grid; the last pair of an odd count is half empty).  bfloat16 tensors and filters_n % 4 == 2 run the 8-byte kernels (k_fwd_wave / k_inv_wave, ac_mdct_generic.hip).
typedef float v4f_t __attribute__((ext_vector_type(4)));
// instances of the 16-byte kernels that form the lane's LDS offsets per frame from opaque copies instead of holding them, hoisted,
// across the frame loop: ~130 instead of ~200 registers; with every instance in that form, slower at most sizes (+2 ... +13 %, 18
// sizes on the same tensors), faster at these: transform 1152 0.490 -> 0.434 ms, 2160 0.508 -> 0.457, 2304 0.537 -> 0.502;
// inverse 2304 0.501 -> 0.479, 7680 0.603 -> 0.545 (B = 256 stereo)
static inline __host__ __device__ constexpr bool wave_rebase(int N, bool inverse) {
  return inverse ? (N == 2304 || N == 7680) : (N == 1152 || N == 2160 || N == 2304);
}
__device__ __forceinline__ float ola2(float a, float x, float b, float y) { return __builtin_fmaf(a, x, b * y); }   // a x + b y, one rounding order
typedef float v2f_t __attribute__((ext_vector_type(2)));
typedef float v2u_t __attribute__((ext_vector_type(2), aligned(4)));   // two floats on the 4-byte grid
constexpr int kWaveVSteps = 4;
template <int LAY>
struct RowPair {
  bool has1;
  int C;   // (LAY 2) floats between successive samples
  // samples m, m + 1 (m even) of the two rows starting at a (and b): (row0[m], row1[m], row0[m+1], row1[m+1]).  No branch on
  // has1: a conditional load would make the wave wait for it at the join, before the transform it is meant to overlap; a
  // half-empty pair reads its one row twice (pair_geo) and never stores the second.
  __device__ __forceinline__ v4f_t load2(const float* a, const float* b, int m) const {
    if constexpr (LAY == 0) {
      return *reinterpret_cast<const v4f_t*>(a + 2 * m);
    } else if constexpr (LAY == 1) {
      const v2f_t fa = *reinterpret_cast<const v2f_t*>(a + m);
      const v2f_t fb = *reinterpret_cast<const v2f_t*>(b + m);
      return v4f_t{fa.x, fb.x, fa.y, fb.y};
    } else {
      // the pair's two channels are adjacent: one 8-byte access on the 4-byte grid per sample (gfx950 takes multi-dword global
      // accesses at dword alignment); the half-empty last pair of an odd channel count reads (c - 1, c) instead of (c, c + 1)
      int o = m * C - (has1 ? 0 : 1);   // (formed where it is used: hoisted out of the frame loop, the addresses of a lane's accesses spill)
      asm volatile("" : "+v"(o));
      const v2u_t s0 = *reinterpret_cast<const v2u_t*>(a + o), s1 = *reinterpret_cast<const v2u_t*>(a + o + C);
      return v4f_t{has1 ? s0.x : s0.y, s0.y, has1 ? s1.x : s1.y, s1.y};
    }
  }
  // the same rows as 16-bit PCM (x = pcm / 32768 on the way in, to_pcm16(x) on the way out, as the wave-level
  // kernels of ac_fast_dev.h do): 8 / 4 bytes per access
  __device__ __forceinline__ v4f_t load2(const int16_t* a, const int16_t* b, int m) const {
    static_assert(LAY <= 1, "16-bit PCM: stereo or mono rows");
    typedef short s4_t __attribute__((ext_vector_type(4)));
    typedef short s2_t __attribute__((ext_vector_type(2)));
    constexpr float k = 1.0f / 32768.0f;
    if constexpr (LAY == 0) {
      const s4_t q = *reinterpret_cast<const s4_t*>(a + 2 * m);
      return v4f_t{(float)q.x * k, (float)q.y * k, (float)q.z * k, (float)q.w * k};
    } else {
      const s2_t qa = *reinterpret_cast<const s2_t*>(a + m), qb = *reinterpret_cast<const s2_t*>(b + m);
      return v4f_t{(float)qa.x * k, (float)qb.x * k, (float)qa.y * k, (float)qb.y * k};
    }
  }
  __device__ __forceinline__ void store2(int16_t* a, int16_t* b, int m, v4f_t v) const {
    static_assert(LAY <= 1, "16-bit PCM: stereo or mono rows");
    typedef short s4_t __attribute__((ext_vector_type(4)));
    typedef short s2_t __attribute__((ext_vector_type(2)));
    auto enc = [](float f) { return to_pcm16(f); };   // (ac_internal.h: the one definition)
    if constexpr (LAY == 0) {
      __builtin_nontemporal_store(s4_t{enc(v.x), enc(v.y), enc(v.z), enc(v.w)}, reinterpret_cast<s4_t*>(a + 2 * m));
    } else {
      __builtin_nontemporal_store(s2_t{enc(v.x), enc(v.z)}, reinterpret_cast<s2_t*>(a + m));
      if (has1) __builtin_nontemporal_store(s2_t{enc(v.y), enc(v.w)}, reinterpret_cast<s2_t*>(b + m));
    }
  }
  __device__ __forceinline__ void store2(float* a, float* b, int m, v4f_t v) const {
    if constexpr (LAY == 0) {
      __builtin_nontemporal_store(v, reinterpret_cast<v4f_t*>(a + 2 * m));
    } else if constexpr (LAY == 1) {
      __builtin_nontemporal_store(v2f_t{v.x, v.z}, reinterpret_cast<v2f_t*>(a + m));
      if (has1) __builtin_nontemporal_store(v2f_t{v.y, v.w}, reinterpret_cast<v2f_t*>(b + m));
    } else {
      int o = m * C;
      asm volatile("" : "+v"(o));
      float* p0 = a + o;
      if (has1) {
        *reinterpret_cast<v2u_t*>(p0) = v2u_t{v.x, v.y};
        *reinterpret_cast<v2u_t*>(p0 + C) = v2u_t{v.z, v.w};
      } else {
        p0[0] = v.x;
        p0[C] = v.z;
      }
    }
  }
};
// pair p of a tensor [B, blocks_per_signal * N, C]: float offsets of its row(s), floats between successive blocks, the
// first of its two stream state rows ([B * C][N / 2]), and whether its second row exists
struct PairGeo {
  size_t off_a, off_b, block_stride;
  long long row0;
  bool has1;
};
template <int LAY>
__device__ __forceinline__ PairGeo pair_geo(long long p, int N, int B, int C, size_t blocks_per_signal) {
  PairGeo g;
  if constexpr (LAY == 2) {
    const int CP = (C + 1) / 2;
    const long long b0 = p / CP;
    const int c = 2 * (int)(p - b0 * CP);
    g.has1 = c + 1 < C;
    g.block_stride = (size_t)N * C;
    g.off_a = (size_t)b0 * blocks_per_signal * g.block_stride + c;
    g.off_b = g.off_a + (g.has1 ? 1 : 0);
    g.row0 = b0 * C + c;
  } else {
    g.has1 = LAY == 0 || 2 * p + 1 < B;
    g.block_stride = (size_t)N * (LAY == 1 ? 1 : 2);
    g.off_a = (size_t)(LAY == 1 ? 2 * p : p) * blocks_per_signal * g.block_stride;
    g.off_b = g.off_a + (g.has1 ? blocks_per_signal * g.block_stride : 0);   // (LAY 1: the next signal, or the same one again)
    g.row0 = 2 * p;
  }
  return g;
}

template <int NC, int NTC, int R0, int R1, int R2, int R3, int LAY, typename TX = float>   // TX: float, or int16_t = 16-bit PCM in
static __global__ __launch_bounds__((NTC > kThreads ? NTC : kThreads), 2) void k_fwd_wave_v(const TX* __restrict__ x, float* __restrict__ X,
                                                          const float* __restrict__ prev_block, const v4f_t* __restrict__ coefv,
                                                          const float* __restrict__ ctab, int Kin, int F, int N_rt, long long ntasks,
                                                          int T, int nstrip, int B, int C, int adj, WavePlan wp) {
  float* smem = reinterpret_cast<float*>(smem_raw);
  const int N = NC ? NC : N_rt, nt = NC ? NTC : wp.nt, gpw = (int)blockDim.x / nt, grp = threadIdx.x / nt, tid = threadIdx.x - grp * nt;
  constexpr bool GRP = wave_in_place(NTC);   // the frame transformed in place (a frame on several waves: one frame per workgroup of NTC lanes)
  const int ps = NC ? pad_shift_ct(NC) : AC_PAD_SHIFT;
  const int per = GRP ? group_floats_per_frame(N, ps) : wave_floats_per_group(N, ps), h = N >> 1, q = N >> 2;
  float2* tw = reinterpret_cast<float2*>(smem + (size_t)gpw * per);
  for (int k = threadIdx.x; k < h; k += blockDim.x) {
    tw[k] = cis_neg(ctab, 16 * k, N);
    tw[h + k] = cis_neg(ctab, 4 * k, N);
    if constexpr (!GRP) tw[2 * h + k] = cis_neg(ctab, 4 * k + 1, N);
  }
  __syncthreads();
  const WaveTabs tb = {tw, tw + 2 * h, tw + h};   // (the in-place form has no pre-twiddle table)
  const float2 pre0 = cis_neg(ctab, 1, N);        // exp(-i pi / (4 N))
  float* base = smem + (size_t)grp * per;
  float2* v = reinterpret_cast<float2*>(base);
  cpair* Bp = reinterpret_cast<cpair*>(base);
  cpair* Ap = reinterpret_cast<cpair*>(base + 4 * padded_len(h, ps));
  const float scale = (float)(1.0 / ((double)N * 1.4142135623730951));
  const long long wg = (long long)blockIdx.x * gpw + grp;
  if (wg >= ntasks) return;
  // task -> (pair, strip); LAY 2 with several frames per workgroup (adj): the channel pairs of one signal and strip sit in one
  // workgroup, so that the cache lines they share (a pair uses 8 of every 4 C bytes) come through one L1 (six channels,
  // N = 120: 2.2 -> 3.4 TB/s; a frame per workgroup measured slower that way: pairs of a signal then stay far apart)
  int sp;
  long long pr;
  if (LAY == 2 && adj) {
    const int CP = (C + 1) / 2;
    const long long rest = wg / CP;
    sp = (int)(rest % nstrip);
    pr = (rest / nstrip) * CP + (wg - rest * CP);
  } else {
    sp = (int)(wg % nstrip);
    pr = wg / nstrip;
  }
  const PairGeo gx = pair_geo<LAY>(pr, N, B, C, (size_t)Kin), gX = pair_geo<LAY>(pr, N, B, C, (size_t)F),
                gp = pair_geo<LAY>(pr, N, B, C, 1);
  const RowPair<LAY> rp = {gx.has1, C};
  const int n0 = sp * T, n1 = min(n0 + T, F);
  v4f_t d0[kWaveVSteps], d1[kWaveVSteps], cy[kWaveVSteps];
  auto load_block = [&](auto xa, auto xb) {
#pragma unroll
    for (int s = 0; s < kWaveVSteps; ++s) {
      const int i = tid + s * nt;
      if (i < q) {
        d0[s] = rp.load2(xa, xb, 2 * i);           // samples 2 i, 2 i + 1
        d1[s] = rp.load2(xa, xb, N - 2 - 2 * i);   // samples N - 2 - 2 i, N - 1 - 2 i
      }
    }
  };
  // a x + b y with one fixed rounding order (a product, then one fused multiply-add): the carry is formed at two places -- at
  // a strip's start and inside the frame loop -- and a frame must not depend on which one served it (chunked = one-shot, bit
  // for bit); left to the compiler's contraction the two sites may fuse the other product
  auto fold2 = [](float a, float x, float b, float y) { return __builtin_fmaf(a, x, b * y); };
  auto carry_of = [&](int s, int i) {   // (v[h - 2 - 2 i], v[h - 1 - 2 i]) of the NEXT frame
    const v4f_t g = coefv[2 * i + 1];
    return v4f_t{fold2(g.z, d0[s].z, g.w, d1[s].x), fold2(g.z, d0[s].w, g.w, d1[s].y), fold2(g.x, d0[s].x, g.y, d1[s].z),
                 fold2(g.x, d0[s].y, g.y, d1[s].w)};
  };
  {
    const bool have = n0 >= 1 || prev_block != nullptr;
    if (n0 >= 1) load_block(x + gx.off_a + (size_t)(n0 - 1) * gx.block_stride, x + gx.off_b + (size_t)(n0 - 1) * gx.block_stride);
    else if (prev_block) load_block(prev_block + gp.off_a, prev_block + gp.off_b);
#pragma unroll
    for (int s = 0; s < kWaveVSteps; ++s) {
      const int i = tid + s * nt;
      cy[s] = (have && i < q) ? carry_of(s, i) : v4f_t{0.f, 0.f, 0.f, 0.f};
    }
  }
  if (n0 < Kin) load_block(x + gx.off_a + (size_t)n0 * gx.block_stride, x + gx.off_b + (size_t)n0 * gx.block_stride);
  constexpr bool REBASE_W = wave_rebase(NC, false);
  const int tid_outer = tid;
  for (int n = n0; n < n1; ++n) {
    int boff = grp * per, tid_l = tid_outer;   // (see k_enc_wave_v: per-frame offsets from opaque copies)
    if constexpr (REBASE_W) asm volatile("" : "+v"(boff), "+v"(tid_l));
    const int tid = tid_l;
    float* base = smem + boff;
    float2* v = reinterpret_cast<float2*>(base);
    cpair* Bp = reinterpret_cast<cpair*>(base);
    cpair* Ap = reinterpret_cast<cpair*>(base + 4 * padded_len(h, ps));
    const bool has_cur = n < Kin;
#pragma unroll
    for (int s = 0; s < kWaveVSteps; ++s) {
      const int i = tid + s * nt;
      if (i < q) {
        v4f_t hi = {0.f, 0.f, 0.f, 0.f};
        if (has_cur) {
          const v4f_t f = coefv[2 * i];
          hi = v4f_t{fold2(f.x, d0[s].x, f.y, d1[s].z), fold2(f.x, d0[s].y, f.y, d1[s].w), fold2(f.z, d0[s].z, f.w, d1[s].x),
                     fold2(f.z, d0[s].w, f.w, d1[s].y)};
        }
        *reinterpret_cast<v4f_t*>(v + h + 2 * i) = hi;
        *reinterpret_cast<v4f_t*>(v + h - 2 - 2 * i) = cy[s];
        if (has_cur) cy[s] = carry_of(s, i);
      }
    }
    if (n + 1 < n1 && n + 1 < Kin)   // lands during the transform
      load_block(x + gx.off_a + (size_t)(n + 1) * gx.block_stride, x + gx.off_b + (size_t)(n + 1) * gx.block_stride);
    group_sync<NTC>();
    if constexpr (GRP) dct4_group_ct<NC, NTC, R0, R1, R2, R3>(v, Bp, tb, pre0, tid);
    else if constexpr (NC != 0) dct4_wave_ct<NC, NTC, R0, R1, R2, R3>(v, Ap, Bp, tb, tid);
    else dct4_wave(v, Ap, Bp, tb, N, tid, nt, wp);
    float* Xa = X + gX.off_a + (size_t)n * gX.block_stride;
    float* Xb = X + gX.off_b + (size_t)n * gX.block_stride;
#pragma unroll
    for (int s = 0; s < 2 * kWaveVSteps; ++s) {
      const int i = tid + s * nt;
      if (i < h) rp.store2(Xa, Xb, 2 * i, *reinterpret_cast<const v4f_t*>(v + 2 * i) * scale);
    }
    group_sync<NTC>();
  }
}

// the synthesis in the same form: wide spectrum loads (the next frame's issued before the overlap-add of this one), the two
// output samples j, N - 1 - j of a lane's pairs as two wide stores, the aliased half of the previous frame in registers
template <int NC, int NTC, int R0, int R1, int R2, int R3, int LAY, typename TX = float>   // TX: float, or int16_t = 16-bit PCM out
static __global__ __launch_bounds__((NTC > kThreads ? NTC : kThreads), 2) void k_inv_wave_v(const float* __restrict__ X, TX* __restrict__ x,
                                                          const float* __restrict__ tail_in, float* __restrict__ tail_out,
                                                          const v4f_t* __restrict__ coefv, const float* __restrict__ ctab, int Kp,
                                                          int nblk, int seg, int nseg, int N_rt, long long ntasks, int B,
                                                          int C, int adj, WavePlan wp) {
  float* smem = reinterpret_cast<float*>(smem_raw);
  const int N = NC ? NC : N_rt, nt = NC ? NTC : wp.nt, gpw = (int)blockDim.x / nt, grp = threadIdx.x / nt, tid = threadIdx.x - grp * nt;
  constexpr bool GRP = wave_in_place(NTC);
  const int ps = NC ? pad_shift_ct(NC) : AC_PAD_SHIFT;
  const int h = N >> 1, q = N >> 2, per = GRP ? group_floats_per_frame(N, ps) : wave_floats_per_group(N, ps);
  float2* tw = reinterpret_cast<float2*>(smem + (size_t)gpw * per);
  for (int k = threadIdx.x; k < h; k += blockDim.x) {
    tw[k] = cis_neg(ctab, 16 * k, N);
    tw[h + k] = cis_neg(ctab, 4 * k, N);
    if constexpr (!GRP) tw[2 * h + k] = cis_neg(ctab, 4 * k + 1, N);
  }
  __syncthreads();
  const WaveTabs tb = {tw, tw + 2 * h, tw + h};
  const float2 pre0 = cis_neg(ctab, 1, N);
  float* base = smem + (size_t)grp * per;
  float2* v = reinterpret_cast<float2*>(base);
  cpair* Bp = reinterpret_cast<cpair*>(base);
  cpair* Ap = reinterpret_cast<cpair*>(base + 4 * padded_len(h, ps));
  const long long wg = (long long)blockIdx.x * gpw + grp;
  if (wg >= ntasks) return;
  int sgm;
  long long pr;
  if (LAY == 2 && adj) {   // (channel pairs of one signal and strip side by side: see k_fwd_wave_v)
    const int CP = (C + 1) / 2;
    const long long rest = wg / CP;
    sgm = (int)(rest % nseg);
    pr = (rest / nseg) * CP + (wg - rest * CP);
  } else {
    sgm = (int)(wg % nseg);
    pr = wg / nseg;
  }
  const PairGeo gX = pair_geo<LAY>(pr, N, B, C, (size_t)Kp), gx = pair_geo<LAY>(pr, N, B, C, (size_t)nblk);
  const RowPair<LAY> rp = {gx.has1, C};
  const v4f_t* cv = coefv + h;   // the synthesis half of the table
  const float scale = 2.0f * 1.4142135623730951f;
  const int nlast = nblk + (tail_out ? 1 : 0);
  const int n0 = sgm * seg;
  const size_t ts = (size_t)gx.row0 * h;   // stream state rows of the pair: ts, ts + h
  // the aliased half u_{n-1}[h + 2 i], [h + 2 i + 1] of the lane's pairs stays in registers from frame to frame
  v4f_t um[kWaveVSteps];
#pragma unroll
  for (int s = 0; s < kWaveVSteps; ++s) {
    const int i = tid + s * nt;
    um[s] = v4f_t{0.f, 0.f, 0.f, 0.f};
    if (n0 == 0 && tail_in && i < q) {
      um[s].x = tail_in[ts + 2 * i];
      um[s].z = tail_in[ts + 2 * i + 1];
      if (rp.has1) {
        um[s].y = tail_in[ts + h + 2 * i];
        um[s].w = tail_in[ts + h + 2 * i + 1];
      }
    }
  }
  v4f_t r[2 * kWaveVSteps];
  auto frame_ok = [&](int t) { const int n = n0 + t; return t < 0 || (n < Kp && n < nblk); };
  auto load_frame = [&](int t) {
    const float* Xa = X + gX.off_a + (size_t)(n0 + t) * gX.block_stride;
    const float* Xb = X + gX.off_b + (size_t)(n0 + t) * gX.block_stride;
#pragma unroll
    for (int s = 0; s < 2 * kWaveVSteps; ++s) {
      const int i = tid + s * nt;
      if (i < h) r[s] = rp.load2(Xa, Xb, 2 * i);
    }
  };
  const int t0 = n0 >= 1 ? -1 : 0;
  if (frame_ok(t0)) load_frame(t0);
  constexpr bool REBASE_W = wave_rebase(NC, true);
  const int tid_outer = tid;
  for (int t = t0; t < seg; ++t) {
    int boff = grp * per, tid_l = tid_outer;
    if constexpr (REBASE_W) asm volatile("" : "+v"(boff), "+v"(tid_l));
    const int tid = tid_l;
    float* base = smem + boff;
    float2* v = reinterpret_cast<float2*>(base);
    cpair* Bp = reinterpret_cast<cpair*>(base);
    cpair* Ap = reinterpret_cast<cpair*>(base + 4 * padded_len(h, ps));
    const int n = n0 + t;
    if (t >= 0 && n >= nlast) break;
    const bool has_n = frame_ok(t);
#pragma unroll
    for (int s = 0; s < 2 * kWaveVSteps; ++s) {
      const int i = tid + s * nt;
      if (i < h) *reinterpret_cast<v4f_t*>(v + 2 * i) = has_n ? r[s] : v4f_t{0.f, 0.f, 0.f, 0.f};
    }
    {   // the next frame's loads land during the transform and the overlap-add
      const int tn = t + 1;
      if (tn < seg && n0 + tn < nlast && frame_ok(tn)) load_frame(tn);
    }
    group_sync<NTC>();
    if (has_n) {
      if constexpr (GRP) dct4_group_ct<NC, NTC, R0, R1, R2, R3>(v, Bp, tb, pre0, tid);
      else if constexpr (NC != 0) dct4_wave_ct<NC, NTC, R0, R1, R2, R3>(v, Ap, Bp, tb, tid);
      else dct4_wave(v, Ap, Bp, tb, N, tid, nt, wp);
    }
    if (t >= 0) {
      if (n < nblk) {
        TX* xa = x + gx.off_a + (size_t)n * gx.block_stride;
        TX* xb = x + gx.off_b + (size_t)n * gx.block_stride;
#pragma unroll
        for (int s = 0; s < kWaveVSteps; ++s) {
          const int i = tid + s * nt;
          if (i < q) {
            const v4f_t A = *reinterpret_cast<const v4f_t*>(v + h - 2 - 2 * i) * scale;   // u_n[h-2-2i], u_n[h-1-2i]
            const v4f_t Bm = um[s];                                                         // u_{n-1}[h+2i], [h+2i+1]
            const v4f_t c0 = cv[2 * i], c1 = cv[2 * i + 1];   // (s1, s2)(2i), (s1, s2)(2i+1) | (s3, s4)(2i), (s3, s4)(2i+1)
            // (one fixed rounding order, as the analysis kernels' fold2: the team form of this kernel returns the same bits)
            const v4f_t o0 = {ola2(c0.x, A.z, c0.y, Bm.x), ola2(c0.x, A.w, c0.y, Bm.y), ola2(c0.z, A.x, c0.w, Bm.z), ola2(c0.z, A.y, c0.w, Bm.w)};
            const v4f_t o1 = {ola2(c1.z, A.x, c1.w, Bm.z), ola2(c1.z, A.y, c1.w, Bm.w), ola2(c1.x, A.z, c1.y, Bm.x), ola2(c1.x, A.w, c1.y, Bm.y)};
            rp.store2(xa, xb, 2 * i, o0);
            rp.store2(xa, xb, N - 2 - 2 * i, o1);
          }
        }
      } else if (tail_out) {
#pragma unroll
        for (int s = 0; s < kWaveVSteps; ++s) {
          const int i = tid + s * nt;
          if (i < q) {
            tail_out[ts + 2 * i] = um[s].x;
            tail_out[ts + 2 * i + 1] = um[s].z;
            if (rp.has1) {
              tail_out[ts + h + 2 * i] = um[s].y;
              tail_out[ts + h + 2 * i + 1] = um[s].w;
            }
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < kWaveVSteps; ++s) {
      const int i = tid + s * nt;
      if (i < q) um[s] = *reinterpret_cast<const v4f_t*>(v + h + 2 * i) * scale;
    }
    group_sync<NTC>();
  }
}

// ---- host side
// dynamic LDS beyond the default 64 KB cap must be requested once per kernel and device: remembered, so that a launch in a
// streaming chain does not pay a driver call each time
template <typename K>
int allow_lds(K kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return AC_OK;
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> granted;
  int dev = 0;
  AC_HIP_CHECK(hipGetDevice(&dev));
  const std::pair<const void*, int> key(reinterpret_cast<const void*>(kernel), dev);
  std::lock_guard<std::mutex> lock(mu);
  auto it = granted.find(key);
  if (it != granted.end() && it->second >= bytes) return AC_OK;
  AC_HIP_CHECK(hipFuncSetAttribute(key.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  granted[key] = bytes;
  return AC_OK;
}

// Sizes with compile-time instances of the 16-byte kernels: filters_n, lanes per frame, super-radices (every filters_n % 4 == 0
// with a 5-smooth half up to 8192 -- the powers of two as well: the wave-level kernels of ac_fast_*.hip leave them the
// rectangular window and, below 1024, more than two channels; the plan lds_wave_plan's search would pick, with lanes >= N / 16).  Strides, round counts and buffer offsets fold into immediates: 960 runs 0.156 -> 0.103 ms against the run-time form of
// the same kernel.  lds_wave_plan returns these plans, so the launch geometry and the instance agree by construction; any
// other size runs the run-time form.
// Plans re-measured against alternatives on the same tensors (tools/plan_ab.py, B = 256 stereo, transform / inverse ms): 576
// (8,6,6) 0.393 / 0.446 -> (6,8,6) 0.389 / 0.398; 7680 (10,8,8,6) 0.574 / 0.589 -> (8,8,10,6) 0.472 / 0.603; at 800, 1152, 2304,
// 2880 and 6144 four other orders and splits each ran within 2 % of (or behind) the plan listed: what keeps those sizes at
// 3.7 - 4.0 TB/s where 960 runs at 4.4 is not the split (profiles/r4/lds_fft_plan_ab.txt).
#ifndef AC_WAVE_CT_SIZES   // (a build for inspection may bring a shorter list)
#define AC_WAVE_CT_SIZES \
  AC_WAVE_CT(16, 4, 8, 0, 0, 0) \
  AC_WAVE_CT(20, 4, 10, 0, 0, 0) \
  AC_WAVE_CT(24, 4, 4, 3, 0, 0) \
  AC_WAVE_CT(32, 4, 4, 4, 0, 0) \
  AC_WAVE_CT(36, 4, 6, 3, 0, 0) \
  AC_WAVE_CT(40, 4, 5, 4, 0, 0) \
  AC_WAVE_CT(48, 4, 6, 4, 0, 0) \
  AC_WAVE_CT(60, 4, 10, 3, 0, 0) \
  AC_WAVE_CT(72, 8, 9, 4, 0, 0) \
  AC_WAVE_CT(80, 8, 8, 5, 0, 0) \
  AC_WAVE_CT(96, 8, 8, 6, 0, 0) \
  AC_WAVE_CT(100, 8, 10, 5, 0, 0) \
  AC_WAVE_CT(108, 8, 9, 6, 0, 0) \
  AC_WAVE_CT(120, 8, 10, 6, 0, 0) \
  AC_WAVE_CT(144, 16, 9, 8, 0, 0) \
  AC_WAVE_CT(160, 16, 10, 8, 0, 0) \
  AC_WAVE_CT(180, 16, 10, 9, 0, 0) \
  AC_WAVE_CT(192, 16, 8, 6, 2, 0) \
  AC_WAVE_CT(200, 16, 10, 10, 0, 0) \
  AC_WAVE_CT(216, 16, 9, 4, 3, 0) \
  AC_WAVE_CT(240, 16, 8, 5, 3, 0) \
  AC_WAVE_CT(288, 32, 6, 6, 4, 0) \
  AC_WAVE_CT(300, 32, 6, 5, 5, 0) \
  AC_WAVE_CT(320, 32, 8, 5, 4, 0) \
  AC_WAVE_CT(324, 32, 9, 6, 3, 0) \
  AC_WAVE_CT(360, 32, 6, 6, 5, 0) \
  AC_WAVE_CT(384, 32, 8, 6, 4, 0) \
  AC_WAVE_CT(400, 32, 8, 5, 5, 0) \
  AC_WAVE_CT(432, 32, 9, 8, 3, 0) \
  AC_WAVE_CT(480, 32, 10, 8, 3, 0) \
  AC_WAVE_CT(500, 32, 10, 5, 5, 0) \
  AC_WAVE_CT(540, 64, 9, 6, 5, 0) \
  AC_WAVE_CT(576, 64, 6, 8, 6, 0) \
  AC_WAVE_CT(600, 64, 10, 6, 5, 0) \
  AC_WAVE_CT(640, 64, 8, 8, 5, 0) \
  AC_WAVE_CT(648, 64, 9, 6, 6, 0) \
  AC_WAVE_CT(720, 64, 10, 6, 6, 0) \
  AC_WAVE_CT(768, 64, 8, 8, 6, 0) \
  AC_WAVE_CT(800, 64, 10, 8, 5, 0) \
  AC_WAVE_CT(864, 64, 9, 8, 6, 0) \
  AC_WAVE_CT(900, 64, 10, 9, 5, 0) \
  AC_WAVE_CT(960, 64, 10, 8, 6, 0) \
  AC_WAVE_CT(972, 64, 9, 9, 6, 0) \
  AC_WAVE_CT(1000, 64, 10, 10, 5, 0) \
  AC_WAVE_CT(1080, 128, 10, 9, 6, 0) \
  AC_WAVE_CT(1152, 128, 9, 8, 8, 0) \
  AC_WAVE_CT(1200, 128, 10, 10, 6, 0) \
  AC_WAVE_CT(1280, 128, 10, 8, 8, 0) \
  AC_WAVE_CT(1296, 128, 9, 9, 8, 0) \
  AC_WAVE_CT(1440, 128, 10, 9, 8, 0) \
  AC_WAVE_CT(1500, 128, 6, 5, 5, 5) \
  AC_WAVE_CT(1536, 128, 8, 8, 6, 2) \
  AC_WAVE_CT(1600, 128, 10, 10, 8, 0) \
  AC_WAVE_CT(1620, 128, 10, 9, 9, 0) \
  AC_WAVE_CT(1728, 128, 9, 8, 4, 3) \
  AC_WAVE_CT(1800, 128, 10, 10, 9, 0) \
  AC_WAVE_CT(1920, 128, 8, 8, 5, 3) \
  AC_WAVE_CT(1944, 128, 9, 9, 4, 3) \
  AC_WAVE_CT(2000, 128, 10, 10, 10, 0) \
  AC_WAVE_CT(2160, 256, 6, 6, 6, 5) \
  AC_WAVE_CT(2304, 256, 8, 6, 6, 4) \
  AC_WAVE_CT(2400, 256, 8, 6, 5, 5) \
  AC_WAVE_CT(2500, 256, 10, 5, 5, 5) \
  AC_WAVE_CT(2560, 256, 8, 8, 5, 4) \
  AC_WAVE_CT(2592, 256, 6, 6, 6, 6) \
  AC_WAVE_CT(2700, 256, 9, 6, 5, 5) \
  AC_WAVE_CT(2880, 256, 8, 6, 6, 5) \
  AC_WAVE_CT(2916, 256, 9, 9, 6, 3) \
  AC_WAVE_CT(3000, 256, 10, 6, 5, 5) \
  AC_WAVE_CT(3072, 256, 8, 8, 6, 4) \
  AC_WAVE_CT(3200, 256, 8, 8, 5, 5) \
  AC_WAVE_CT(3240, 256, 9, 9, 5, 4) \
  AC_WAVE_CT(3456, 256, 9, 8, 8, 3) \
  AC_WAVE_CT(3600, 256, 9, 8, 5, 5) \
  AC_WAVE_CT(3840, 256, 10, 8, 8, 3) \
  AC_WAVE_CT(3888, 256, 9, 9, 8, 3) \
  AC_WAVE_CT(4000, 256, 10, 8, 5, 5) \
  AC_WAVE_CT(4096, 256, 8, 8, 8, 4) \
  AC_WAVE_CT(4320, 512, 9, 8, 6, 5) \
  AC_WAVE_CT(4500, 512, 10, 9, 5, 5) \
  AC_WAVE_CT(4608, 512, 8, 8, 6, 6) \
  AC_WAVE_CT(4800, 512, 10, 8, 6, 5) \
  AC_WAVE_CT(4860, 512, 9, 9, 6, 5) \
  AC_WAVE_CT(5000, 512, 10, 10, 5, 5) \
  AC_WAVE_CT(5120, 512, 8, 8, 8, 5) \
  AC_WAVE_CT(5184, 512, 9, 8, 6, 6) \
  AC_WAVE_CT(5400, 512, 10, 9, 6, 5) \
  AC_WAVE_CT(5760, 512, 10, 8, 6, 6) \
  AC_WAVE_CT(5832, 512, 9, 9, 6, 6) \
  AC_WAVE_CT(6000, 512, 10, 10, 6, 5) \
  AC_WAVE_CT(6144, 512, 8, 8, 8, 6) \
  AC_WAVE_CT(6400, 512, 10, 8, 8, 5) \
  AC_WAVE_CT(6480, 512, 9, 9, 8, 5) \
  AC_WAVE_CT(6912, 512, 9, 8, 8, 6) \
  AC_WAVE_CT(7200, 512, 10, 9, 8, 5) \
  AC_WAVE_CT(7680, 512, 8, 8, 10, 6) \
  AC_WAVE_CT(7776, 512, 9, 9, 8, 6) \
  AC_WAVE_CT(8000, 512, 10, 10, 8, 5) \
  AC_WAVE_CT(8100, 512, 10, 9, 9, 5) \
  AC_WAVE_CT(8192, 512, 8, 8, 8, 8) \
  AC_WAVE_CT(64, 4, 8, 4, 0, 0) \
  AC_WAVE_CT(128, 8, 8, 8, 0, 0) \
  AC_WAVE_CT(256, 16, 8, 8, 2, 0) \
  AC_WAVE_CT(512, 32, 8, 8, 4, 0) \
  AC_WAVE_CT(1024, 64, 8, 8, 8, 0) \
  AC_WAVE_CT(2048, 128, 8, 8, 8, 2)
#endif

// defined in ac_mdct_generic.hip, with the dispatch
bool lds_wave_ct_size(int N);   // a size of AC_WAVE_CT_SIZES
bool wave_ct_off();             // AC_LDS_WAVE_NOCT: the compile-time instances off (A/B measurements)
WavePlan lds_wave_plan(int N, bool groups = true);   // groups: frames dealt to more than one wave allowed (the 16-byte kernels)
bool lds_wave_vec_ok(const ac_mdct_plan* p, const WavePlan& wp, int C);   // the 16-byte kernels serve this plan
int wave_v_layout(int C, std::initializer_list<const void*> ptrs);        // LAY of RowPair for these tensors, -1: none
void wave_v_geometry(int N, const WavePlan& wp, int* w, int* gpw, size_t* lds);
int wave_strip(long long pairs, int per_sig, int gpw, int w, size_t lds, int cus, double extra);

// sizes with instances on 16-bit PCM rows (stereo / mono): the frame lengths of the speech and music codecs this tier is for
#define AC_WAVE_PCM_SIZES             \
  AC_WAVE_CT(120, 8, 10, 6, 0, 0)    \
  AC_WAVE_CT(240, 16, 8, 5, 3, 0)    \
  AC_WAVE_CT(480, 32, 10, 8, 3, 0)   \
  AC_WAVE_CT(960, 64, 10, 8, 6, 0)   \
  AC_WAVE_CT(1920, 128, 8, 8, 5, 3)  \
  AC_WAVE_CT(576, 64, 6, 8, 6, 0)    \
  AC_WAVE_CT(1152, 128, 9, 8, 8, 0)
template <int LAY, typename TX = float>
static int launch_fwd_wave_v(const ac_mdct_plan* p, const TX* x, float* X, const float* prev_block, int B, int Kin, int F,
                             int C, hipStream_t s) {
  constexpr bool PCM = !std::is_same<TX, float>::value;
  const WavePlan wp = lds_wave_plan(p->N);
  size_t lds = 0;
  int w = 1, gpw = 1;
  wave_v_geometry(p->N, wp, &w, &gpw, &lds);
  const long long pairs = LAY == 0 ? (long long)B : LAY == 1 ? ((long long)B + 1) / 2 : (long long)B * ((C + 1) / 2);
  const int adj = LAY == 2 && gpw >= (C + 1) / 2;   // (see the kernel: channel pairs of a signal in one workgroup)
  const int T = wave_strip(pairs, F, gpw, w, lds, p->cus, 0.25);   // (every strip reads one block more than it has frames)
  const int nstrip = (F + T - 1) / T;
  const long long ntasks = pairs * nstrip;
  const long long g = (ntasks + gpw - 1) / gpw;
  const int st2 = check_grid(g);
  if (st2) return st2 < 0 ? st2 : AC_OK;
  int st = AC_OK;
  bool done = false;
  if constexpr (PCM) {
#define AC_WAVE_CT(NC, NTC, R0, R1, R2, R3)                                                                                   \
  if (!done && p->N == NC) {                                                                                                   \
    done = true;                                                                                                               \
    st = allow_lds(k_fwd_wave_v<NC, NTC, R0, R1, R2, R3, LAY, TX>, lds);                                                       \
    if (!st)                                                                                                                   \
      hipLaunchKernelGGL((k_fwd_wave_v<NC, NTC, R0, R1, R2, R3, LAY, TX>), dim3((unsigned)g), dim3(64 * w), lds, s, x, X,      \
                         prev_block, reinterpret_cast<const v4f_t*>(p->d_coefv), p->d_ctab, Kin, F, p->N, ntasks, T, nstrip,   \
                         B, C, adj, wp);                                                                                       \
  }
    AC_WAVE_PCM_SIZES
#undef AC_WAVE_CT
    if (!done) return AC_EUNSUPPORTED;
    if (st) return st;
    AC_HIP_CHECK(hipGetLastError());
    return AC_OK;
  } else {
#define AC_WAVE_CT(NC, NTC, R0, R1, R2, R3)                                                                                   \
  if (!done && p->N == NC && !wave_ct_off()) {                                                                                 \
    done = true;                                                                                                               \
    st = allow_lds(k_fwd_wave_v<NC, NTC, R0, R1, R2, R3, LAY>, lds);                                                          \
    if (!st)                                                                                                                   \
      hipLaunchKernelGGL((k_fwd_wave_v<NC, NTC, R0, R1, R2, R3, LAY>), dim3((unsigned)g), dim3(64 * w), lds, s, x, X,         \
                         prev_block, reinterpret_cast<const v4f_t*>(p->d_coefv), p->d_ctab, Kin, F, p->N, ntasks, T, nstrip,   \
                         B, C, adj, wp);                                                                                       \
  }
  AC_WAVE_CT_SIZES
#undef AC_WAVE_CT
  if (!done) {
    st = allow_lds(k_fwd_wave_v<0, 0, 0, 0, 0, 0, LAY>, lds);
    if (!st)
      hipLaunchKernelGGL((k_fwd_wave_v<0, 0, 0, 0, 0, 0, LAY>), dim3((unsigned)g), dim3(64 * w), lds, s, x, X, prev_block,
                         reinterpret_cast<const v4f_t*>(p->d_coefv), p->d_ctab, Kin, F, p->N, ntasks, T, nstrip, B, C, adj, wp);
  }
  if (st) return st;
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
  }
}
template <int LAY, typename TX = float>
static int launch_inv_wave_v(const ac_mdct_plan* p, const float* X, TX* x, const float* tail_in, float* tail_out, int B,
                             int Kp, int nblk, int C, hipStream_t s) {
  constexpr bool PCM = !std::is_same<TX, float>::value;
  const WavePlan wp = lds_wave_plan(p->N);
  size_t lds = 0;
  int w = 1, gpw = 1;
  wave_v_geometry(p->N, wp, &w, &gpw, &lds);
  const int per_sig = nblk + (tail_out ? 1 : 0);
  const long long pairs = LAY == 0 ? (long long)B : LAY == 1 ? ((long long)B + 1) / 2 : (long long)B * ((C + 1) / 2);
  const int adj = LAY == 2 && gpw >= (C + 1) / 2;
  const int seg = wave_strip(pairs, per_sig, gpw, w, lds, p->cus, 1.0);   // (every strip but a signal's first transforms one frame more)
  const int nseg = (per_sig + seg - 1) / seg;
  const long long ntasks = pairs * nseg;
  const long long g = (ntasks + gpw - 1) / gpw;
  const int st2 = check_grid(g);
  if (st2) return st2 < 0 ? st2 : AC_OK;
  int st = AC_OK;
  bool done = false;
  if constexpr (PCM) {
#define AC_WAVE_CT(NC, NTC, R0, R1, R2, R3)                                                                                   \
  if (!done && p->N == NC) {                                                                                                   \
    done = true;                                                                                                               \
    st = allow_lds(k_inv_wave_v<NC, NTC, R0, R1, R2, R3, LAY, TX>, lds);                                                       \
    if (!st)                                                                                                                   \
      hipLaunchKernelGGL((k_inv_wave_v<NC, NTC, R0, R1, R2, R3, LAY, TX>), dim3((unsigned)g), dim3(64 * w), lds, s, X, x,      \
                         tail_in, tail_out, reinterpret_cast<const v4f_t*>(p->d_coefv), p->d_ctab, Kp, nblk, seg, nseg, p->N,  \
                         ntasks, B, C, adj, wp);                                                                               \
  }
    AC_WAVE_PCM_SIZES
#undef AC_WAVE_CT
    if (!done) return AC_EUNSUPPORTED;
    if (st) return st;
    AC_HIP_CHECK(hipGetLastError());
    return AC_OK;
  } else {
#define AC_WAVE_CT(NC, NTC, R0, R1, R2, R3)                                                                                   \
  if (!done && p->N == NC && !wave_ct_off()) {                                                                                 \
    done = true;                                                                                                               \
    st = allow_lds(k_inv_wave_v<NC, NTC, R0, R1, R2, R3, LAY>, lds);                                                          \
    if (!st)                                                                                                                   \
      hipLaunchKernelGGL((k_inv_wave_v<NC, NTC, R0, R1, R2, R3, LAY>), dim3((unsigned)g), dim3(64 * w), lds, s, X, x,         \
                         tail_in, tail_out, reinterpret_cast<const v4f_t*>(p->d_coefv), p->d_ctab, Kp, nblk, seg, nseg, p->N,  \
                         ntasks, B, C, adj, wp);                                                                               \
  }
  AC_WAVE_CT_SIZES
#undef AC_WAVE_CT
  if (!done) {
    st = allow_lds(k_inv_wave_v<0, 0, 0, 0, 0, 0, LAY>, lds);
    if (!st)
      hipLaunchKernelGGL((k_inv_wave_v<0, 0, 0, 0, 0, 0, LAY>), dim3((unsigned)g), dim3(64 * w), lds, s, X, x, tail_in, tail_out,
                         reinterpret_cast<const v4f_t*>(p->d_coefv), p->d_ctab, Kp, nblk, seg, nseg, p->N, ntasks, B, C, adj, wp);
  }
  if (st) return st;
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
  }
}

}  // namespace ac
