// The masking model of the wave-level kernels for filters_n = 1024 / 2048 (ac_fast_dev.h): its image, the per-lane
// constants and psy_stage(), the epilogue the fused encode (ac_fast_fwd_dev.h) and the stand-alone kernels
// (ac_fast_psy.hip) run on a frame in registers.
#pragma once
#include "ac_fast_dev.h"

namespace ac {
namespace {

// ---- psy image (32-bit words) in ac_psy_plan::d_fast for filter_bands_n = 128 R and 64 Bark bands; the first PL_LDS
// words are copied into LDS once per workgroup, the rest is held in registers.  The spectrum passes through the wave's
// 8 KB intensity image in NH = R / 8 halves of 1024 bins.
template <int R>
struct PsyGeo {
  static constexpr int NH = R / 8;
  static constexpr int PL_HALF = (R == 8) ? 12 : 16;          // gather-list length / 2 (per half of the spectrum)
  static constexpr int FN = 128 * R;
  static constexpr int PL_G = 0;                              // [128]         spreading prototype g
  static constexpr int PL_LST = 128;                          // [NH][PL_HALF][64]  gather lists: two 16-bit LDS byte offsets per word
  static constexpr int PL_LDS = PL_LST + NH * PL_HALF * 64;   // R = 8: 896 words = 3584 bytes
  static constexpr int PL_BAND = PL_LDS;                      // [NH + 1][64] x 4 words: per-lane (= per Bark band) constants
  //   group h < NH: edge offsets of half h (lo | hi << 16), wf, wl, quiet      group NH: beta, rho, u0, u1
  static constexpr int PL_IDX = PL_BAND + (NH + 1) * 256;     // [R / 4][64] x 4 words: byte offsets (lo | hi << 16) of the
  //   threshold entries of the two bins of granule 64 i + lane, word i
  static constexpr int P_TOTAL = PL_IDX + (R / 4) * 256;
  static constexpr int PSY_LDS = PL_LDS * 4;
  // bf16 tiles of the spreading matrix for the MFMA form of the band x band product (spread_mfma): hi table, lo table
  static constexpr int PL_MF = P_TOTAL;
  static constexpr int P_TOTAL_MF = PL_MF + 2 * (MF_TAB_BYTES / 4);
};
// bytes of LDS the MFMA tiles take behind the psy image (SPREAD 0: f32 VALU product, 1: bf16, 2: split bf16)
constexpr int mf_lds(int spread) { return spread * MF_TAB_BYTES; }

// ------------------------------------------------------------------------------------------------------
// psychoacoustic epilogue on one frame (both channels) held in natural order: xq[i] = (X[2q], X[2q+1]) x (c0, c1),
// q = 64 i + lane.  tonality: psychoacoustic.py:102-120; threshold: :122-148 with :169-210 (factorised,
// SURVEY App. A.3) and :301-331 (Bark mapping as per-band ranges / per-bin entry lookups).
// ------------------------------------------------------------------------------------------------------
struct PsyParams {
  const uint32_t* tab;   // ac_psy_plan::d_fast
  float alpha, inv_alpha, drown;
};

// per-lane (= per Bark band) constants and the lane's threshold-entry offsets, held in registers
template <int R>
struct PsyLane {
  v4f bc0[R / 8];   // per half: edge offsets (lo | hi << 16), wf, wl, quiet
  v4f bc1;          // beta, rho, u0, u1
  v4f idx[R / 4];   // byte offsets (lo | hi << 16) of the entries of the two bins of granule 64 i + lane, word i
};
// wave_base = byte offset of the wave's buffer inside the workgroup's LDS object: the packed 16-bit offsets become
// absolute, so unpacking one costs a single and / shift inside the loop
template <int R>
__device__ __forceinline__ PsyLane<R> load_psy_lane(const uint32_t* __restrict__ tab, int lane, uint32_t wave_base) {
  using P = PsyGeo<R>;
  PsyLane<R> c;
  const uint32_t both = wave_base * 0x10001u;
  auto rebase = [both](float f) { return __uint_as_float(__float_as_uint(f) + both); };
#pragma unroll
  for (int h = 0; h < P::NH; ++h) {
    c.bc0[h] = reinterpret_cast<const v4f*>(tab + P::PL_BAND)[h * 64 + lane];
    c.bc0[h].x = rebase(c.bc0[h].x);
  }
  c.bc1 = reinterpret_cast<const v4f*>(tab + P::PL_BAND)[P::NH * 64 + lane];
#pragma unroll
  for (int i = 0; i < R / 4; ++i) {
    const v4f w = reinterpret_cast<const v4f*>(tab + P::PL_IDX)[i * 64 + lane];
    c.idx[i] = v4f{rebase(w.x), rebase(w.y), rebase(w.z), rebase(w.w)};
  }
  return c;
}

// ------------------------------------------------------------------------------------------------------
// Band x band product with the Toeplitz spreading matrix on the matrix cores (BASELINE configs[3]):
//   out_j = sum_i Q_i S[i, j],  S[i, j] = g[64 - i + j]   (psychoacoustic.py:205-207)
// as 16 (MODE 1) or 32 (MODE 2) v_mfma_f32_4x4x4_16b_bf16.  The instruction's 16 blocks are the 16 column tiles of S
// (block b = bands 4 b .. 4 b + 3, so D lands with band j in lane j, the layout the epilogue continues in); step s
// contracts bands 4 s .. 4 s + 3.  The A tile of step s (4 rows x 4 bands) is the same for every block: it sits in the
// four lanes of block s and cbsz = 4 / abid = s broadcast it.  Rows 0, 1 = the two signals of the pair; MODE 1 leaves
// rows 2, 3 zero (plain bf16, ~3 significant digits: the tolerance is stated in the tests); MODE 2 splits Q = hi + lo
// (rows 2, 3 carry the lo parts) and S = hi + lo (a second B table), four partial products in f32 accumulators, ~16
// mantissa bits -- inside the 1e-4 parity bar.  B tile of step s in lane l: g[64 - 4 s - k + l], k = 0..3 = four
// consecutive entries of the reversed prototype; four copies of the table, shifted by one entry each, make the read an
// aligned 8-byte read for every lane (copy l & 3).  The compiler pairs the reads of two steps into ds_read2_b64, which
// the LDS serves in groups of 16 consecutive lanes over 32 banks: the copies sit 288 bytes = 8 banks (mod 32) apart, so
// the four copies a group touches (8 dwords each) fall on disjoint banks.
// mf = LDS copy of the hi table (MF_TAB_BYTES) followed by the lo table.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {   // v_cvt_pk_bf16_f32 (round to nearest even)
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v2f{a, b}, v2b));
}
template <int K>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {   // lane K of every quad to the whole quad
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, K * 0x55, 0xf, 0xf, false);
}
template <int S, int MODE>
struct MfSteps {
  static __device__ __forceinline__ void run(const v4s a, const char* bhi, v4f& d0, v4f& d1) {
    MfSteps<S - 1, MODE>::run(a, bhi, d0, d1);
    const v4s b = *reinterpret_cast<const v4s*>(bhi + 8 * S);
    if (MODE == 2) {
      d0 = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(a, b, d0, 4, S, 0);
      const v4s bl = *reinterpret_cast<const v4s*>(bhi + MF_TAB_BYTES + 8 * S);
      d1 = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(a, bl, d1, 4, S, 0);
    } else if (S & 1) {
      d1 = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(a, b, d1, 4, S, 0);
    } else {
      d0 = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(a, b, d0, 4, S, 0);
    }
  }
};
template <int MODE>
struct MfSteps<-1, MODE> {
  static __device__ __forceinline__ void run(const v4s, const char*, v4f&, v4f&) {}
};
template <int MODE>
__device__ __forceinline__ v2f spread_mfma(v2f Q, const char* mf, int lane) {
  const uint32_t whi = pk_bf16(Q.x, Q.y);
  // quad-local 4 x 4 transpose of 16-bit values: lane 4 s + i gets row i of bands 4 s .. 4 s + 3.  Every lane
  // evaluates all broadcasts before the select (a DPP read needs its source lane active)
  const int i = lane & 3;
  const bool lo_row = i >= 2;
  uint32_t c0 = quad_bcast<0>(whi), c1 = quad_bcast<1>(whi), c2 = quad_bcast<2>(whi), c3 = quad_bcast<3>(whi);
  if (MODE == 2) {
    const float hx = __uint_as_float(whi << 16), hy = __uint_as_float(whi & 0xffff0000u);
    const uint32_t wlo = pk_bf16(Q.x - hx, Q.y - hy);
    const uint32_t l0 = quad_bcast<0>(wlo), l1 = quad_bcast<1>(wlo), l2 = quad_bcast<2>(wlo), l3 = quad_bcast<3>(wlo);
    c0 = lo_row ? l0 : c0, c1 = lo_row ? l1 : c1, c2 = lo_row ? l2 : c2, c3 = lo_row ? l3 : c3;
  } else {
    c0 = lo_row ? 0u : c0, c1 = lo_row ? 0u : c1, c2 = lo_row ? 0u : c2, c3 = lo_row ? 0u : c3;
  }
  const uint32_t sel = (i & 1) ? 0x07060302u : 0x05040100u;   // the signal's half of each word
  const uint2 au = {__builtin_amdgcn_perm(c1, c0, sel), __builtin_amdgcn_perm(c3, c2, sel)};
  const v4s a = __builtin_bit_cast(v4s, au);
  // (kept inside the frame loop: hoisted, the 16 / 32 tiles would pin 32 / 64 registers)
  const uint32_t boff = in_loop((uint32_t)((lane & 3) * MF_COPY_STRIDE + 8 * (16 - (lane >> 2))));
  v4f d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
  MfSteps<15, MODE>::run(a, mf + boff, d0, d1);
  const v4f d = d0 + d1;
  return MODE == 2 ? v2f{d.x + d.z, d.y + d.w} : v2f{d.x, d.y};
}

// buf = the wave's LDS region (WAVE_LDS_PSY bytes), pimg = the workgroup's copy of the psy image
// lds0 = base of the workgroup's LDS object (the absolute offsets of PsyLane count from it)
struct NoEmit {
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void operator()(int, const v4f&) {}
};
template <class E, class = void>
struct emit_pins_products : std::false_type {};
template <class E>
struct emit_pins_products<E, std::void_t<decltype(E::pin_products)>> : std::true_type {};
// EMIT: begin() once the masking model has its per-entry values, then (i, threshold of granule 64 i + lane) as each granule
// of the threshold row comes out of the entry lookup (the kernels with element-wise epilogues consume it there instead of
// holding the whole row)
template <int R, bool WANT_T, bool WANT_THR, int SPREAD = 0, bool T_BF16 = false, class EMIT = NoEmit>
__device__ __forceinline__ void psy_stage(const v4f (&xq)[R], char* lds0, char* buf, const uint32_t* pimg,
                                          const PsyLane<R>& pc, const PsyParams& pp, int lane, v2f& t, v4f (&thr)[R],
                                          EMIT emit = EMIT()) {
  using P = PsyGeo<R>;
  if (WANT_T) {
    v2f slog = {0.f, 0.f}, ssq = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < R; ++i) {
      v4f I = xq[i] * xq[i];
      // the squares stay rounded products: left to -ffp-contract=fast, the compiler fuses one of the two squares of
      // ie + io into the sum -- which one differs between instantiations of this code (fused encode with / without
      // element-wise epilogues, 16-bit PCM input, stand-alone tonality), and with it the last bit of the tonality
      asm("" : "+v"(I));
      const v2f ie = v2f{I.x, I.y}, io = v2f{I.z, I.w};
      ssq += ie + io;
      // ln max(eps, a) + ln max(eps, b) = ln(max(eps, a) max(eps, b)): one v_log per two bins; the product stays
      // in the normal float range for |X| < 1e9 (>= 1e-28)
      slog += log2v(maxv(ie, kEps) * maxv(io, kEps));
    }
    slog.x = wave_sum(slog.x);
    slog.y = wave_sum(slog.y);
    ssq.x = wave_sum(ssq.x);
    ssq.y = wave_sum(ssq.y);
    const v2f am = ssq * (1.0f / P::FN) + kEps;
    // sfm = 10 log10(gm / am) with gm = exp(mean ln I)  ==  10 log10(2) (mean log2 I - log2 am)
    const v2f sfm = 3.0102999566398120f * (slog * (1.0f / P::FN) - log2v(am));
    const v2f tt = sfm * (-1.0f / 60.0f);
    // a frame with a NaN or an infinite intensity has a NaN tonality, as tf.maximum / reduce_mean / tf.minimum make it
    // (psychoacoustic.py:113-118): its sum of squares is not finite (v_max / v_min alone would return the other operand)
    t = v2f{(ssq.x - ssq.x == 0.0f) ? fminf(tt.x, 1.0f) : __builtin_nanf(""), (ssq.y - ssq.y == 0.0f) ? fminf(tt.y, 1.0f) : __builtin_nanf("")};
    if (T_BF16) {   // bfloat16 tensors: the threshold is computed from the tonality the caller gets
      const s2 e = Bf16Fmt::enc2(t.x, t.y);
      t = v2f{Bf16Fmt::dec(e.x), Bf16Fmt::dec(e.y)};
    }
  }
  if (!WANT_THR) return;

  // P_j = sum_f I_f W[f, j]  (:312-313): lane = Bark band; the two edge bins carry weights wf / wl, the interior
  // (weight 1) is gathered as single bins + 8-bin chunk sums through a host-built list of LDS offsets.  The spectrum
  // goes through the 8 KB image in halves of 1024 bins; an edge or list entry outside the half points at the zero slot.
  v2f P0 = {0.f, 0.f}, P1 = {0.f, 0.f};
#pragma unroll
  for (int h = 0; h < P::NH; ++h) {
    wave_sync();
    {
      // intensities in natural order: granule q = (I[2q], I[2q+1]) x (c0, c1) at byte 16 (q ^ ((q >> 4) & 3))
      const int lsw = lane ^ ((lane >> 4) & 3);
#pragma unroll
      for (int i = 0; i < 8; ++i) *reinterpret_cast<v4f*>(buf + 16 * lsw + 1024 * i) = xq[8 * h + i] * xq[8 * h + i];
    }
    wave_sync();
    // sums over aligned chunks of 8 bins (4 granules): lane c owns chunks c and c + 64
    {
      const int x = (lane >> 2) & 3;
      const char* cb = buf + 64 * lane;
      const int o0 = 16 * x, o1 = 16 * (1 ^ x), o2 = 16 * (2 ^ x), o3 = 16 * (3 ^ x);
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2) {
        const char* c2 = cb + 4096 * i2;
        const v4f g0 = *reinterpret_cast<const v4f*>(c2 + o0), g1 = *reinterpret_cast<const v4f*>(c2 + o1),
                  g2 = *reinterpret_cast<const v4f*>(c2 + o2), g3 = *reinterpret_cast<const v4f*>(c2 + o3);
        const v4f s = (g0 + g1) + (g2 + g3);
        *reinterpret_cast<v2f*>(buf + S8_OFF + 8 * lane + 512 * i2) = v2f{s.x + s.z, s.y + s.w};
      }
    }
    wave_sync();
    const v4f bc0 = pc.bc0[h];
    const uint32_t edge = in_loop(__float_as_uint(bc0.x));
    P0 += *reinterpret_cast<const v2f*>(lds0 + (edge & 0xffffu)) * bc0.y;
    P1 += *reinterpret_cast<const v2f*>(lds0 + (edge >> 16)) * bc0.z;
#pragma unroll
    for (int hlf = 0; hlf < P::PL_HALF; ++hlf) {
      const uint32_t w = pimg[P::PL_LST + (h * P::PL_HALF + hlf) * 64 + lane];
      P0 += *reinterpret_cast<const v2f*>(buf + (w & 0xffffu));
      P1 += *reinterpret_cast<const v2f*>(buf + (w >> 16));
    }
  }
  const v2f Pj = P0 + P1;
  v2f Q = exp2v(pp.alpha * log2v(maxv(Pj, kEps)));   // max(eps, P)^alpha  (:206)
  // a band with a NaN intensity stays NaN (tf.maximum): through the band x band product it poisons every band of its frame and
  // signal, as the reference's dense einsum does (:205-207)
  Q = v2f{Pj.x == Pj.x ? Q.x : Pj.x, Pj.y == Pj.y ? Q.y : Pj.y};
  v2f acc;
  if (SPREAD == 0) {
    wave_sync();
    *reinterpret_cast<v2f*>(buf + 8 * lane) = Q;
    wave_sync();
    // sum_i Q_i S[i, j], S[i, j] = g[64 - i + j]  (:205-207 with the offset factor pulled out of the sum)
    v2f acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};
    const float* gp = reinterpret_cast<const float*>(pimg + P::PL_G) + 64 + lane;
#pragma unroll 8
    for (int i = 0; i < 64; i += 2) {
      const v4f qq = *reinterpret_cast<const v4f*>(buf + 8 * i);   // Q_i, Q_{i+1} (broadcast read)
      acc0 += v2f{qq.x, qq.y} * gp[-i];
      acc1 += v2f{qq.z, qq.w} * gp[-i - 1];
    }
    acc = acc0 + acc1;
  } else {
    acc = spread_mfma<SPREAD>(Q, reinterpret_cast<const char*>(pimg) + P::PSY_LDS, lane);
  }
  const v4f bc1 = pc.bc1;
  // t beta + 9 t: the kernels round 9 t and fuse t beta into the sum.  An EMIT that declares pin_products (the quantising
  // encode, whose thresholds must be k_fwd_fast's to the last bit) pins that choice: left to -ffp-contract=fast, its
  // instance rounds t beta and fuses 9 t
  v2f offset;
  if constexpr (emit_pins_products<typename std::remove_reference<EMIT>::type>::value) {
    v2f t9 = 9.0f * t;
    asm("" : "+v"(t9));
    offset = (1.0f - pp.drown) * (t * bc1.x + t9 + 5.5f);
  } else {
    offset = (1.0f - pp.drown) * (t * bc1.x + 9.0f * t + 5.5f);                                // (:185-191)
  }
  const v2f fac = exp2v(offset * (-pp.alpha * 0.33219280948873623f));                          // 10^(-alpha O / 10)
  const v2f T = exp2v(pp.inv_alpha * log2v(maxv(fac * acc, kEps)));                             // (:208)
  v2f G = maxv(T, pc.bc0[0].w);                                                                 // (:144)
  {   // NaN where the reference has NaN: a poisoned product or a NaN tonality (the clamps -- v_max -- would drop it)
    const float px = acc.x + t.x, py = acc.y + t.y;
    G = v2f{px == px ? G.x : px, py == py ? G.y : py};
  }
  v2f Gn;
  Gn.x = __shfl_down(G.x, 1, 64);   // G of band j + 1
  Gn.y = __shfl_down(G.y, 1, 64);
  // thr of the bins of band j: interior bins sqrt(max(eps, G_j rho_j)); the bin shared with band j+1
  // sqrt(max(eps, G_j u0 + G_{j+1} u1))  (:330-331) -- one value per entry, not per bin
  const v2f A0 = maxv(G * bc1.y, kEps), A1 = maxv(G * bc1.z + Gn * bc1.w, kEps);
  wave_sync();
  // v_sqrt_f32 (1 ulp); arguments are >= 1e-14, far from the denormal range
  // (a poisoned frame: every band's G is NaN, and so is every entry)
  *reinterpret_cast<v4f*>(buf + 16 * lane) = v4f{G.x == G.x ? __builtin_amdgcn_sqrtf(A0.x) : G.x, G.y == G.y ? __builtin_amdgcn_sqrtf(A0.y) : G.y,
                                                 G.x == G.x ? __builtin_amdgcn_sqrtf(A1.x) : G.x, G.y == G.y ? __builtin_amdgcn_sqrtf(A1.y) : G.y};   // entry e at byte 8 e
  wave_sync();
  emit.begin();
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const v4f ww = pc.idx[i >> 2];
    const float wf = (i & 3) == 0 ? ww.x : (i & 3) == 1 ? ww.y : (i & 3) == 2 ? ww.z : ww.w;
    const uint32_t w = in_loop(__float_as_uint(wf));
    const v2f a0 = *reinterpret_cast<const v2f*>(lds0 + (w & 0xffffu));
    const v2f a1 = *reinterpret_cast<const v2f*>(lds0 + (w >> 16));
    if constexpr (std::is_same<EMIT, NoEmit>::value) thr[i] = v4f{a0.x, a0.y, a1.x, a1.y};
    else emit(i, v4f{a0.x, a0.y, a1.x, a1.y});
  }
}

// EMIT of the fused encode with AC_EMIT_NOISY (stereo float32 rows)
template <int R>
struct NoisyEmit {
  const v4f* X_row;   // this lane's granules of the spectrum row the wave has just stored
  v4f* thr_row;
  v4f* noisy_row;
  uint64_t i4base, key;
  v4f xr[R];
  __device__ __forceinline__ void begin() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the wave's own stores of X have landed
#pragma unroll
    for (int i = 0; i < R; ++i) xr[i] = X_row[64 * i];
  }
  __device__ __forceinline__ void operator()(int i, const v4f& th_i) {
    __builtin_nontemporal_store(th_i, thr_row + 64 * i);
    float g0, g1, g2, g3;
    const uint64_t i4 = i4base + 64u * i;
    normal_pair(key, 2 * i4, g0, g1);
    normal_pair(key, 2 * i4 + 1, g2, g3);
    __builtin_nontemporal_store(v4f{noisy_of(xr[i].x, th_i.x, g0), noisy_of(xr[i].y, th_i.y, g1), noisy_of(xr[i].z, th_i.z, g2),
                                    noisy_of(xr[i].w, th_i.w, g3)}, noisy_row + 64 * i);
    __builtin_amdgcn_sched_barrier(0);   // one granule at a time: interleaved, the sixteen draws of a row spill registers
  }
};

// (host; here because PsyParams has internal linkage: every object that launches the stage fills its own)
PsyParams psy_params(const ac_psy_plan* p, float drown) {
  PsyParams pp;
  pp.tab = reinterpret_cast<const uint32_t*>(p->d_fast);
  pp.alpha = (float)p->alpha;
  pp.inv_alpha = (float)(1.0 / p->alpha);
  pp.drown = drown;
  return pp;
}

}  // namespace
}  // namespace ac
