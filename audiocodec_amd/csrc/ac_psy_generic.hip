// The generic masking model and its backward: any filter_bands_n, any channel count, any Bark-band count, in float32, float64
// and on bfloat16 tensors.  They are the path for the plans and dtypes the wave-level kernels (ac_fast_*.hip, ac_psy_mid.hip)
// do not cover and an independent on-device cross-check for them.  One launcher per kernel, templated over the storage type.
// gfx950 only.
#include "ac_generic_dev.h"
#include "ac_lds_fft_dev.h"   // (kThreads, smem_raw)

namespace ac {

// ------------------------------------------------------------------------------------------------
// tonality (psychoacoustic.py:102-120), one workgroup per (b, frame, c)
// ------------------------------------------------------------------------------------------------
template <typename T>
__device__ inline T block_sum(T v, T* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  T s = 0;
  for (int w = 0; w < kThreads / 64; ++w) s += red[w];
  return s;
}
template <typename TIO, typename TC = typename Compute<TIO>::type>
static __global__ __launch_bounds__(kThreads) void k_tonality_generic(const TIO* __restrict__ X, TIO* __restrict__ t,
                                                               int C, int N) {
  __shared__ TC red[kThreads / 64];
  const TC eps = (TC)1e-14;
  const long long wg = blockIdx.x;   // (b*F + f)*C + c
  const int c = (int)(wg % C);
  const long long bf = wg / C;
  const TIO* Xi = X + (size_t)bf * N * C + c;
  TC slog = 0, ssq = 0;
  for (int k = threadIdx.x; k < N; k += kThreads) {
    const TC a = ldv(Xi + (size_t)k * C);
    const TC I = a * a;
    slog += m_log(m_max(eps, I));
    ssq += I;
  }
  slog = block_sum(slog, red);
  ssq = block_sum(ssq, red);
  if (threadIdx.x == 0) {
    const TC gm = m_exp(slog / (TC)N);
    const TC am = ssq / (TC)N + eps;
    const TC sfm = (TC)10 * m_log(gm / am) / (TC)2.302585092994046;
    stv(t + wg, m_min(sfm / (TC)-60, (TC)1));
  }
}

// ------------------------------------------------------------------------------------------------
// global masking threshold (psychoacoustic.py:122-148 with :169-210, :301-331), factorised form
// one workgroup per (b, frame, c)
// ------------------------------------------------------------------------------------------------
template <typename TIO, typename TC = typename Compute<TIO>::type>
static __global__ __launch_bounds__(kThreads) void k_threshold_generic(
    const TIO* __restrict__ X, const TIO* __restrict__ t, TIO* __restrict__ thr, TC drown, TC alpha,
    const int32_t* __restrict__ wb_ptr, const int32_t* __restrict__ wb_idx, const TC* __restrict__ wb_val,
    const int32_t* __restrict__ wi_ptr, const int32_t* __restrict__ wi_idx, const TC* __restrict__ wi_val,
    const TC* __restrict__ S, const TC* __restrict__ quiet, const TC* __restrict__ beta, int C, int N,
    int M) {
  TC* I = reinterpret_cast<TC*>(smem_raw);   // [N]
  TC* Q = I + N;                             // [M]
  TC* G = Q + M;                             // [M]
  const TC eps = (TC)1e-14;
  const long long wg = blockIdx.x;
  const int c = (int)(wg % C);
  const long long bf = wg / C;
  const TIO* Xi = X + (size_t)bf * N * C + c;
  for (int k = threadIdx.x; k < N; k += kThreads) {
    const TC a = ldv(Xi + (size_t)k * C);
    I[k] = a * a;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < M; j += kThreads) {   // _to_bark_intensity (:301-315)
    TC P = 0;
    for (int e = wb_ptr[j]; e < wb_ptr[j + 1]; ++e) P += I[wb_idx[e]] * wb_val[e];
    Q[j] = m_pow(m_max(eps, P), alpha);               // (:206)
  }
  __syncthreads();
  const TC tt = ldv(t + wg);
  for (int j = threadIdx.x; j < M; j += kThreads) {   // _masking_intensity_in_bark (:169-210)
    TC acc = 0;
    for (int i = 0; i < M; ++i) acc += Q[i] * S[(size_t)i * M + j];
    const TC offset = ((TC)1 - drown) * (tt * beta[j] + (TC)9 * tt + (TC)5.5);     // (:185-191)
    const TC fac = m_pow((TC)10, -alpha * offset / (TC)10);                         // (:197)
    const TC T = m_pow(m_max(eps, fac * acc), (TC)1 / alpha);                       // (:208)
    G[j] = m_max(T, quiet[j]);                                                      // (:144)
  }
  __syncthreads();
  TIO* out = thr + (size_t)bf * N * C + c;
  for (int k = threadIdx.x; k < N; k += kThreads) {   // _bark_intensity_to_freq_ampl (:317-331)
    TC acc = 0;
    for (int e = wi_ptr[k]; e < wi_ptr[k + 1]; ++e) acc += G[wi_idx[e]] * wi_val[e];
    stv(out + (size_t)k * C, m_sqrt(m_max(eps, acc)));
  }
}

// ------------------------------------------------------------------------------------------------
// backward passes of the masking model (adjoints of the two kernels above); one workgroup per (b, frame, c)
// ------------------------------------------------------------------------------------------------
// t = min(c' [mean_f ln max(eps, I_f) - ln(mean_f I_f + eps)], 1), c' = (10 / ln 10) / (-60), I_f = X_f^2:
// d t / d X_f = c' (1/N) ([I_f > eps] / I_f - 1 / (mean I + eps)) 2 X_f   where the clamp is inactive
// TIO: the tensors' element type (float, double, bfloat16); TC: the arithmetic and the constant tables (float, double)
template <typename TIO, typename TC = typename Compute<TIO>::type>
static __global__ __launch_bounds__(kThreads) void k_tonality_bwd_generic(const TIO* __restrict__ X,
                                                                   const TIO* __restrict__ gt,
                                                                   TIO* __restrict__ gX, int accumulate, int C,
                                                                   int N) {
  __shared__ TC red[kThreads / 64];
  const TC eps = (TC)1e-14;
  const long long wg = blockIdx.x;   // (b*F + f)*C + c
  const int c = (int)(wg % C);
  const long long bf = wg / C;
  const TIO* Xi = X + (size_t)bf * N * C + c;
  TIO* gi = gX + (size_t)bf * N * C + c;
  TC slog = 0, ssq = 0;
  for (int k = threadIdx.x; k < N; k += kThreads) {
    const TC a = ldv(Xi + (size_t)k * C);
    slog += m_log(a * a > eps ? a * a : eps);
    ssq += a * a;
  }
  slog = block_sum(slog, red);
  ssq = block_sum(ssq, red);
  const TC am = ssq / (TC)N + eps;
  const TC cc = ((TC)10 / (TC)2.302585092994046) / (TC)-60;
  const TC tt = cc * (slog / (TC)N - m_log(am));
  const TC g = (tt < (TC)1) ? (TC)ldv(gt + wg) * cc / (TC)N : (TC)0;
  for (int k = threadIdx.x; k < N; k += kThreads) {
    const TC a = ldv(Xi + (size_t)k * C);
    const TC I = a * a;
    const TC d = g * ((I > eps ? (TC)1 / I : (TC)0) - (TC)1 / am) * (TC)2 * a;
    stv(gi + (size_t)k * C, accumulate ? (TC)ldv(gi + (size_t)k * C) + d : d);
  }
}

// thr_f = sqrt(max(eps, E_f)), E_f = sum_j G_j Winv[j,f], G_j = max(T_j, quiet_j), T_j = max(eps, Y_j)^(1/alpha),
// Y_j = fac_j A_j, A_j = sum_i Q_i S[i,j], Q_i = max(eps, P_i)^alpha, P_i = sum_f X_f^2 W[f,i],
// fac_j = 10^(-alpha O_j / 10), O_j = (1 - drown)(t beta_j + 9 t + 5.5).  The adjoint walks the chain backwards;
// every max() passes the gradient to its active branch.
template <typename TIO, typename TC = typename Compute<TIO>::type>
static __global__ __launch_bounds__(kThreads) void k_threshold_bwd_generic(
    const TIO* __restrict__ X, const TIO* __restrict__ t, const TIO* __restrict__ gthr, TIO* __restrict__ gX,
    TIO* __restrict__ gt, TC drown, TC alpha,
    const int32_t* __restrict__ wb_ptr, const int32_t* __restrict__ wb_idx, const TC* __restrict__ wb_val,
    const int32_t* __restrict__ wi_ptr, const int32_t* __restrict__ wi_idx, const TC* __restrict__ wi_val,
    const int32_t* __restrict__ wf_ptr, const int32_t* __restrict__ wf_idx, const TC* __restrict__ wf_val,
    const int32_t* __restrict__ vb_ptr, const int32_t* __restrict__ vb_idx, const TC* __restrict__ vb_val,
    const TC* __restrict__ S, const TC* __restrict__ quiet, const TC* __restrict__ beta, int C, int N,
    int M, int s_in_lds) {
  TC* smem = reinterpret_cast<TC*>(smem_raw);
  __shared__ TC red[kThreads / 64];
  const TC kEps = (TC)1e-14;
  TC* xs = smem;        // [N] X
  TC* gE = xs + N;      // [N] d L / d E
  TC* P = gE + N;       // [M]
  TC* Q = P + M;        // [M]
  TC* A = Q + M;        // [M]
  TC* G = A + M;        // [M]
  TC* gA = G + M;       // [M]
  TC* gP = gA + M;      // [M]
  TC* part = gP + M;    // [4][M] partial sums of the band x band products
  TC* Ss = part + 4 * M;   // [M][M] spreading matrix (when it fits)
  const long long wg = blockIdx.x;
  const int c = (int)(wg % C);
  const long long bf = wg / C;
  const TIO* Xi = X + (size_t)bf * N * C + c;
  const TIO* gi = gthr + (size_t)bf * N * C + c;
  for (int k = threadIdx.x; k < N; k += kThreads) xs[k] = ldv(Xi + (size_t)k * C);
  if (s_in_lds)
    for (int k = threadIdx.x; k < M * M; k += kThreads) Ss[k] = S[k];
  const TC* Sm = s_in_lds ? Ss : S;
  __syncthreads();
  // the band loops run on four groups of 64 threads: group q takes every fourth term, partial sums meet in LDS
  const int q = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int j0 = 0; j0 < M; j0 += 64) {
    const int j = j0 + l;
    TC p = 0.f;
    if (j < M)
      for (int e = wb_ptr[j] + q; e < wb_ptr[j + 1]; e += 4) p += xs[wb_idx[e]] * xs[wb_idx[e]] * wb_val[e];
    if (j < M) part[q * M + j] = p;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < M; j += kThreads) {
    const TC p = (part[j] + part[M + j]) + (part[2 * M + j] + part[3 * M + j]);
    P[j] = p;
    Q[j] = m_pow(p > kEps ? p : kEps, alpha);
  }
  __syncthreads();
  for (int j0 = 0; j0 < M; j0 += 64) {
    const int j = j0 + l;
    TC acc = 0.f;
    if (j < M)
      for (int i = q; i < M; i += 4) acc += Q[i] * Sm[(size_t)i * M + j];
    if (j < M) part[q * M + j] = acc;
  }
  __syncthreads();
  const TC tt = t[wg];
  for (int j = threadIdx.x; j < M; j += kThreads) {
    const TC acc = (part[j] + part[M + j]) + (part[2 * M + j] + part[3 * M + j]);
    const TC fac = m_pow((TC)10, -alpha * ((TC)1 - drown) * (tt * beta[j] + (TC)9 * tt + (TC)5.5) / (TC)10);
    A[j] = acc;
    {
      const TC Tj = m_pow(fac * acc > kEps ? fac * acc : kEps, (TC)1 / alpha);
      G[j] = Tj > quiet[j] ? Tj : quiet[j];
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < N; k += kThreads) {
    TC E = 0.f;
    for (int e = wi_ptr[k]; e < wi_ptr[k + 1]; ++e) E += G[wi_idx[e]] * wi_val[e];
    gE[k] = (E > kEps) ? (TC)ldv(gi + (size_t)k * C) * (TC)0.5 / m_sqrt(E) : (TC)0;
  }
  __syncthreads();
  for (int j0 = 0; j0 < M; j0 += 64) {
    const int j = j0 + l;
    TC gG = 0.f;
    if (j < M)
      for (int e = vb_ptr[j] + q; e < vb_ptr[j + 1]; e += 4) gG += gE[vb_idx[e]] * vb_val[e];
    if (j < M) part[q * M + j] = gG;
  }
  __syncthreads();
  TC gt_part = 0.f;
  for (int j = threadIdx.x; j < M; j += kThreads) {
    const TC gG = (part[j] + part[M + j]) + (part[2 * M + j] + part[3 * M + j]);
    const TC fac = m_pow((TC)10, -alpha * ((TC)1 - drown) * (tt * beta[j] + (TC)9 * tt + (TC)5.5) / (TC)10);
    const TC Y = fac * A[j];
    const TC T = m_pow(Y > kEps ? Y : kEps, (TC)1 / alpha);
    const TC gT = (T > quiet[j]) ? gG : (TC)0;
    const TC gY = (Y > kEps) ? gT * T / (alpha * Y) : (TC)0;
    gA[j] = gY * fac;
    // d fac / d t = fac (-alpha ln 10 / 10) (1 - drown) (beta_j + 9)
    gt_part += gY * A[j] * fac * (-alpha * (TC)0.2302585092994046) * ((TC)1 - drown) * (beta[j] + (TC)9);
  }
  gt_part = block_sum(gt_part, red);   // (contains the barriers that publish gA)
  if (threadIdx.x == 0) stv(gt + wg, gt_part);
  for (int i0 = 0; i0 < M; i0 += 64) {
    const int i = i0 + l;
    TC gQ = 0.f;
    if (i < M)
      for (int j = q; j < M; j += 4) gQ += Sm[(size_t)i * M + j] * gA[j];
    if (i < M) part[q * M + i] = gQ;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < M; i += kThreads) {
    const TC gQ = (part[i] + part[M + i]) + (part[2 * M + i] + part[3 * M + i]);
    gP[i] = (P[i] > kEps) ? gQ * alpha * Q[i] / P[i] : (TC)0;
  }
  __syncthreads();
  TIO* go = gX + (size_t)bf * N * C + c;
  for (int k = threadIdx.x; k < N; k += kThreads) {
    TC gI = 0.f;
    for (int e = wf_ptr[k]; e < wf_ptr[k + 1]; ++e) gI += gP[wf_idx[e]] * wf_val[e];
    stv(go + (size_t)k * C, (TC)2 * xs[k] * gI);
  }
}

// ------------------------------------------------------------------------------------------------
// launchers: one per kernel, for every storage type TIO the masking model admits
// ------------------------------------------------------------------------------------------------
// the plan's value tables in the arithmetic type TC: the float set (float32 / bfloat16 tensors) or the float64 set
template <typename TC>
struct PsyVals {
  const TC *wb_val, *wi_val, *wf_val, *vb_val, *S, *quiet, *beta;
};
template <typename TC>
static PsyVals<TC> psy_vals(const ac_psy_plan* p) {
  if constexpr (std::is_same<TC, double>::value)
    return {p->d_wb_val64, p->d_wi_val64, p->d_wf_val64, p->d_vb_val64, p->d_S64, p->d_quiet64, p->d_beta64};
  else
    return {p->d_wb_val, p->d_wi_val, p->d_wf_val, p->d_vb_val, p->d_S, p->d_quiet, p->d_beta};
}

template <typename TIO>
static int launch_tonality_T(const ac_psy_plan* p, const TIO* X, TIO* t, int B, int F, int C, hipStream_t s) {
  const long long nwg = (long long)B * F * C;
  const int st = check_grid(nwg);
  if (st) return st < 0 ? st : AC_OK;
  hipLaunchKernelGGL((k_tonality_generic<TIO>), dim3((unsigned)nwg), dim3(kThreads), 0, s, X, t, C, p->N);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

template <typename TIO, typename TC = typename Compute<TIO>::type>
static int launch_threshold_T(const ac_psy_plan* p, const TIO* X, const TIO* t, TC drown, TIO* thr, const PsyVals<TC>& v, int B,
                              int F, int C, hipStream_t s) {
  const long long nwg = (long long)B * F * C;
  const int st = check_grid(nwg);
  if (st) return st < 0 ? st : AC_OK;
  const size_t lds = ((size_t)p->N + 2 * (size_t)p->M) * sizeof(TC);
  if constexpr (std::is_same<TC, double>::value)
    AC_REQUIRE(lds <= 64 * 1024, "filter_bands_n = %d / bark_bands_n = %d too large for the float64 kernel", p->N, p->M);
  else
    AC_REQUIRE(lds <= 64 * 1024, "filter_bands_n = %d / bark_bands_n = %d too large for the generic kernel", p->N, p->M);
  hipLaunchKernelGGL((k_threshold_generic<TIO, TC>), dim3((unsigned)nwg), dim3(kThreads), lds, s, X, t, thr, drown, (TC)p->alpha,
                     p->d_wb_ptr, p->d_wb_idx, v.wb_val, p->d_wi_ptr, p->d_wi_idx, v.wi_val, v.S, v.quiet, v.beta, C, p->N, p->M);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

template <typename TIO>
static int launch_tonality_bwd_T(const ac_psy_plan* p, const TIO* X, const TIO* gt, TIO* gX, int accumulate, int B, int F, int C,
                                 hipStream_t s) {
  const long long nwg = (long long)B * F * C;
  const int st = check_grid(nwg);
  if (st) return st < 0 ? st : AC_OK;
  hipLaunchKernelGGL((k_tonality_bwd_generic<TIO>), dim3((unsigned)nwg), dim3(kThreads), 0, s, X, gt, gX, accumulate, C, p->N);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

template <typename TIO, typename TC = typename Compute<TIO>::type>
static int launch_threshold_bwd_T(const ac_psy_plan* p, const TIO* X, const TIO* t, TC drown, const TIO* gthr, TIO* gX, TIO* gt,
                                  const PsyVals<TC>& v, int B, int F, int C, hipStream_t s) {
  const long long nwg = (long long)B * F * C;
  const int st = check_grid(nwg);
  if (st) return st < 0 ? st : AC_OK;
  size_t lds = (2 * (size_t)p->N + 10 * (size_t)p->M) * sizeof(TC);
  AC_REQUIRE(lds <= 64 * 1024, "filter_bands_n = %d / bark_bands_n = %d too large for the backward kernel", p->N, p->M);
  const size_t with_s = lds + (size_t)p->M * p->M * sizeof(TC);
  const int s_in_lds = with_s <= 64 * 1024;
  if (s_in_lds) lds = with_s;
  hipLaunchKernelGGL((k_threshold_bwd_generic<TIO, TC>), dim3((unsigned)nwg), dim3(kThreads), lds, s, X, t, gthr, gX, gt, drown,
                     (TC)p->alpha, p->d_wb_ptr, p->d_wb_idx, v.wb_val, p->d_wi_ptr, p->d_wi_idx, v.wi_val, p->d_wf_ptr, p->d_wf_idx,
                     v.wf_val, p->d_vb_ptr, p->d_vb_idx, v.vb_val, v.S, v.quiet, v.beta, C, p->N, p->M, s_in_lds);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

// ---- the entry points of the unit (ac_internal.h): tensors of `dtype`, one of the three the masking model admits (there is no
// float16 masking model: psychoacoustic.py:42-43)
template <typename F>
static int with_psy_dtype(int dtype, F&& f) {
  return with_dtype<float, double, bf16_t>(dtype, f);
}
int launch_tonality_typed(const ac_psy_plan* p, const void* X, void* t, int dtype, int B, int F, int C, hipStream_t s) {
  return with_psy_dtype(dtype, [&](auto tag) {
    using TIO = typename decltype(tag)::type;
    return launch_tonality_T(p, (const TIO*)X, (TIO*)t, B, F, C, s);
  });
}
int launch_threshold_typed(const ac_psy_plan* p, const void* X, const void* t, double drown, void* thr, int dtype, int B, int F,
                           int C, hipStream_t s) {
  return with_psy_dtype(dtype, [&](auto tag) {
    using TIO = typename decltype(tag)::type;
    using TC = typename Compute<TIO>::type;
    return launch_threshold_T(p, (const TIO*)X, (const TIO*)t, (TC)drown, (TIO*)thr, psy_vals<TC>(p), B, F, C, s);
  });
}
int launch_tonality_bwd_typed(const ac_psy_plan* p, const void* X, const void* gt, void* gX, int accumulate, int dtype, int B, int F,
                              int C, hipStream_t s) {
  return with_psy_dtype(dtype, [&](auto tag) {
    using TIO = typename decltype(tag)::type;
    return launch_tonality_bwd_T(p, (const TIO*)X, (const TIO*)gt, (TIO*)gX, accumulate, B, F, C, s);
  });
}
int launch_threshold_bwd_typed(const ac_psy_plan* p, const void* X, const void* t, double drown, const void* gthr, void* gX, void* gt,
                               int dtype, int B, int F, int C, hipStream_t s) {
  return with_psy_dtype(dtype, [&](auto tag) {
    using TIO = typename decltype(tag)::type;
    using TC = typename Compute<TIO>::type;
    return launch_threshold_bwd_T(p, (const TIO*)X, (const TIO*)t, (TC)drown, (const TIO*)gthr, (TIO*)gX, (TIO*)gt, psy_vals<TC>(p), B,
                                  F, C, s);
  });
}

}  // namespace ac
