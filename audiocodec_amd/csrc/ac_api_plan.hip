// C ABI, plans: create / adjoint / with_row_budget / destroy of the two plan objects, and what a plan says about itself.
#include <cmath>
#include <cstdlib>

#include "ac_api_internal.h"

namespace ac {

// Creation calls upload tables and zero state with the synchronous runtime calls.  Those go to the null stream, a queue that
// nothing orders with a caller's non-blocking streams, and a hipMemset of device memory is allowed to return before the
// device has run it (as CUDA's is).  The plan builders and ac_stream_create end with this wait, so that what they enqueued
// is in place before any first use on any stream; creation may block the host.
hipError_t creation_sync() { return hipStreamSynchronize(nullptr); }
int creation_done() {
  AC_HIP_CHECK(creation_sync());
  return AC_OK;
}

static int check_device(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    set_error("no HIP device available");
    return AC_ENODEV;
  }
  if (device < 0 || device >= count) {
    set_error("device %d out of range (have %d)", device, count);
    return AC_EINVAL;
  }
  return AC_OK;
}

static int compute_units(int device) {   // 256 where the runtime does not say
  int cus = 0;
  return hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0 ? cus : 256;
}

}  // namespace ac

using namespace ac;

extern "C" {

// ---- plans --------------------------------------------------------------------------------------

int ac_mdct_plan_create(int N, int window, int device, ac_mdct_plan** out) {
  return ac_mdct_plan_create_pre(N, window, AC_F64, device, out);
}

static int mdct_plan_build(int N, int window, int precompute, const FoldCoef& c, int adjoint, int device, ac_mdct_plan** out) {
  int st = check_device(device);
  if (st) return st;
  DeviceGuard guard(device);
  ac_mdct_plan* p = new_or_error<ac_mdct_plan>();
  if (!p) return AC_ENOMEM;
  p->N = N;
  p->window = window;
  p->device = device;
  p->pre = precompute;
  p->adjoint = adjoint;
  p->coef = c;
  p->cus = compute_units(device);
  const int h = N / 2;
  std::vector<float> coef(8 * (size_t)h);
  const std::vector<double>* v[8] = {&c.a1, &c.a2, &c.a3, &c.a4, &c.s1, &c.s2, &c.s3, &c.s4};
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < h; ++j) coef[(size_t)i * h + j] = (float)(*v[i])[j];
  std::vector<float> ctab(8 * (size_t)N);
  for (size_t i = 0; i < ctab.size(); ++i) ctab[i] = (float)std::cos(3.14159265358979323846 * (double)i / (4.0 * N));
  std::vector<double> coef64(8 * (size_t)h), ctab64(8 * (size_t)N);
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < h; ++j) coef64[(size_t)i * h + j] = (*v[i])[j];
  for (size_t i = 0; i < ctab64.size(); ++i) ctab64[i] = std::cos(3.14159265358979323846 * (double)i / (4.0 * N));
  st = p->tables.upload(coef, &p->d_coef);
  if (!st && N % 4 == 0) {
    // per pair of samples (2 i, 2 i + 1), i < N / 4: analysis (a1, a2)(2i), (a1, a2)(2i+1) | (a3, a4)(h-1-2i), (a3, a4)(h-2-2i);
    // synthesis (behind the N / 2 analysis entries) (s1, s2)(2i), (s1, s2)(2i+1) | (s3, s4)(2i), (s3, s4)(2i+1)
    std::vector<float> cv(8 * (size_t)h);
    for (int i = 0; i < h / 2; ++i) {
      float* f = &cv[8 * (size_t)i];
      float* g = &cv[4 * (size_t)h + 8 * (size_t)i];
      const int j = 2 * i, m = h - 1 - 2 * i;
      f[0] = (float)c.a1[j], f[1] = (float)c.a2[j], f[2] = (float)c.a1[j + 1], f[3] = (float)c.a2[j + 1];
      f[4] = (float)c.a3[m], f[5] = (float)c.a4[m], f[6] = (float)c.a3[m - 1], f[7] = (float)c.a4[m - 1];
      g[0] = (float)c.s1[j], g[1] = (float)c.s2[j], g[2] = (float)c.s1[j + 1], g[3] = (float)c.s2[j + 1];
      g[4] = (float)c.s3[j], g[5] = (float)c.s4[j], g[6] = (float)c.s3[j + 1], g[7] = (float)c.s4[j + 1];
    }
    st = p->tables.upload(cv, &p->d_coefv);
  }
  if (!st) st = p->tables.upload(ctab, &p->d_ctab);
  if (!st) st = p->tables.upload(coef64, &p->d_coef64);
  if (!st) st = p->tables.upload(ctab64, &p->d_ctab64);
  if (!st && fast_mdct_supported(N, c)) {
    st = fast_mdct_plan_init(p);
    if (!st) p->fast = 1;
  }
  if (!st) st = creation_done();
  if (st) {
    ac_mdct_plan_destroy(p);
    return st;
  }
  *out = p;
  return AC_OK;
}

int ac_mdct_plan_create_pre(int N, int window, int precompute, int device, ac_mdct_plan** out) {
  AC_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  AC_REQUIRE_PRE(precompute);
  AC_REQUIRE(N >= 2 && (N % 2) == 0, "number of filters used in mdct transformation needs to be even (got %d)", N);
  AC_REQUIRE(N <= 8192, "filters_n = %d not supported (max 8192)", N);
  AC_REQUIRE(valid_window(window), "unknown window id %d", window);
  FoldCoef c;
  fold_coefficients(N, window, c, precompute);
  return mdct_plan_build(N, window, precompute, c, 0, device, out);
}

// The transposed filter bank of `plan` as a plan of its own: with T = the analysis bank (x -> X) and S = the synthesis bank
// (X -> x) of `plan`,  ac_mdct_inverse(adjoint, g)[:, N:-N] = 4 N T^T g   and   ac_mdct_forward(adjoint, g)[:, 1:-1] = S^T g / (4 N).
// The DCT-IV is symmetric, so only the O(N) fold transposes: block m of T^T g takes the second half of frame m through
// (a1, a2) and the first half of frame m + 1 through (a3, a4) -- the synthesis form with s1' = reverse(a3), s2' = a1,
// s3' = reverse(a4), s4' = a2; likewise a1' = s2, a2' = s4, a3' = reverse(s1), a4' = reverse(s3).  For Princen-Bradley
// windows computed in float64 the adjoint equals the plan itself (F^-1 = F^T); for the rectangular window
// (mdctransformer.py:209-229) and float32-precomputed ones it does not, and the backward passes need it.
int ac_mdct_plan_adjoint(const ac_mdct_plan* plan, ac_mdct_plan** out) {
  AC_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  AC_REQUIRE(plan != nullptr, "plan is NULL");
  const FoldCoef& c = plan->coef;
  FoldCoef t;
  t.a1 = c.s2;
  t.a2 = c.s4;
  t.a3.assign(c.s1.rbegin(), c.s1.rend());
  t.a4.assign(c.s3.rbegin(), c.s3.rend());
  t.s1.assign(c.a3.rbegin(), c.a3.rend());
  t.s2 = c.a1;
  t.s3.assign(c.a4.rbegin(), c.a4.rend());
  t.s4 = c.a2;
  return mdct_plan_build(plan->N, plan->window, plan->pre, t, plan->adjoint ? 0 : 1, plan->device, out);
}

int ac_mdct_plan_destroy(ac_mdct_plan* p) {
  if (!p) return AC_OK;
  DeviceGuard guard(p->device);
  p->tables.release();
  delete p;
  return AC_OK;
}

static int default_spreading() {
  // The spreading product of a plan created without an explicit choice: the split-bfloat16 matrix-core form where the
  // wave-level kernels serve the plan (measured 2 % faster on the fused encode, thresholds within 1e-5 of the float32
  // form), the float32 form everywhere else.  AC_SPREAD (0 / 1 / 2) overrides: tuning hook, read once.
  static const int dflt = [] {
    const char* e = getenv("AC_SPREAD");
    const int v = e ? atoi(e) : AC_SPREAD_BF16X2_MFMA;
    return v >= 0 && v <= 2 ? v : AC_SPREAD_BF16X2_MFMA;
  }();
  return dflt;
}

int ac_psy_plan_create(int N, int M, double sample_rate, double alpha, int device, ac_psy_plan** out) {
  return ac_psy_plan_create_pre(N, M, sample_rate, alpha, device, -1, AC_F64, out);
}

int ac_psy_plan_create_ex(int N, int M, double sample_rate, double alpha, int device, int spreading, ac_psy_plan** out) {
  AC_REQUIRE(spreading >= AC_SPREAD_F32 && spreading <= AC_SPREAD_BF16X2_MFMA, "spreading = %d is not one of AC_SPREAD_*", spreading);
  return ac_psy_plan_create_pre(N, M, sample_rate, alpha, device, spreading, AC_F64, out);
}

static int psy_plan_build(int N, int M, double sample_rate, double alpha, int device, int spreading, int precompute,
                          ac_psy_plan** out);

int ac_psy_plan_create_pre(int N, int M, double sample_rate, double alpha, int device, int spreading, int precompute,
                           ac_psy_plan** out) {
  AC_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  AC_REQUIRE_PRE(precompute);
  AC_REQUIRE(spreading >= -1 && spreading <= AC_SPREAD_BF16X2_MFMA, "spreading = %d is not one of AC_SPREAD_* (or -1: default)", spreading);
  if (spreading >= 0) return psy_plan_build(N, M, sample_rate, alpha, device, spreading, precompute, out);
  const int dflt = default_spreading();
  int st = psy_plan_build(N, M, sample_rate, alpha, device, dflt, precompute, out);
  if (st == AC_EUNSUPPORTED && dflt != 0) st = psy_plan_build(N, M, sample_rate, alpha, device, 0, precompute, out);
  return st;
}

static int psy_plan_build(int N, int M, double sample_rate, double alpha, int device, int spreading, int precompute,
                          ac_psy_plan** out) {
  AC_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  AC_REQUIRE(spreading >= AC_SPREAD_F32 && spreading <= AC_SPREAD_BF16X2_MFMA, "spreading = %d is not one of AC_SPREAD_*", spreading);
  AC_REQUIRE(N >= 1 && M >= 1, "filter_bands_n (%d) and bark_bands_n (%d) must be positive", N, M);
  AC_REQUIRE(N <= 8192 && M <= 4096, "filter_bands_n = %d / bark_bands_n = %d not supported", N, M);
  AC_REQUIRE(sample_rate > 0 && alpha > 0, "sample_rate and alpha must be positive");
  int st = check_device(device);
  if (st) return st;
  DeviceGuard guard(device);
  ac_psy_plan* p = new_or_error<ac_psy_plan>();
  if (!p) return AC_ENOMEM;
  p->N = N;
  p->M = M;
  p->device = device;
  p->sample_rate = sample_rate;
  p->alpha = alpha;
  p->pre = precompute;
  p->cus = compute_units(device);
  psy_tables(N, M, sample_rate, alpha, p->host, precompute);
  SparseRows wb, wi, wf, vb;
  w_by_band(p->host, wb);
  winv_by_bin(p->host, wi);
  w_by_bin(p->host, wf);
  winv_by_band(p->host, vb);
  p->wb_max = wb.max_row;
  p->wi_max = wi.max_row;
  std::vector<float> S(p->host.S.size()), quiet(M);
  for (size_t i = 0; i < S.size(); ++i) S[i] = (float)p->host.S[i];
  for (int j = 0; j < M; ++j) quiet[j] = (float)p->host.quiet[j];
  st = p->tables.upload(wb.ptr, &p->d_wb_ptr);
  if (!st) st = p->tables.upload(wb.idx, &p->d_wb_idx);
  if (!st) st = p->tables.upload(wb.val, &p->d_wb_val);
  if (!st) st = p->tables.upload(wi.ptr, &p->d_wi_ptr);
  if (!st) st = p->tables.upload(wi.idx, &p->d_wi_idx);
  if (!st) st = p->tables.upload(wi.val, &p->d_wi_val);
  if (!st) st = p->tables.upload(wf.ptr, &p->d_wf_ptr);
  if (!st) st = p->tables.upload(wf.idx, &p->d_wf_idx);
  if (!st) st = p->tables.upload(wf.val, &p->d_wf_val);
  if (!st) st = p->tables.upload(vb.ptr, &p->d_vb_ptr);
  if (!st) st = p->tables.upload(vb.idx, &p->d_vb_idx);
  if (!st) st = p->tables.upload(vb.val, &p->d_vb_val);
  if (!st) st = p->tables.upload(S, &p->d_S);
  if (!st) st = p->tables.upload(quiet, &p->d_quiet);
  if (!st) st = p->tables.upload(p->host.beta, &p->d_beta);
  {
    // the same constants in float64 (AC_F64 entry points): W / W_inv entries in CSR order, S, quiet, and the offset
    // grid linspace(0, max_bark, M) evaluated in float64 (psychoacoustic.py:187-189 with compute_dtype = float64)
    std::vector<double> wbv(wb.idx.size()), wiv(wi.idx.size()), wfv(wf.idx.size()), vbv(vb.idx.size()), beta64(M);
    for (int j = 0; j < M; ++j)
      for (int e = wb.ptr[j]; e < wb.ptr[j + 1]; ++e) wbv[e] = p->host.W[(size_t)wb.idx[e] * M + j];
    for (int f = 0; f < N; ++f)
      for (int e = wi.ptr[f]; e < wi.ptr[f + 1]; ++e) wiv[e] = p->host.W_inv[(size_t)wi.idx[e] * N + f];
    for (int f = 0; f < N; ++f)   // the transposed walks (backward passes): W by bin, W_inv by band
      for (int e = wf.ptr[f]; e < wf.ptr[f + 1]; ++e) wfv[e] = p->host.W[(size_t)f * M + wf.idx[e]];
    for (int j = 0; j < M; ++j)
      for (int e = vb.ptr[j]; e < vb.ptr[j + 1]; ++e) vbv[e] = p->host.W_inv[(size_t)j * N + vb.idx[e]];
    const double stop = p->host.max_bark, step = (M > 1) ? stop / (double)(M - 1) : 0.0;
    for (int j = 0; j < M; ++j) beta64[j] = step * (double)j;
    if (M > 1) beta64[M - 1] = stop;
    if (!st) st = p->tables.upload(wbv, &p->d_wb_val64);
    if (!st) st = p->tables.upload(wiv, &p->d_wi_val64);
    if (!st) st = p->tables.upload(wfv, &p->d_wf_val64);
    if (!st) st = p->tables.upload(vbv, &p->d_vb_val64);
    if (!st) st = p->tables.upload(p->host.S, &p->d_S64);
    if (!st) st = p->tables.upload(p->host.quiet, &p->d_quiet64);
    if (!st) st = p->tables.upload(beta64, &p->d_beta64);
  }
  {
    // quantiser: scale-factor band offsets and the band of every bin (ac_quant.hip)
    std::vector<int32_t> qoff;
    scale_bands(sample_rate, N, M, qoff);
    std::vector<uint16_t> qband(N);
    for (int j = 0; j < M; ++j)
      for (int i = qoff[j]; i < qoff[j + 1]; ++i) qband[i] = (uint16_t)j;
    if (!st) st = p->tables.upload(qoff, &p->d_qoff);
    if (!st) st = p->tables.upload(qband, &p->d_qband);
  }
  if (!st && fast_psy_supported(p)) {
    st = fast_psy_plan_init(p);
    if (!st) p->fast = 1;
  }
  if (!st && mid_psy_supported(p)) {   // (beside the fused epilogue's tables where both apply: more than two channels, psy_mid_serves)
    st = mid_psy_plan_init(p);
    if (!st) p->mid = 1;
    if (!st && runs_psy_plan_init(p) == AC_EHIP) st = AC_EHIP;   // (tables without the run structure keep the band walk)
  }
  if (!st && spreading != AC_SPREAD_F32) {
    if (p->fast) {
      p->spread = spreading;
    } else {
      set_error("the matrix-core spreading product needs the wave-level masking model (filter_bands_n 1024 or 2048, 64 Bark "
                "bands); got filter_bands_n = %d, bark_bands_n = %d", N, M);
      st = AC_EUNSUPPORTED;
    }
  }
  if (!st) st = creation_done();
  if (st) {
    ac_psy_plan_destroy(p);
    return st;
  }
  *out = p;
  return AC_OK;
}

// `plan` with a row budget, as a plan of its own: the same constants, built again for the same device (it owns its tables)
int ac_psy_plan_with_row_budget(const ac_psy_plan* plan, int row_bits, int kmin, ac_psy_plan** out) {
  AC_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  AC_REQUIRE(plan != nullptr, "plan is NULL");
  AC_REQUIRE(kmin >= -254 && kmin <= 254, "kmin (%d) outside [-254, 254]", kmin);
  AC_REQUIRE(row_bits >= 5 * plan->M, "row_bits (%d) below 5 * bark_bands_n = %d, the length of a row that stores no band",
             row_bits, 5 * plan->M);
  ac_psy_plan* p = nullptr;
  const int st = psy_plan_build(plan->N, plan->M, plan->sample_rate, plan->alpha, plan->device, plan->spread, plan->pre, &p);
  if (st) return st;
  p->row_bits = row_bits;
  p->kmin = kmin;
  *out = p;
  return AC_OK;
}

int ac_psy_plan_row_budget(const ac_psy_plan* plan, int* row_bits, int* kmin) {
  AC_REQUIRE(plan != nullptr, "plan is NULL");
  if (row_bits) *row_bits = plan->row_bits;
  if (kmin) *kmin = plan->row_bits ? plan->kmin : 0;
  return AC_OK;
}

int ac_psy_plan_destroy(ac_psy_plan* p) {
  if (!p) return AC_OK;
  DeviceGuard guard(p->device);
  p->tables.release();
  delete p;
  return AC_OK;
}

int ac_mdct_plan_is_fast(const ac_mdct_plan* p) { return p ? p->fast : 0; }

int ac_psy_plan_is_fast(const ac_psy_plan* p) { return p ? p->fast : 0; }
int ac_psy_plan_spreading(const ac_psy_plan* p) { return p ? p->spread : 0; }
int ac_psy_plan_tier(const ac_psy_plan* p) { return !p ? 0 : p->fast ? 2 : p->mid ? 1 : 0; }

int ac_mdct_plan_tier(const ac_mdct_plan* p, int C) {
  if (!p || C < 1) return -1;
  if (wave_level(p, C, 0, 1)) return 3;
  return lds_fft_tier_of(p, C);
}

}  // extern "C"
