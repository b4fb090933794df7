// C ABI of libaudiocodec_amd.so (see include/audiocodec_amd.h).  gfx950 only.  This unit: the error state, the test hooks and
// the host-only builders; the entry points that touch the device are in ac_api_plan / _encode / _quant / _stream.hip.
#include <cstdlib>
#include <cstring>

#include "ac_api_internal.h"

namespace ac {

static thread_local std::string g_err;
int g_force_generic = 0;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

bool env_is_1(const char* name) {
  const char* e = getenv(name);
  return e && atoi(e) == 1;
}

}  // namespace ac

using namespace ac;

extern "C" {

int ac_version(void) { return AC_VERSION; }
const char* ac_last_error(void) { return g_err.c_str(); }

int ac_set_force_generic(int on) {
  // a test hook, not a product switch: honoured only in processes started with AC_TESTING=1 (read once)
  static const bool testing = [] { const char* e = getenv("AC_TESTING"); return e && atoi(e) != 0; }();
  if (!testing) {
    set_error("ac_set_force_generic is a test hook: start the process with AC_TESTING=1 to use it");
    return AC_EUNSUPPORTED;
  }
  g_force_generic = on ? 1 : 0;
  return AC_OK;
}

int ac_testing_runs_image(int N, int M, double sample_rate, double alpha, int precompute, unsigned* image, int cap, int* layout) {
  AC_REQUIRE(N >= 2 && (N & 1) == 0 && M >= 1 && layout, "ac_testing_runs_image: bad arguments");
  PsyTables t;
  psy_tables(N, M, sample_rate, alpha, t, precompute);
  std::vector<uint32_t> w;
  RunsLayout L;
  if (!build_runs(t, &w, &L)) {
    set_error("tables without the run structure");
    return AC_EUNSUPPORTED;
  }
  const int v[17] = {L.words, L.lw, L.kb, L.n4, L.n16, L.n64, L.o4, L.o16, L.o64, L.oz, L.slot,
                     L.off_S, L.off_bc, L.off_bd, L.off_lst, L.off_bw, L.off_idx};
  for (int i = 0; i < 17; ++i) layout[i] = v[i];
  if (image)
    for (int i = 0; i < L.words && i < cap; ++i) image[i] = w[(size_t)i];
  return AC_OK;
}

// ---- host-only builders ------------------------------------------------------------------------

int ac_mdct_fold_coefficients_host(int N, int window, double* coef) {
  return ac_mdct_fold_coefficients_host_pre(N, window, AC_F64, coef);
}

int ac_mdct_fold_coefficients_host_pre(int N, int window, int precompute, double* coef) {
  AC_REQUIRE(N >= 2 && (N % 2) == 0, "number of filters used in mdct transformation needs to be even (got %d)", N);
  AC_REQUIRE(valid_window(window), "unknown window id %d", window);
  AC_REQUIRE_PRE(precompute);
  AC_REQUIRE(coef != nullptr, "coef is NULL");
  FoldCoef c;
  fold_coefficients(N, window, c, precompute);
  const int h = N / 2;
  const std::vector<double>* v[8] = {&c.a1, &c.a2, &c.a3, &c.a4, &c.s1, &c.s2, &c.s3, &c.s4};
  for (int i = 0; i < 8; ++i) std::memcpy(coef + (size_t)i * h, v[i]->data(), h * sizeof(double));
  return AC_OK;
}

int ac_mdct_dense_matrices_host(int N, int window, float* H, float* H_inv) {
  return ac_mdct_dense_matrices_host_pre(N, window, AC_F64, H, H_inv);
}

int ac_mdct_dense_matrices_host_pre(int N, int window, int precompute, float* H, float* H_inv) {
  AC_REQUIRE(N >= 2 && (N % 2) == 0, "number of filters used in mdct transformation needs to be even (got %d)", N);
  AC_REQUIRE(valid_window(window), "unknown window id %d", window);
  AC_REQUIRE_PRE(precompute);
  FoldCoef c;
  fold_coefficients(N, window, c, precompute);
  const int h = N / 2;
  const size_t NN = (size_t)N * N;
  if (H) {
    // H[n, r, k] = F[r, k] d_n[k]; n = 0 uses columns k >= h (current block), n = 1 columns k < h
    std::memset(H, 0, 2 * NN * sizeof(float));
    for (int j = 0; j < h; ++j) {
      H[0 * NN + (size_t)j * N + (h + j)] = (float)c.a1[j];                  // F[j, h+j]
      H[0 * NN + (size_t)(N - 1 - j) * N + (h + j)] = (float)c.a2[j];        // F[N-1-j, h+j]
      H[1 * NN + (size_t)(h - 1 - j) * N + j] = (float)c.a3[j];              // F[h-1-j, j]
      H[1 * NN + (size_t)(h + j) * N + j] = (float)c.a4[j];                  // F[h+j, j]
    }
  }
  if (H_inv) {
    // H_inv[n, r, k] = e_n[r] Finv[r, k]; n = 0 rows r < h, n = 1 rows r >= h
    std::memset(H_inv, 0, 2 * NN * sizeof(float));
    for (int j = 0; j < h; ++j) {
      H_inv[0 * NN + (size_t)(h - 1 - j) * N + j] = (float)c.s1[j];          // Finv[h-1-j, j]
      H_inv[0 * NN + (size_t)(h - 1 - j) * N + (N - 1 - j)] = (float)c.s3[j];
      H_inv[1 * NN + (size_t)(h + j) * N + j] = (float)c.s2[j];              // Finv[h+j, j]
      H_inv[1 * NN + (size_t)(h + j) * N + (N - 1 - j)] = (float)c.s4[j];
    }
  }
  return AC_OK;
}

int ac_psy_tables_host(int N, int M, double sample_rate, double alpha, float* W, float* W_inv, float* S,
                       float* quiet, double* scalars) {
  AC_REQUIRE(N >= 1 && M >= 1, "filter_bands_n (%d) and bark_bands_n (%d) must be positive", N, M);
  AC_REQUIRE(sample_rate > 0 && alpha > 0, "sample_rate and alpha must be positive");
  PsyTables t;
  psy_tables(N, M, sample_rate, alpha, t);
  if (W) for (size_t i = 0; i < t.W.size(); ++i) W[i] = (float)t.W[i];
  if (W_inv) for (size_t i = 0; i < t.W_inv.size(); ++i) W_inv[i] = (float)t.W_inv[i];
  if (S) for (size_t i = 0; i < t.S.size(); ++i) S[i] = (float)t.S[i];
  if (quiet) for (size_t i = 0; i < t.quiet.size(); ++i) quiet[i] = (float)t.quiet[i];
  if (scalars) {
    scalars[0] = t.max_frequency;
    scalars[1] = t.max_bark;
    scalars[2] = t.bark_band_width;
    scalars[3] = t.dB_MIN;
  }
  return AC_OK;
}

int ac_psy_tables_host_f64(int N, int M, double sample_rate, double alpha, double* W, double* W_inv, double* S,
                           double* quiet, double* scalars) {
  return ac_psy_tables_host_pre(N, M, sample_rate, alpha, AC_F64, W, W_inv, S, quiet, scalars);
}

int ac_psy_tables_host_pre(int N, int M, double sample_rate, double alpha, int precompute, double* W, double* W_inv,
                           double* S, double* quiet, double* scalars) {
  AC_REQUIRE(N >= 1 && M >= 1, "filter_bands_n (%d) and bark_bands_n (%d) must be positive", N, M);
  AC_REQUIRE(sample_rate > 0 && alpha > 0, "sample_rate and alpha must be positive");
  AC_REQUIRE_PRE(precompute);
  PsyTables t;
  psy_tables(N, M, sample_rate, alpha, t, precompute);
  if (W) std::copy(t.W.begin(), t.W.end(), W);
  if (W_inv) std::copy(t.W_inv.begin(), t.W_inv.end(), W_inv);
  if (S) std::copy(t.S.begin(), t.S.end(), S);
  if (quiet) std::copy(t.quiet.begin(), t.quiet.end(), quiet);
  if (scalars) {
    scalars[0] = t.max_frequency;
    scalars[1] = t.max_bark;
    scalars[2] = t.bark_band_width;
    scalars[3] = t.dB_MIN;
  }
  return AC_OK;
}

int ac_psy_scale_bands_host(double sample_rate, int filter_bands_n, int bark_bands_n, int32_t* offsets) {
  AC_REQUIRE(filter_bands_n >= 1 && bark_bands_n >= 1, "filter_bands_n (%d) and bark_bands_n (%d) must be positive",
             filter_bands_n, bark_bands_n);
  AC_REQUIRE(sample_rate > 0, "sample_rate must be positive");
  AC_REQUIRE(offsets != nullptr, "offsets is NULL");
  std::vector<int32_t> off;
  scale_bands(sample_rate, filter_bands_n, bark_bands_n, off);
  std::copy(off.begin(), off.end(), offsets);
  return AC_OK;
}

}  // extern "C"
