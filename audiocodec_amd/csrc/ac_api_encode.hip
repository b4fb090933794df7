// C ABI, analysis side: the transform, the masking model and their backward passes, the fused encode with its forms that
// emit codes or packed rows or transrate them, their *_launches queries, and the placement probe.
#include "ac_api_internal.h"

namespace ac {

// whether the wave-level kernels take this call (plans at filters_n 512 / 256 serve a subset, see ac_internal.h)
bool wave_level(const ac_mdct_plan* p, int C, int iof, int blocks) {
  if (!p->fast || g_force_generic) return false;
  // float32 tensors of more than two channels: the channel-pair instances of the LDS-FFT tier (2.2 - 3 TB/s) rather than
  // the wave-level kernels' strided form (0.9 - 1.5); every float32 route -- one-shot, streaming, the encode -- asks here, so
  // they stay bit-equal to each other.  16-bit PCM of more than two channels keeps the strided form.
  if (iof == 0 && C > 2 && lds_fft_tier_of(p, C) == 2) return false;
  return fast_mdct_frames_per_wave(p->N) == 1 || fast_multi_serves(p, C, iof, blocks);
}
// Which masking-model kernels serve C channels of a plan: the general-layout ones (strided channel pairs) take more than
// two channels off the fused epilogue's kernels too when the plan holds both forms and runs the default spreading product
// (theirs: split bfloat16 on the matrix cores)
bool psy_mid_serves(const ac_psy_plan* p, int C) {
  return p->mid && !g_force_generic && (!p->fast || (C > 2 && p->spread == AC_SPREAD_BF16X2_MFMA));
}
bool psy_fast_serves(const ac_psy_plan* p, int C) { return p->fast && !g_force_generic && !psy_mid_serves(p, C); }
int check_dims(int B, int K, int C) {
  AC_REQUIRE(B >= 0 && K >= 0 && C >= 0, "negative dimension (B=%d, blocks=%d, C=%d)", B, K, C);
  return AC_OK;
}
// a transform plan and a masking-model plan that one call takes together
int check_plan_pair(const ac_mdct_plan* mdct, const ac_psy_plan* psy) {
  AC_REQUIRE(mdct != nullptr && psy != nullptr, "plan is NULL");
  AC_REQUIRE(mdct->N == psy->N, "mdct filters_n (%d) != psychoacoustic filter_bands_n (%d)", mdct->N, psy->N);
  AC_REQUIRE(mdct->device == psy->device, "plans live on different devices");
  return AC_OK;
}
// the slot length of a caller's ac_packed_out: the one the plan's row budget gives
int check_row_bytes(const ac_packed_out& po, const ac_psy_plan* psy) {
  AC_REQUIRE(po.row_bytes == plan_row_bytes(psy), "row_bytes (%lld) is not the plan's ceil(%d / 32) * 4 = %lld",
             (long long)po.row_bytes, psy->row_bits, (long long)plan_row_bytes(psy));
  return AC_OK;
}
// what the calls that take packed rows to packed rows (AC_IN_PACKED, AC_IN_MIX) ask of their plans and float tensors
int check_rows_to_rows(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const float* X, const float* t, const float* thr, int B,
                       int K, int C, const char* flag) {
  int st = check_plan_pair(mdct, psy);
  if (!st) st = check_dims(B, K, C);
  if (!st) st = check_quant(psy, B, K + 1, C);
  if (st) return st;
  AC_REQUIRE(psy->row_bits != 0, "%s needs a plan with a row budget (ac_psy_plan_with_row_budget)", flag);
  AC_REQUIRE(X == nullptr && t == nullptr && thr == nullptr, "%s writes no X, t or thr: they must be NULL", flag);
  return AC_OK;
}
static int refuse_pcm16() {
  set_error("16-bit PCM is served at filters_n 64 ... 2048 in powers of two ('vorbis' or 'sine' window; below 1024: mono / "
            "stereo) and at 120 / 240 / 480 / 960 / 1920 / 576 / 1152 (mono / stereo)");
  return AC_EUNSUPPORTED;
}

static int mdct_forward(const ac_mdct_plan* p, const void* x, bool pcm16, float* X, int B, int K, int C, void* stream) {
  AC_REQUIRE(p != nullptr, "plan is NULL");
  int st = check_dims(B, K, C);
  if (st) return st;
  if (B == 0 || C == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && (x != nullptr || K == 0), "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(x, X);
  DeviceGuard guard(p->device);
  hipStream_t s = (hipStream_t)stream;
  if (wave_level(p, C, pcm16 ? 1 : 0, K))
    return launch_fwd_fast(p, nullptr, x, pcm16, X, nullptr, nullptr, 0.f, nullptr, B, K, K + 1, C, s);
  if (pcm16) {
    if (lds_fft_serves_pcm16(p, C)) return launch_fwd_lds_pcm16(p, static_cast<const int16_t*>(x), X, B, K, C, s);
    return refuse_pcm16();
  }
  return launch_fwd_typed(p, x, X, nullptr, AC_F32, B, K, K + 1, C, s);
}

int mdct_inverse(const ac_mdct_plan* p, const float* X, void* x, bool pcm16, int B, int Kp, int C, void* stream) {
  AC_REQUIRE(p != nullptr, "plan is NULL");
  int st = check_dims(B, Kp, C);
  if (st) return st;
  if (B == 0 || C == 0) return AC_OK;
  AC_REQUIRE(x != nullptr && (X != nullptr || Kp == 0), "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(x, X);
  DeviceGuard guard(p->device);
  hipStream_t s = (hipStream_t)stream;
  if (wave_level(p, C, pcm16 ? 1 : 0, Kp)) return launch_inv_fast(p, X, x, pcm16, nullptr, nullptr, B, Kp, Kp + 1, C, s);
  if (pcm16) {
    if (lds_fft_serves_pcm16(p, C)) return launch_inv_lds_pcm16(p, X, static_cast<int16_t*>(x), B, Kp, C, s);
    return refuse_pcm16();
  }
  return launch_inv_typed(p, X, x, nullptr, nullptr, AC_F32, B, Kp, Kp + 1, C, s);
}

// Whether AC_EMIT_CODES is one launch (k_fwd_fast_q); AC_ENCODE_QUANT_NOFUSE=1 sends every configuration down the two
// launches.  (This hook and its three kin are for A/B measurements: read per call, so that one process can time both forms)
static bool encode_quantized_fuses(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C) {
  if (env_is_1("AC_ENCODE_QUANT_NOFUSE")) return false;
  return !g_force_generic && wave_level(mdct, C, 0, 1) && psy_fast_serves(psy, C) && fast_encode_quant_serves(mdct, psy, C);
}
// whether AC_EMIT_PACKED is one launch (k_fwd_fast_qp); AC_ENCODE_PACKED_NOFUSE=1 sends every configuration down the composition
bool encode_packed_fuses(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C) {
  if (env_is_1("AC_ENCODE_PACKED_NOFUSE")) return false;
  return encode_quantized_fuses(mdct, psy, C) && fast_encode_pack_serves(mdct, psy, C);
}
// whether packed rows are transrated in one launch (k_transrate_p); AC_TRANSRATE_NOFUSE=1: as above
static bool transrate_fuses(const ac_psy_plan* psy) {
  if (env_is_1("AC_TRANSRATE_NOFUSE")) return false;
  return !g_force_generic && transrate_serves(psy);
}
// whether the packed rows of S sources are mixed in one launch (k_mix_p); AC_MIX_NOFUSE=1: as above
static bool mix_fuses(const ac_psy_plan* psy, int S) {
  if (env_is_1("AC_MIX_NOFUSE")) return false;
  return transrate_fuses(psy) && mix_serves(psy, S);
}
// whether the packed rows of S sources are routed to O outputs in one launch (k_route_p); AC_ROUTE_NOFUSE=1: as above
static bool route_fuses(const ac_psy_plan* psy, int S, int O) {
  if (env_is_1("AC_ROUTE_NOFUSE")) return false;
  return mix_fuses(psy, S) && route_serves(psy, S, O);
}
// whether the level of packed rows is one launch (k_level_p); AC_LEVEL_NOFUSE=1: as above
static bool level_fuses(const ac_psy_plan* psy) {
  if (env_is_1("AC_LEVEL_NOFUSE")) return false;
  return !g_force_generic && level_serves(psy);
}
// whether packed rows are protected in one launch (k_protect_p); AC_PROTECT_NOFUSE=1: as above
static bool protect_fuses(const ac_psy_plan* psy, int red_bits) {
  if (env_is_1("AC_PROTECT_NOFUSE")) return false;
  return transrate_fuses(psy) && protect_serves(psy, red_bits);
}

}  // namespace ac

using namespace ac;

extern "C" {

int ac_mdct_forward(const ac_mdct_plan* p, const float* x, float* X, int B, int K, int C, void* stream) {
  return mdct_forward(p, x, false, X, B, K, C, stream);
}
int ac_mdct_forward_pcm16(const ac_mdct_plan* p, const int16_t* x, float* X, int B, int K, int C, void* stream) {
  return mdct_forward(p, x, true, X, B, K, C, stream);
}
int ac_mdct_inverse(const ac_mdct_plan* p, const float* X, float* x, int B, int Kp, int C, void* stream) {
  return mdct_inverse(p, X, x, false, B, Kp, C, stream);
}
int ac_mdct_inverse_pcm16(const ac_mdct_plan* p, const float* X, int16_t* x, int B, int Kp, int C, void* stream) {
  return mdct_inverse(p, X, x, true, B, Kp, C, stream);
}

int ac_tonality(const ac_psy_plan* p, const float* X, float* t, int B, int F, int C, void* stream) {
  AC_REQUIRE(p != nullptr, "plan is NULL");
  int st = check_dims(B, F, C);
  if (st) return st;
  if (B == 0 || C == 0 || F == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && t != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(X);
  DeviceGuard guard(p->device);
  hipStream_t s = (hipStream_t)stream;
  if (psy_fast_serves(p, C)) return launch_psy_fast(p, X, nullptr, t, nullptr, 0.f, B, F, C, s);
  if (psy_mid_serves(p, C)) return launch_psy_mid(p, X, nullptr, t, nullptr, 0.f, B, F, C, s);
  return launch_tonality_typed(p, X, t, AC_F32, B, F, C, s);
}

int ac_mask_threshold(const ac_psy_plan* p, const float* X, const float* t, float drown, float* thr, int B, int F,
                      int C, void* stream) {
  AC_REQUIRE(p != nullptr, "plan is NULL");
  int st = check_dims(B, F, C);
  if (st) return st;
  if (B == 0 || C == 0 || F == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && t != nullptr && thr != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(X, thr);
  DeviceGuard guard(p->device);
  hipStream_t s = (hipStream_t)stream;
  if (psy_fast_serves(p, C)) return launch_psy_fast(p, X, t, nullptr, thr, drown, B, F, C, s);
  if (psy_mid_serves(p, C)) return launch_psy_mid(p, X, t, nullptr, thr, drown, B, F, C, s);
  return launch_threshold_typed(p, X, t, drown, thr, AC_F32, B, F, C, s);
}

int ac_tonality_backward(const ac_psy_plan* p, const float* X, const float* grad_t, float* grad_X, int accumulate, int B,
                         int F, int C, void* stream) {
  AC_REQUIRE(p != nullptr, "plan is NULL");
  int st = check_dims(B, F, C);
  if (st) return st;
  if (B == 0 || C == 0 || F == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && grad_t != nullptr && grad_X != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(X, grad_X);
  DeviceGuard guard(p->device);
  if (p->fast && !g_force_generic)
    return launch_psy_bwd_fast(p, X, nullptr, 0.f, nullptr, grad_t, grad_X, nullptr, accumulate, B, F, C,
                               (hipStream_t)stream);
  return launch_tonality_bwd_typed(p, X, grad_t, grad_X, accumulate, AC_F32, B, F, C, (hipStream_t)stream);
}

int ac_mask_threshold_backward(const ac_psy_plan* p, const float* X, const float* t, float drown, const float* grad_thr,
                               float* grad_X, float* grad_t, int B, int F, int C, void* stream) {
  AC_REQUIRE(p != nullptr, "plan is NULL");
  int st = check_dims(B, F, C);
  if (st) return st;
  if (B == 0 || C == 0 || F == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && t != nullptr && grad_thr != nullptr && grad_X != nullptr && grad_t != nullptr,
             "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(X, grad_thr, grad_X);
  DeviceGuard guard(p->device);
  if (p->fast && !g_force_generic)
    return launch_psy_bwd_fast(p, X, t, drown, grad_thr, nullptr, grad_X, grad_t, 0, B, F, C, (hipStream_t)stream);
  return launch_threshold_bwd_typed(p, X, t, drown, grad_thr, grad_X, grad_t, AC_F32, B, F, C, (hipStream_t)stream);
}

static int encode_fused(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const void* x, bool pcm16, float* X, float* t,
                        float* thr, float drown, int B, int K, int C, void* stream) {
  int st = check_plan_pair(mdct, psy);
  if (!st) st = check_dims(B, K, C);
  if (st) return st;
  if (B == 0 || C == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && t != nullptr && thr != nullptr && (x != nullptr || K == 0), "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(x, X, thr);
  DeviceGuard guard(mdct->device);
  hipStream_t s = (hipStream_t)stream;
  if (mdct->fast && psy->fast && !g_force_generic && wave_level(mdct, C, pcm16 ? 1 : 0, K) && psy_fast_serves(psy, C)) {
    if (!fused_encode_takes_two_launches(mdct->N, C, pcm16 ? 1 : 0))
      return launch_fwd_fast(mdct, psy, x, pcm16, X, t, thr, drown, nullptr, B, K, K + 1, C, s);
    st = launch_fwd_fast(mdct, nullptr, x, pcm16, X, nullptr, nullptr, 0.f, nullptr, B, K, K + 1, C, s);
    if (!st) st = launch_psy_fast(psy, X, nullptr, t, thr, drown, B, K + 1, C, s);
    return st;
  }
  // filters_n 64 ... 512: the several-frames-per-wave kernels with the general-layout masking model in the same launch
  if (!g_force_generic && mdct->fast && fast_multi_fuses(mdct, psy, C, pcm16 ? 1 : 0, K))
    return launch_fwd_fast(mdct, psy, x, 0, X, t, thr, drown, nullptr, B, K, K + 1, C, s);
  // the LDS-FFT tier's instances with the masking model on the frame while it is in LDS
  if (!pcm16 && !wave_level(mdct, C, 0, K) && K >= 1 && wave_encode_fuses(mdct, psy, C, x, X, thr))
    return launch_enc_wave(mdct, psy, static_cast<const float*>(x), X, t, thr, drown, nullptr, B, K, K + 1, C, s);
  // un-fused composition for configurations the fused kernel does not cover: the transform, then tonality + threshold in
  // one wave-level pass over X where the general-layout masking kernels serve the plan, else the two generic kernels
  st = mdct_forward(mdct, x, pcm16, X, B, K, C, stream);
  if (!st && psy_mid_serves(psy, C)) return launch_psy_mid(psy, X, nullptr, t, thr, drown, B, K + 1, C, s);
  if (!st) st = ac_tonality(psy, X, t, B, K + 1, C, stream);
  if (!st) st = ac_mask_threshold(psy, X, t, drown, thr, B, K + 1, C, stream);
  return st;
}

int ac_encode_launches(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C) {
  if (!plans_match(mdct, psy) || C < 1) return 0;
  if (g_force_generic) return 3;
  if (mdct->fast && psy->fast && wave_level(mdct, C, 0, 1) && psy_fast_serves(psy, C))
    return fused_encode_takes_two_launches(mdct->N, C, 0) ? 2 : 1;
  if (mdct->fast && fast_multi_fuses(mdct, psy, C, 0, 1)) return 1;
  if (!wave_level(mdct, C, 0, 1) && wave_encode_fuses(mdct, psy, C, nullptr, nullptr, nullptr)) return 1;   // (tensors on the 16-byte grid)
  return (psy_mid_serves(psy, C) || psy_fast_serves(psy, C)) ? 2 : 3;
}

int ac_encode_fused(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const float* x, float* X, float* t, float* thr,
                    float drown, int B, int K, int C, void* stream) {
  return encode_fused(mdct, psy, x, false, X, t, thr, drown, B, K, C, stream);
}

int ac_encode_quantized_launches(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C) {
  if (!plans_match(mdct, psy) || C < 1) return 0;
  return encode_quantized_fuses(mdct, psy, C) ? 1 : 2;
}
// (16-bit PCM: every instance of k_fwd_fast_q16 / qb16 passed its register gate, so the one launch serves where the float32
// one does)
int ac_encode_quantized_launches_pcm16(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C) {
  return ac_encode_quantized_launches(mdct, psy, C);
}

// ac_encode_fused_ex with AC_EMIT_CODES (pcm16: with AC_IN_PCM16, x is int16)
static int encode_quantized(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const void* x, bool pcm16, float* X, float* t,
                            float* thr, float drown, int16_t* codes, int8_t* sf, int B, int K, int C, void* stream) {
  int st = check_plan_pair(mdct, psy);
  if (!st) st = check_dims(B, K, C);
  if (!st) st = check_quant(psy, B, K + 1, C);
  if (st) return st;
  if (B == 0 || C == 0) return AC_OK;
  AC_REQUIRE(codes != nullptr && sf != nullptr, "AC_EMIT_CODES without its output tensors (codes, sf)");
  if (encode_quantized_fuses(mdct, psy, C)) {
    AC_REQUIRE(x != nullptr || K == 0, "NULL tensor pointer");
    AC_REQUIRE_ALIGNED(x, X, thr, codes, sf);
    DeviceGuard guard(mdct->device);
    // at the plan's row budget where it has one, as quantize_of_plan
    const auto launch = psy->row_bits ? (pcm16 ? launch_fwd_fast_quant_budget_pcm16 : launch_fwd_fast_quant_budget)
                                      : (pcm16 ? launch_fwd_fast_quant_pcm16 : launch_fwd_fast_quant);
    return launch(mdct, psy, x, X, t, thr, drown, codes, sf, B, K, K + 1, C, (hipStream_t)stream);
  }
  AC_REQUIRE(X != nullptr && t != nullptr && thr != nullptr,
             "AC_EMIT_CODES: X, t and thr are required as intermediates where ac_encode_quantized_launches%s() returns 2",
             pcm16 ? "_pcm16" : "");
  AC_REQUIRE_ALIGNED(codes, sf);
  st = encode_fused(mdct, psy, x, pcm16, X, t, thr, drown, B, K, C, stream);
  if (st) return st;
  DeviceGuard guard(psy->device);
  return quantize_of_plan(psy, X, thr, codes, sf, B, K + 1, C, (hipStream_t)stream);
}

int ac_encode_packed_launches(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C) {
  if (!plans_match(mdct, psy) || C < 1 || !psy->row_bits) return 0;
  return encode_packed_fuses(mdct, psy, C) ? 1 : ac_encode_launches(mdct, psy, C) + 2;
}
// (16-bit PCM: every instance of k_fwd_fast_qp16 passed its register gate)
int ac_encode_packed_launches_pcm16(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C) {
  return ac_encode_packed_launches(mdct, psy, C);
}

// ac_encode_fused_ex with AC_EMIT_PACKED (pcm16: with AC_IN_PCM16, x is int16)
static int encode_packed_rows(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const void* x, bool pcm16, const float* X,
                              const float* t, const float* thr, float drown, const ac_packed_out* out, const void* out1, int B,
                              int K, int C, void* stream) {
  int st = check_plan_pair(mdct, psy);
  if (!st) st = check_dims(B, K, C);
  if (!st) st = check_quant(psy, B, K + 1, C);
  if (st) return st;
  AC_REQUIRE(psy->row_bits != 0, "AC_EMIT_PACKED needs a plan with a row budget (ac_psy_plan_with_row_budget)");
  AC_REQUIRE(X == nullptr && t == nullptr && thr == nullptr, "AC_EMIT_PACKED writes no X, t or thr: they must be NULL");
  AC_REQUIRE(out1 == nullptr, "AC_EMIT_PACKED takes one ac_packed_out as out0: out1 must be NULL");
  AC_REQUIRE(out != nullptr, "AC_EMIT_PACKED without its ac_packed_out");
  const ac_packed_out po = *out;
  st = check_row_bytes(po, psy);
  if (st) return st;
  if (B == 0 || C == 0) return AC_OK;
  if (!encode_packed_fuses(mdct, psy, C)) {
    set_error("AC_EMIT_PACKED: no kernel encodes to packed rows in one launch for filters_n = %d, bark_bands_n = %d, %d "
              "channels, row budget %d here (ac_encode_packed_launches%s() != 1): use the composition -- %s, "
              "ac_quantize_budget, then ac_pack at row starts r * row_bytes into zero-filled data",
              mdct->N, psy->M, C, psy->row_bits, pcm16 ? "_pcm16" : "", pcm16 ? "ac_encode_fused_pcm16" : "ac_encode_fused");
    return AC_EUNSUPPORTED;
  }
  AC_REQUIRE(po.data != nullptr && po.fits != nullptr && (x != nullptr || K == 0), "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(x, po.data);
  DeviceGuard guard(mdct->device);
  return (pcm16 ? launch_fwd_fast_pack_rows_pcm16 : launch_fwd_fast_pack_rows)(mdct, psy, x, drown, po.data, po.row_bytes, po.fits,
                                                                              B, K, K + 1, C, (hipStream_t)stream);
}

int ac_transrate_launches(const ac_psy_plan* psy, int C) {
  if (!psy || C < 1 || !psy->row_bits) return 0;
  return transrate_fuses(psy) ? 1 : 3;   // ac_unpack, ac_quantize_budget (thr == NULL), ac_pack
}

// ac_encode_fused_ex with AC_IN_PACKED | AC_EMIT_PACKED: rows [B,K+1,C] of `in` to slots of `out` at the plan's row budget
static int transrate_packed_rows(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const ac_packed_rows* in, const float* X,
                                 const float* t, const float* thr, const ac_packed_out* out, int16_t* offset, int B, int K,
                                 int C, void* stream) {
  int st = check_rows_to_rows(mdct, psy, X, t, thr, B, K, C, "AC_IN_PACKED");
  if (st) return st;
  AC_REQUIRE(in != nullptr, "AC_IN_PACKED without its ac_packed_rows (x)");
  AC_REQUIRE(out != nullptr, "AC_IN_PACKED without its ac_packed_out (out0)");
  const ac_packed_rows rows = *in;
  const ac_packed_out po = *out;
  st = check_row_bytes(po, psy);
  if (st) return st;
  // (refused ahead of the empty shape and of the "no kernel" refusal, as ac_unpack does; check_packed_rows asks again below)
  AC_REQUIRE(rows.nbytes >= 0, "negative nbytes (%lld)", (long long)rows.nbytes);
  if (B == 0 || C == 0) return AC_OK;
  if (!transrate_fuses(psy)) {
    set_error("AC_IN_PACKED: no kernel transrates packed rows in one launch for filters_n = %d, bark_bands_n = %d, row budget "
              "%d here (ac_transrate_launches() != 1): use the composition -- ac_unpack, ac_quantize_budget with thr == NULL "
              "at kmin 0, then ac_pack at row starts r * row_bytes into zero-filled data", psy->N, psy->M, psy->row_bits);
    return AC_EUNSUPPORTED;
  }
  st = check_packed_rows(rows, true, po.data != nullptr && po.fits != nullptr);
  if (st) return st;
  AC_REQUIRE_ALIGNED(po.data, offset);
  DeviceGuard guard(psy->device);
  return launch_transrate(psy, rows.data, rows.nbytes, rows.index, po.data, po.row_bytes, po.fits, offset,
                          (long long)B * (K + 1) * C, (hipStream_t)stream);
}

int ac_mix_launches(const ac_psy_plan* psy, int C, int S) {
  if (!psy || C < 1 || S < 1 || !psy->row_bits) return 0;
  return mix_fuses(psy, S) ? 1 : 2 * S + 2;   // S ac_unpack, S ac_dequantize, ac_quantize_budget, ac_pack
}

// ac_encode_fused_ex with AC_IN_PACKED | AC_EMIT_PACKED | AC_IN_MIX: rows [B,K+1,C] of every source of `in` summed into slots of
// `out` at the plan's row budget
static int mix_packed_rows(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const ac_mix_rows* in, const float* X, const float* t,
                           const float* thr, const ac_packed_out* out, int16_t* offset, int B, int K, int C, void* stream) {
  int st = check_rows_to_rows(mdct, psy, X, t, thr, B, K, C, "AC_IN_MIX");
  if (st) return st;
  AC_REQUIRE(in != nullptr, "AC_IN_MIX without its ac_mix_rows (x)");
  AC_REQUIRE(out != nullptr, "AC_IN_MIX without its ac_packed_out (out0)");
  const ac_mix_rows mix = *in;
  const ac_packed_out po = *out;
  st = check_row_bytes(po, psy);
  if (st) return st;
  AC_REQUIRE(mix.sources_n >= 1, "sources_n (%d) below 1", (int)mix.sources_n);
  AC_REQUIRE(mix.src != nullptr, "ac_mix_rows: src is NULL");
  for (int i = 0; i < mix.sources_n; ++i) {
    AC_REQUIRE(mix.gain == nullptr || (mix.gain[i] >= -254 && mix.gain[i] <= 254), "gain[%d] (%d) outside [-254, 254]", i,
               mix.gain ? (int)mix.gain[i] : 0);
    AC_REQUIRE(mix.src[i].nbytes >= 0, "source %d: negative nbytes (%lld)", i, (long long)mix.src[i].nbytes);
    AC_REQUIRE(mix.src[i].index != nullptr || B == 0 || C == 0, "source %d: index is NULL", i);
  }
  if (B == 0 || C == 0) return AC_OK;
  if (!mix_fuses(psy, mix.sources_n)) {
    set_error("AC_IN_MIX: no kernel mixes the packed rows of %d sources in one launch for filters_n = %d, bark_bands_n = %d, row "
              "budget %d here (ac_mix_launches() != 1): use the composition -- ac_unpack and ac_dequantize per source at sf + "
              "gain, float32 adds in source order, ac_quantize_budget at kmin 0 under thr = step(s0) sqrt(3), then ac_pack at row "
              "starts r * row_bytes into zero-filled data", (int)mix.sources_n, psy->N, psy->M, psy->row_bits);
    return AC_EUNSUPPORTED;
  }
  for (int i = 0; i < mix.sources_n; ++i) {
    st = check_packed_rows(mix.src[i], true, po.data != nullptr && po.fits != nullptr);
    if (st) return st;
  }
  AC_REQUIRE_ALIGNED(po.data, offset);
  DeviceGuard guard(psy->device);
  return launch_mix(psy, mix.sources_n, mix.src, mix.gain, mix.active, po.data, po.row_bytes, po.fits, offset,
                    (long long)B * (K + 1) * C, (hipStream_t)stream);
}

int ac_route_launches(const ac_psy_plan* psy, int C, int S, int O) {
  if (!psy || C < 1 || S < 1 || O < 1 || !psy->row_bits) return 0;
  return route_fuses(psy, S, O) ? 1 : O * ac_mix_launches(psy, C, S);   // the AC_IN_MIX call of every output
}

// ac_encode_fused_ex with AC_IN_PACKED | AC_EMIT_PACKED | AC_IN_ROUTE: rows [B,K+1,C] of every source of `in` mixed into slots of
// every output of `out` at the plan's row budget
static int route_packed_rows(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const ac_route_rows* in, const float* X,
                             const float* t, const float* thr, const ac_packed_out* out, int16_t* offset, int B, int K, int C,
                             void* stream) {
  int st = check_rows_to_rows(mdct, psy, X, t, thr, B, K, C, "AC_IN_ROUTE");
  if (st) return st;
  AC_REQUIRE(in != nullptr, "AC_IN_ROUTE without its ac_route_rows (x)");
  AC_REQUIRE(out != nullptr, "AC_IN_ROUTE without its ac_packed_out (out0)");
  const ac_route_rows route = *in;
  const ac_packed_out po = *out;
  st = check_row_bytes(po, psy);
  if (st) return st;
  AC_REQUIRE(route.sources_n >= 1, "sources_n (%d) below 1", (int)route.sources_n);
  AC_REQUIRE(route.outputs_n >= 1, "outputs_n (%d) below 1", (int)route.outputs_n);
  AC_REQUIRE(route.src != nullptr, "ac_route_rows: src is NULL");
  AC_REQUIRE(route.gain != nullptr, "ac_route_rows: gain is NULL");
  for (long long k = 0; k < (long long)route.outputs_n * route.sources_n; ++k)
    AC_REQUIRE(route.gain[k] == AC_ROUTE_MUTE || (route.gain[k] >= -254 && route.gain[k] <= 254),
               "gain[%lld] (%d) is neither in [-254, 254] nor AC_ROUTE_MUTE", k, (int)route.gain[k]);
  for (int i = 0; i < route.sources_n; ++i) {
    AC_REQUIRE(route.src[i].nbytes >= 0, "source %d: negative nbytes (%lld)", i, (long long)route.src[i].nbytes);
    AC_REQUIRE(route.src[i].index != nullptr || B == 0 || C == 0, "source %d: index is NULL", i);
  }
  if (B == 0 || C == 0) return AC_OK;
  if (!route_fuses(psy, route.sources_n, route.outputs_n)) {
    set_error("AC_IN_ROUTE: no kernel routes the packed rows of %d sources to %d outputs in one launch for filters_n = %d, "
              "bark_bands_n = %d, row budget %d here (ac_route_launches() != 1): use the composition -- AC_IN_MIX per output on the "
              "sources it hears, in source order, at its gains", (int)route.sources_n, (int)route.outputs_n, psy->N, psy->M,
              psy->row_bits);
    return AC_EUNSUPPORTED;
  }
  for (int i = 0; i < route.sources_n; ++i) {
    st = check_packed_rows(route.src[i], true, po.data != nullptr && po.fits != nullptr);
    if (st) return st;
  }
  AC_REQUIRE_ALIGNED(po.data, offset);
  DeviceGuard guard(psy->device);
  return launch_route(psy, route.sources_n, route.outputs_n, route.src, route.gain, route.active, po.data, po.row_bytes, po.fits,
                      offset, (long long)B * (K + 1) * C, (hipStream_t)stream);
}

int ac_level_launches(const ac_psy_plan* psy, int C) {
  if (!psy || C < 1) return 0;
  return level_fuses(psy) ? 1 : 0;   // (elsewhere the library has no launch of its own: ac_unpack and the caller's sums)
}

// ac_encode_fused_ex with AC_IN_PACKED | AC_EMIT_LEVEL: the energy of rows [B,K+1,C] of `in`, and whether a row holds a bad band
// 
static int level_packed_rows(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const ac_packed_rows* in, const float* X,
                             const float* t, const float* thr, float* energy, uint8_t* bad, int B, int K, int C, void* stream) {
  int st = check_plan_pair(mdct, psy);
  if (!st) st = check_dims(B, K, C);
  if (!st) st = check_quant(psy, B, K + 1, C);
  if (st) return st;
  AC_REQUIRE(X == nullptr && t == nullptr && thr == nullptr, "AC_EMIT_LEVEL writes no X, t or thr: they must be NULL");
  AC_REQUIRE(in != nullptr, "AC_EMIT_LEVEL without its ac_packed_rows (x)");
  const ac_packed_rows rows = *in;
  AC_REQUIRE(rows.nbytes >= 0, "negative nbytes (%lld)", (long long)rows.nbytes);
  AC_REQUIRE(energy != nullptr || B == 0 || C == 0, "AC_EMIT_LEVEL without its energy tensor (out0)");
  if (B == 0 || C == 0) return AC_OK;
  if (!level_fuses(psy)) {
    set_error("AC_EMIT_LEVEL: no kernel takes the level of packed rows in one launch for filters_n = %d, bark_bands_n = %d here "
              "(ac_level_launches() != 1): use the composition -- ac_unpack, the squares of the codes summed per band as "
              "integers, fp32(fp32(Q) fp32(step(sf) step(sf))) per band, the fold tree of float32 adds", psy->N, psy->M);
    return AC_EUNSUPPORTED;
  }
  st = check_packed_rows(rows, true, true);
  if (st) return st;
  AC_REQUIRE_ALIGNED(energy);
  DeviceGuard guard(psy->device);
  return launch_level(psy, rows.data, rows.nbytes, rows.index, energy, bad, (long long)B * (K + 1) * C, (hipStream_t)stream);
}

// ac_encode_fused_ex with AC_SELECT_ACTIVE: the levels of S sources [S,B,K+1,C] to the active mask of the n loudest
static int select_active(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const ac_select_rows* in, const float* X, const float* t,
                         const float* thr, uint8_t* active, const void* out1, int B, int K, int C, void* stream) {
  int st = check_plan_pair(mdct, psy);
  if (!st) st = check_dims(B, K, C);
  if (st) return st;
  AC_REQUIRE(X == nullptr && t == nullptr && thr == nullptr && out1 == nullptr,
             "AC_SELECT_ACTIVE writes no X, t or thr and takes no out1: they must be NULL");
  AC_REQUIRE(in != nullptr, "AC_SELECT_ACTIVE without its ac_select_rows (x)");
  const ac_select_rows sel = *in;
  AC_REQUIRE(sel.sources_n >= 1, "sources_n (%d) below 1", (int)sel.sources_n);
  AC_REQUIRE(sel.n >= 0 && sel.n <= sel.sources_n, "n (%d) outside [0, sources_n = %d]", (int)sel.n, (int)sel.sources_n);
  AC_REQUIRE(sel.release >= 0.f && sel.release <= 1.f, "release (%g) outside [0, 1]", (double)sel.release);   // (NaN fails both)
  AC_REQUIRE(sel.gate >= 0.f, "gate (%g) is negative or NaN", (double)sel.gate);
  AC_REQUIRE((sel.energy != nullptr && active != nullptr) || B == 0 || C == 0, "AC_SELECT_ACTIVE: energy or the output (out0) is NULL");
  if (sel.sources_n > AC_SELECT_MAX_SOURCES) {
    set_error("AC_SELECT_ACTIVE: %d sources, the kernel ranks at most AC_SELECT_MAX_SOURCES = %d (a lane of a wave each): rank them "
              "frame by frame by the rules of the header", (int)sel.sources_n, AC_SELECT_MAX_SOURCES);
    return AC_EUNSUPPORTED;
  }
  if (B == 0 || C == 0) return AC_OK;
  AC_REQUIRE_ALIGNED(sel.energy, sel.state);
  DeviceGuard guard(psy->device);
  return launch_select(sel.energy, sel.valid, active, sel.state, sel.sources_n, B, K + 1, C, sel.n, sel.release, sel.gate,
                       (hipStream_t)stream);
}

int ac_protect_launches(const ac_psy_plan* psy, int C, int red_bits) {
  if (!psy || C < 1 || !psy->row_bits || red_bits < 5 * psy->M) return 0;
  if (protect_fuses(psy, red_bits)) return 1;
  // the composition: a transrate at each budget (the copies into the slots are the caller's)
  const bool one = transrate_fuses(psy);
  return (one ? 1 : 3) + (one && red_bits <= kPackRowsMaxBits ? 1 : 3);
}

// of one chunk of a stream (k_protect_ps): served exactly where the one-shot call is
int ac_protect_chunk_launches(const ac_psy_plan* psy, int C, int red_bits) { return ac_protect_launches(psy, C, red_bits); }

// ac_encode_fused_ex with AC_IN_PACKED | AC_EMIT_PACKED | AC_EMIT_REDUNDANT: rows [B,K+1,C] of `in` to the protected slots of
// `out`; with AC_EMIT_CARRY the rows are one chunk of a stream and out1 its ac_protect_carry
static int protect_packed_rows(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const ac_packed_rows* in, const float* X,
                               const float* t, const float* thr, const ac_protected_out* out, const void* out1, bool chunk,
                               int B, int K, int C, void* stream) {
  int st = check_plan_pair(mdct, psy);
  if (!st) st = check_dims(B, K, C);
  if (!st) st = check_quant(psy, B, K + 1, C);
  if (st) return st;
  AC_REQUIRE(psy->row_bits != 0, "AC_EMIT_REDUNDANT needs a plan with a row budget (ac_psy_plan_with_row_budget)");
  AC_REQUIRE(X == nullptr && t == nullptr && thr == nullptr && (chunk || out1 == nullptr),
             "AC_EMIT_REDUNDANT writes no X, t or thr and takes no out1: they must be NULL");
  ac_protect_carry pc = {};
  if (chunk) {
    AC_REQUIRE(out1 != nullptr, "AC_EMIT_CARRY without its ac_protect_carry (out1)");
    pc = *static_cast<const ac_protect_carry*>(out1);
    AC_REQUIRE(pc.row_out != nullptr && pc.fits_out != nullptr && pc.offset_out != nullptr, "ac_protect_carry: a NULL output");
    AC_REQUIRE(pc.row_in == nullptr || (pc.fits_in != nullptr && pc.offset_in != nullptr), "ac_protect_carry: row_in without fits_in, offset_in");
    AC_REQUIRE(pc.row_in != pc.row_out && pc.fits_in != pc.fits_out && pc.offset_in != pc.offset_out,
               "ac_protect_carry: in and out must be distinct buffers (the carry is double buffered)");
    AC_REQUIRE_ALIGNED(pc.row_in, pc.row_out);
  }
  AC_REQUIRE(in != nullptr, "AC_EMIT_REDUNDANT without its ac_packed_rows (x)");
  AC_REQUIRE(out != nullptr, "AC_EMIT_REDUNDANT without its ac_protected_out (out0)");
  const ac_packed_rows rows = *in;
  const ac_protected_out po = *out;
  AC_REQUIRE(po.row_bytes == plan_row_bytes(psy), "row_bytes (%lld) is not the plan's ceil(%d / 32) * 4 = %lld",
             (long long)po.row_bytes, psy->row_bits, (long long)plan_row_bytes(psy));
  AC_REQUIRE(po.red_bits >= 5 * psy->M, "red_bits (%d) below 5 * bark_bands_n = %d, the length of a row that stores no band",
             (int)po.red_bits, 5 * psy->M);
  AC_REQUIRE(rows.nbytes >= 0, "negative nbytes (%lld)", (long long)rows.nbytes);
  if (B == 0 || C == 0) return AC_OK;
  if (!protect_fuses(psy, po.red_bits)) {
    set_error("AC_EMIT_REDUNDANT: no kernel protects packed rows in one launch for filters_n = %d, bark_bands_n = %d, row budget "
              "%d, redundant budget %d here (ac_protect_launches() != 1): use the composition -- the AC_IN_PACKED | AC_EMIT_PACKED "
              "call at each budget, then copies into the two parts of every slot of zero-filled data", psy->N, psy->M,
              psy->row_bits, (int)po.red_bits);
    return AC_EUNSUPPORTED;
  }
  st = check_packed_rows(rows, true, po.data != nullptr && po.fits != nullptr && po.red_fits != nullptr);
  if (st) return st;
  AC_REQUIRE_ALIGNED(po.data, po.offset, po.red_offset);
  DeviceGuard guard(psy->device);
  if (chunk)
    return launch_protect_stream(psy, rows.data, rows.nbytes, rows.index, po.data, po.row_bytes, po.red_bits, po.fits, po.red_fits,
                                 po.offset, po.red_offset, pc.row_in, pc.fits_in, pc.offset_in, pc.row_out, pc.fits_out,
                                 pc.offset_out, B, K + 1, C, (hipStream_t)stream);
  return launch_protect(psy, rows.data, rows.nbytes, rows.index, po.data, po.row_bytes, po.red_bits, po.fits, po.red_fits, po.offset,
                        po.red_offset, B, K + 1, C, (hipStream_t)stream);
}

int ac_encode_fused_ex(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const float* x, float* X, float* t, float* thr,
                       float drown, int flags, void* noisy_v, void* db_norm_v, uint64_t seed, int B, int K, int C,
                       void* stream) {
  AC_REQUIRE((flags & ~(AC_EMIT_NOISY | AC_EMIT_DB_NORM | AC_EMIT_CODES | AC_EMIT_PACKED | AC_IN_PCM16 | AC_IN_PACKED |
                        AC_EMIT_REDUNDANT | AC_EMIT_CARRY | AC_IN_MIX | AC_IN_ROUTE | AC_EMIT_LEVEL | AC_SELECT_ACTIVE)) == 0,
             "unknown flags %#x", flags);
  if (flags & AC_SELECT_ACTIVE) {
    AC_REQUIRE(flags == AC_SELECT_ACTIVE, "AC_SELECT_ACTIVE goes alone (got %#x): levels are ranked into an active mask", flags);
    return select_active(mdct, psy, reinterpret_cast<const ac_select_rows*>(x), X, t, thr, static_cast<uint8_t*>(noisy_v), db_norm_v,
                         B, K, C, stream);
  }
  if (flags & AC_EMIT_LEVEL) {
    AC_REQUIRE(flags == (AC_IN_PACKED | AC_EMIT_LEVEL),
               "AC_EMIT_LEVEL goes with AC_IN_PACKED alone (got %#x): the level of packed rows is taken", flags);
    return level_packed_rows(mdct, psy, reinterpret_cast<const ac_packed_rows*>(x), X, t, thr, static_cast<float*>(noisy_v),
                             static_cast<uint8_t*>(db_norm_v), B, K, C, stream);
  }
  if (flags & AC_IN_ROUTE) {
    AC_REQUIRE(flags == (AC_IN_PACKED | AC_EMIT_PACKED | AC_IN_ROUTE),
               "AC_IN_ROUTE goes with AC_IN_PACKED | AC_EMIT_PACKED alone (got %#x): the packed rows of several sources are routed to "
               "several mixes", flags);
    return route_packed_rows(mdct, psy, reinterpret_cast<const ac_route_rows*>(x), X, t, thr,
                             static_cast<const ac_packed_out*>(noisy_v), static_cast<int16_t*>(db_norm_v), B, K, C, stream);
  }
  if (flags & AC_IN_MIX) {
    AC_REQUIRE(flags == (AC_IN_PACKED | AC_EMIT_PACKED | AC_IN_MIX),
               "AC_IN_MIX goes with AC_IN_PACKED | AC_EMIT_PACKED alone (got %#x): the packed rows of several sources are mixed", flags);
    return mix_packed_rows(mdct, psy, reinterpret_cast<const ac_mix_rows*>(x), X, t, thr, static_cast<const ac_packed_out*>(noisy_v),
                           static_cast<int16_t*>(db_norm_v), B, K, C, stream);
  }
  if (flags & (AC_EMIT_REDUNDANT | AC_EMIT_CARRY)) {
    AC_REQUIRE((flags & ~AC_EMIT_CARRY) == (AC_IN_PACKED | AC_EMIT_PACKED | AC_EMIT_REDUNDANT),
               "AC_EMIT_REDUNDANT goes with AC_IN_PACKED | AC_EMIT_PACKED alone, AC_EMIT_CARRY beside the three (got %#x): packed "
               "rows are protected", flags);
    return protect_packed_rows(mdct, psy, reinterpret_cast<const ac_packed_rows*>(x), X, t, thr,
                               static_cast<const ac_protected_out*>(noisy_v), db_norm_v, (flags & AC_EMIT_CARRY) != 0, B, K, C, stream);
  }
  if (flags & AC_IN_PACKED) {
    AC_REQUIRE(flags == (AC_IN_PACKED | AC_EMIT_PACKED),
               "AC_IN_PACKED goes with AC_EMIT_PACKED alone (got %#x): packed rows are transrated to packed rows", flags);
    return transrate_packed_rows(mdct, psy, reinterpret_cast<const ac_packed_rows*>(x), X, t, thr,
                                 static_cast<const ac_packed_out*>(noisy_v), static_cast<int16_t*>(db_norm_v), B, K, C, stream);
  }
  // AC_IN_PCM16: x is int16, under AC_EMIT_CODES or AC_EMIT_PACKED only
  const bool pcm16 = (flags & AC_IN_PCM16) != 0;
  const int emit = flags & ~AC_IN_PCM16;
  AC_REQUIRE(!pcm16 || emit == AC_EMIT_CODES || emit == AC_EMIT_PACKED,
             "AC_IN_PCM16 goes with AC_EMIT_CODES or AC_EMIT_PACKED alone (got %#x): the encode of 16-bit PCM to X, t and thr is "
             "ac_encode_fused_pcm16", flags);
  if (emit & AC_EMIT_PACKED) {
    AC_REQUIRE(emit == AC_EMIT_PACKED, "AC_EMIT_PACKED excludes the other output flags (got %#x)", flags);
    return encode_packed_rows(mdct, psy, x, pcm16, X, t, thr, drown, static_cast<const ac_packed_out*>(noisy_v), db_norm_v, B, K,
                              C, stream);
  }
  if (emit & AC_EMIT_CODES) {
    AC_REQUIRE(emit == AC_EMIT_CODES, "AC_EMIT_CODES excludes the other output flags (got %#x)", flags);
    return encode_quantized(mdct, psy, x, pcm16, X, t, thr, drown, static_cast<int16_t*>(noisy_v), static_cast<int8_t*>(db_norm_v),
                            B, K, C, stream);
  }
  float* noisy = static_cast<float*>(noisy_v);
  float* db_norm = static_cast<float*>(db_norm_v);
  AC_REQUIRE(!(flags & AC_EMIT_NOISY) || noisy != nullptr || B == 0 || C == 0, "AC_EMIT_NOISY without an output tensor");
  AC_REQUIRE(!(flags & AC_EMIT_DB_NORM) || db_norm != nullptr || B == 0 || C == 0, "AC_EMIT_DB_NORM without an output tensor");
  float* o_noisy = (flags & AC_EMIT_NOISY) ? noisy : nullptr;
  float* o_dbn = (flags & AC_EMIT_DB_NORM) ? db_norm : nullptr;
  if (!o_noisy && !o_dbn) return encode_fused(mdct, psy, x, false, X, t, thr, drown, B, K, C, stream);
  int st = check_plan_pair(mdct, psy);
  if (!st) st = check_dims(B, K, C);
  if (st) return st;
  if (B == 0 || C == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && t != nullptr && thr != nullptr && (x != nullptr || K == 0), "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(x, X, thr, o_noisy, o_dbn);
  if (mdct->fast && psy->fast && !g_force_generic && fast_epilogue_supported(mdct, psy, 0, C)) {
    DeviceGuard guard(mdct->device);
    return launch_fwd_fast(mdct, psy, x, 0, X, t, thr, drown, nullptr, B, K, K + 1, C, (hipStream_t)stream, nullptr, o_noisy,
                           o_dbn, seed);
  }
  // elsewhere: the encode, then the two element-wise kernels over X (same values as the fused epilogue)
  st = encode_fused(mdct, psy, x, false, X, t, thr, drown, B, K, C, stream);
  const size_t n = (size_t)B * (size_t)(K + 1) * (size_t)mdct->N * (size_t)C;
  if (!st && o_noisy) st = ac_add_noise(X, thr, o_noisy, n, seed, stream);
  if (!st && o_dbn) st = ac_amplitude_to_db(X, o_dbn, n, 1, stream);
  return st;
}

int ac_encode_fused_pcm16(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const int16_t* x, float* X, float* t,
                          float* thr, float drown, int B, int K, int C, void* stream) {
  return encode_fused(mdct, psy, x, true, X, t, thr, drown, B, K, C, stream);
}

// ---- buffer placement probe ---------------------------------------------------------------------
int ac_probe_placement(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const float* x, float* X, float* t,
                       float* const* thr_candidates, int n_candidates, int B, int K, int C, void* stream, int* best,
                       float* ms) {
  AC_REQUIRE(mdct != nullptr && psy != nullptr, "plan is NULL");
  AC_REQUIRE(thr_candidates != nullptr && n_candidates >= 1 && best != nullptr, "no candidates");
  for (int j = 0; j < n_candidates; ++j) AC_REQUIRE(thr_candidates[j] != nullptr, "candidate %d is NULL", j);
  DeviceGuard guard(mdct->device);
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t e0, e1;
  AC_HIP_CHECK(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    set_error("hipEventCreate failed in ac_probe_placement");
    return AC_EHIP;
  }
  int st = AC_OK, arg = 0;
  float best_ms = 0.f;
  for (int j = 0; j < n_candidates && !st; ++j) {
    float med[3];
    st = ac_encode_fused(mdct, psy, x, X, t, thr_candidates[j], 0.f, B, K, C, stream);   // warm-up
    for (int r = 0; r < 3 && !st; ++r) {
      if (hipEventRecord(e0, s) != hipSuccess) st = AC_EHIP;
      if (!st) st = ac_encode_fused(mdct, psy, x, X, t, thr_candidates[j], 0.f, B, K, C, stream);
      if (!st && (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                  hipEventElapsedTime(&med[r], e0, e1) != hipSuccess))
        st = AC_EHIP;
    }
    if (st) break;
    std::sort(med, med + 3);
    if (ms) ms[j] = med[1];
    if (j == 0 || med[1] < best_ms) {
      best_ms = med[1];
      arg = j;
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st == AC_EHIP) set_error("HIP event call failed in ac_probe_placement");
  if (!st) *best = arg;
  return st;
}

int ac_encode_fused_typed(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const void* x, void* X, void* t, void* thr,
                          double drown, int dtype, int B, int K, int C, void* stream) {
  AC_REQUIRE_DTYPE(dtype);
  if (dtype == AC_F32)
    return ac_encode_fused(mdct, psy, static_cast<const float*>(x), static_cast<float*>(X), static_cast<float*>(t),
                           static_cast<float*>(thr), (float)drown, B, K, C, stream);
  int st = check_plan_pair(mdct, psy);
  if (!st) st = check_dims(B, K, C);
  if (st) return st;
  if (B == 0 || C == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && t != nullptr && thr != nullptr && (x != nullptr || K == 0), "NULL tensor pointer");
  // bfloat16 tensors, stereo / mono, both plans wave-level: one fused launch (mono at filters_n = 2048 excepted, as in
  // encode_fused); otherwise the three typed entry points in sequence
  if (dtype == AC_BF16 && mdct->fast && psy->fast && !g_force_generic && C <= 2 &&
      !fused_encode_takes_two_launches(mdct->N, C, 2)) {
    DeviceGuard guard(mdct->device);
    return launch_fwd_fast(mdct, psy, x, 2, static_cast<float*>(X), static_cast<float*>(t), static_cast<float*>(thr),
                           (float)drown, nullptr, B, K, K + 1, C, (hipStream_t)stream);
  }
  st = ac_mdct_forward_typed(mdct, x, X, dtype, B, K, C, stream);
  if (!st) st = ac_tonality_typed(psy, X, t, dtype, B, K + 1, C, stream);
  if (!st) st = ac_mask_threshold_typed(psy, X, t, drown, thr, dtype, B, K + 1, C, stream);
  return st;
}

}  // extern "C"
