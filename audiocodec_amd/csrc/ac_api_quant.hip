// C ABI, quantised side: the element-wise utilities, the quantiser and rate control, the synthesis from codes or packed rows,
// pack / unpack, and the compute_dtype variants of the entry points that are not encodes.
#include "ac_api_internal.h"

namespace ac {

int check_quant(const ac_psy_plan* psy, int B, int F, int C) {
  AC_REQUIRE(psy != nullptr, "plan is NULL");
  AC_REQUIRE(B >= 0 && F >= 0 && C >= 0, "negative dimension (B=%d, frames=%d, C=%d)", B, F, C);
  AC_REQUIRE(psy->N % 2 == 0, "the quantiser needs an even filter_bands_n (got %d)", psy->N);
  AC_REQUIRE(psy->d_qoff != nullptr && psy->d_qband != nullptr, "plan has no quantiser tables");
  return AC_OK;
}
// the quantiser of a plan: at the plan's row budget where it has one (no offset or row-bits tensor to fill), else k_quantize
int quantize_of_plan(const ac_psy_plan* psy, const float* X, const float* thr, int16_t* codes, int8_t* sf, int B, int F,
                     int C, hipStream_t s) {
  if (psy->row_bits)
    return launch_quantize_budget(psy, X, thr, psy->row_bits, nullptr, psy->kmin, codes, sf, nullptr, nullptr, B, F, C, s);
  return launch_quantize(psy, X, thr, codes, sf, B, F, C, s);
}
// What every reader of an ac_packed_rows asks of it, in the order they all report it.  need_index: false where there is no row
// to read.  others_given: the call's other tensors are there (one message covers them); their alignment follows at the call.
int check_packed_rows(const ac_packed_rows& rows, bool need_index, bool others_given) {
  AC_REQUIRE(rows.nbytes >= 0, "negative nbytes (%lld)", (long long)rows.nbytes);
  AC_REQUIRE((rows.index != nullptr || !need_index) && others_given, "NULL tensor pointer");
  AC_REQUIRE(rows.data != nullptr || rows.nbytes == 0, "data is NULL");
  AC_REQUIRE_ALIGNED(rows.data, rows.index);
  return AC_OK;
}

static bool decode_quantized_fuses(const ac_mdct_plan* mdct, int C) {
  return !g_force_generic && wave_level(mdct, C, 0, 1) && fast_inv_quant_serves(mdct, C);
}
// whether packed rows are decoded in one launch (k_inv_fast_p); AC_DECODE_PACKED_NOFUSE=1 sends every configuration down
// ac_unpack + ac_decode_quantized (read per call, as the hooks of ac_api_encode.hip)
bool decode_packed_fuses(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C) {
  if (env_is_1("AC_DECODE_PACKED_NOFUSE")) return false;
  return decode_quantized_fuses(mdct, C) && fast_inv_packed_serves(mdct, psy, C);
}

}  // namespace ac

using namespace ac;

extern "C" {

// ---- element-wise utilities ------------------------------------------------------------------------

int ac_amplitude_to_db(const float* a, float* out, size_t n, int norm, void* stream) {
  AC_REQUIRE(n == 0 || (a != nullptr && out != nullptr), "NULL tensor pointer");
  return launch_db_typed(a, out, n, norm, AC_F32, (hipStream_t)stream);
}

int ac_amplitude_to_db_backward(const float* a, const float* grad_out, float* grad_a, size_t n, int norm, void* stream) {
  AC_REQUIRE(n == 0 || (a != nullptr && grad_out != nullptr && grad_a != nullptr), "NULL tensor pointer");
  return launch_db_bwd(a, grad_out, grad_a, n, norm, (hipStream_t)stream);
}

int ac_add_noise(const float* X, const float* thr, float* out, size_t n, uint64_t seed, void* stream) {
  AC_REQUIRE(n == 0 || (thr != nullptr && out != nullptr), "NULL tensor pointer");   // X == NULL: zeros
  return launch_add_noise_typed(X, thr, out, n, seed, AC_F32, (hipStream_t)stream);
}

// ---- quantiser (ac_quant.hip) -----------------------------------------------

int ac_quantize(const ac_psy_plan* psy, const float* X, const float* thr, int16_t* codes, int8_t* sf, int B, int F, int C,
                void* stream) {
  int st = check_quant(psy, B, F, C);
  if (st) return st;
  if (B == 0 || F == 0 || C == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && thr != nullptr && codes != nullptr && sf != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(X, thr, codes, sf);
  DeviceGuard guard(psy->device);
  return quantize_of_plan(psy, X, thr, codes, sf, B, F, C, (hipStream_t)stream);
}

int ac_dequantize(const ac_psy_plan* psy, const int16_t* codes, const int8_t* sf, float* X, int B, int F, int C, void* stream) {
  int st = check_quant(psy, B, F, C);
  if (st) return st;
  if (B == 0 || F == 0 || C == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && codes != nullptr && sf != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(X, codes, sf);
  DeviceGuard guard(psy->device);
  return launch_dequantize(psy, codes, sf, X, B, F, C, (hipStream_t)stream);
}

int ac_quantize_budget(const ac_psy_plan* psy, const float* X, const float* thr, int row_bits, const int32_t* row_bits_per_row,
                       int kmin, int16_t* codes, int8_t* sf, int16_t* offset, int32_t* row_bits_out, int B, int F, int C,
                       void* stream) {
  int st = check_quant(psy, B, F, C);
  if (st) return st;
  AC_REQUIRE(kmin >= -254 && kmin <= 254, "kmin (%d) outside [-254, 254]", kmin);
  AC_REQUIRE(row_bits_per_row != nullptr || row_bits >= 5 * psy->M,
             "row_bits (%d) below 5 * bark_bands_n = %d, the length of a row that stores no band", row_bits, 5 * psy->M);
  if (thr == nullptr && X != nullptr) {   // X addresses one ac_quantized_rows: the requantiser
    AC_REQUIRE(kmin >= 0, "kmin (%d) outside [0, 254]: thr is NULL (requantising), and an offset below 0 cannot restore what "
               "the first quantiser dropped", kmin);
    if (B == 0 || F == 0 || C == 0) return AC_OK;
    const ac_quantized_rows in = *reinterpret_cast<const ac_quantized_rows*>(X);
    AC_REQUIRE(in.codes != nullptr && in.sf != nullptr && codes != nullptr && sf != nullptr && offset != nullptr,
               "NULL tensor pointer");
    AC_REQUIRE_ALIGNED(in.codes, in.sf, codes, sf, offset, row_bits_per_row, row_bits_out);
    DeviceGuard guard(psy->device);
    return launch_requantize_budget(psy, in.codes, in.sf, row_bits, row_bits_per_row, kmin, codes, sf, offset, row_bits_out, B,
                                    F, C, (hipStream_t)stream);
  }
  if (B == 0 || F == 0 || C == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && thr != nullptr && codes != nullptr && sf != nullptr && offset != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(X, thr, codes, sf, offset, row_bits_per_row, row_bits_out);
  DeviceGuard guard(psy->device);
  return launch_quantize_budget(psy, X, thr, row_bits, row_bits_per_row, kmin, codes, sf, offset, row_bits_out, B, F, C,
                                (hipStream_t)stream);
}

size_t ac_clip_budget_scratch_bytes(const ac_psy_plan* psy, int B, int F, int C) {
  if (psy == nullptr || B <= 0 || F <= 0 || C <= 0) return 0;
  return clip_budget_scratch_bytes(psy, B, (long long)F * C);
}

int ac_quantize_clip_budget(const ac_psy_plan* psy, const float* X, const float* thr, int64_t clip_bits,
                            const int64_t* clip_bits_per_clip, int kmin, int16_t* codes, int8_t* sf, int16_t* offset,
                            int32_t* row_bits_out, int16_t* clip_offset, int64_t* clip_bits_out, void* scratch, int B, int F,
                            int C, void* stream) {
  int st = check_quant(psy, B, F, C);
  if (st) return st;
  AC_REQUIRE(kmin >= -254 && kmin <= 254, "kmin (%d) outside [-254, 254]", kmin);
  const long long floor_bits = (long long)F * C * 32 * ((5 * psy->M + 31) / 32);
  AC_REQUIRE(clip_bits_per_clip != nullptr || clip_bits >= floor_bits,
             "clip_bits (%lld) below frames * C * 32 * ceil(5 * bark_bands_n / 32) = %lld, the length of a clip that stores "
             "no band", (long long)clip_bits, floor_bits);
  if (B == 0 || F == 0 || C == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && thr != nullptr && codes != nullptr && sf != nullptr && offset != nullptr, "NULL tensor pointer");
  AC_REQUIRE(scratch != nullptr, "scratch of ac_clip_budget_scratch_bytes() = %zu bytes is required",
             ac_clip_budget_scratch_bytes(psy, B, F, C));
  AC_REQUIRE_ALIGNED(X, thr, codes, sf, offset, clip_bits_per_clip, row_bits_out, clip_offset, clip_bits_out, scratch);
  DeviceGuard guard(psy->device);
  return launch_quantize_clip_budget(psy, X, thr, clip_bits, clip_bits_per_clip, kmin, codes, sf, offset, row_bits_out,
                                     clip_offset, clip_bits_out, scratch, B, F, C, (hipStream_t)stream);
}

int ac_decode_quantized_launches(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C) {
  if (!plans_match(mdct, psy) || C < 1) return 0;
  return decode_quantized_fuses(mdct, C) ? 1 : 2;
}

int ac_decode_packed_launches(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C) {
  if (!plans_match(mdct, psy) || C < 1) return 0;
  return decode_packed_fuses(mdct, psy, C) ? 1 : 1 + ac_decode_quantized_launches(mdct, psy, C);
}

int ac_decode_quantized(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const int16_t* codes, const int8_t* sf, float* x,
                        int16_t* pcm16, float* scratch, int B, int Kp, int C, void* stream) {
  int st = check_plan_pair(mdct, psy);
  if (!st) st = check_quant(psy, B, Kp, C);
  if (st) return st;
  AC_REQUIRE((x != nullptr) != (pcm16 != nullptr), "exactly one of x (float32) and pcm16 must be given");
  if (B == 0 || C == 0) return AC_OK;
  void* out = x ? static_cast<void*>(x) : static_cast<void*>(pcm16);
  if (sf == nullptr && codes != nullptr) {   // codes addresses one ac_packed_rows: the rows of the packed bitstream
    const ac_packed_rows rows = *reinterpret_cast<const ac_packed_rows*>(codes);
    if (!decode_packed_fuses(mdct, psy, C)) {
      set_error("sf is NULL (packed rows), and no kernel decodes packed rows in one launch for filters_n = %d, bark_bands_n "
                "= %d, %d channels here (ac_decode_packed_launches() != 1): unpack them with ac_unpack and pass codes and sf",
                mdct->N, psy->M, C);
      return AC_EUNSUPPORTED;
    }
    st = check_packed_rows(rows, Kp != 0, true);
    if (st) return st;
    AC_REQUIRE_ALIGNED(out);
    // scratch addresses one ac_conceal: rows that did not arrive are concealed
    const uint8_t* lost = nullptr;
    int max_age = 0;
    int64_t redundant_at = 0;   // nonzero: a lost row whose successor arrived is recovered
    if (scratch != nullptr) {
      const ac_conceal cl = *reinterpret_cast<const ac_conceal*>(scratch);
      max_age = cl.max_age;
      // AC_CONCEAL_REDUNDANT in a max_age that is not negative: scratch addresses the longer ac_conceal_redundant
      if (max_age >= 0 && (max_age & AC_CONCEAL_REDUNDANT)) {
        redundant_at = reinterpret_cast<const ac_conceal_redundant*>(scratch)->redundant_at;
        max_age &= ~AC_CONCEAL_REDUNDANT;
        AC_REQUIRE(redundant_at >= 1 && redundant_at <= 2147483647ll, "redundant_at (%lld) outside [1, 2^31)",
                   (long long)redundant_at);
        AC_REQUIRE(cl.lost != nullptr, "AC_CONCEAL_REDUNDANT without lost");
      }
      AC_REQUIRE(max_age >= 0 && max_age <= AC_CONCEAL_MAX_AGE, "max_age (%d) outside [0, %d]", max_age, AC_CONCEAL_MAX_AGE);
      lost = cl.lost;
    }
    DeviceGuard guard(mdct->device);
    if (Kp >= 1 && lost != nullptr && redundant_at != 0)
      return launch_inv_fast_packed_recover(mdct, psy, rows.data, rows.nbytes, rows.index, lost, max_age, redundant_at, out,
                                            pcm16 != nullptr, B, Kp, C, (hipStream_t)stream);
    if (Kp >= 1 && lost != nullptr)
      return launch_inv_fast_packed_conceal(mdct, psy, rows.data, rows.nbytes, rows.index, lost, max_age, out, pcm16 != nullptr,
                                            B, Kp, C, (hipStream_t)stream);
    if (Kp >= 1)
      return launch_inv_fast_packed(mdct, psy, rows.data, rows.nbytes, rows.index, out, pcm16 != nullptr, nullptr, nullptr, B, Kp,
                                    Kp + 1, C, (hipStream_t)stream);
    return mdct_inverse(mdct, nullptr, out, pcm16 != nullptr, B, Kp, C, stream);
  }
  AC_REQUIRE(Kp == 0 || (codes != nullptr && sf != nullptr), "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(codes, sf, out);
  DeviceGuard guard(mdct->device);
  hipStream_t s = (hipStream_t)stream;
  if (Kp >= 1 && decode_quantized_fuses(mdct, C))
    return launch_inv_fast_quant(mdct, psy, codes, sf, out, pcm16 != nullptr, B, Kp, C, s);
  AC_REQUIRE(Kp == 0 || scratch != nullptr,
             "scratch [B, Kp, N, C] float32 is required where ac_decode_quantized_launches() returns 2");
  AC_REQUIRE_ALIGNED(scratch);
  if (Kp >= 1) {
    st = launch_dequantize(psy, codes, sf, scratch, B, Kp, C, s);
    if (st) return st;
  }
  return mdct_inverse(mdct, scratch, out, pcm16 != nullptr, B, Kp, C, stream);
}

// ---- packed bitstream (ac_pack.hip) ----------------------------------------

size_t ac_pack_scratch_bytes(int B, int F, int C) {
  if (B <= 0 || F <= 0 || C <= 0) return 0;
  return pack_scratch_bytes((long long)B * F * C);
}

int ac_pack_index(const ac_psy_plan* psy, const int16_t* codes, const int8_t* sf, int64_t* index, int64_t* total, void* scratch,
                  int B, int F, int C, void* stream) {
  int st = check_quant(psy, B, F, C);
  if (st) return st;
  AC_REQUIRE(total != nullptr, "total is NULL");
  DeviceGuard guard(psy->device);
  if (B == 0 || F == 0 || C == 0) {
    AC_HIP_CHECK(hipMemsetAsync(total, 0, sizeof(int64_t), (hipStream_t)stream));
    return AC_OK;
  }
  AC_REQUIRE(codes != nullptr && sf != nullptr && index != nullptr, "NULL tensor pointer");
  AC_REQUIRE(scratch != nullptr || ac_pack_scratch_bytes(B, F, C) == 0,
             "scratch of ac_pack_scratch_bytes() = %zu bytes is required", ac_pack_scratch_bytes(B, F, C));
  AC_REQUIRE_ALIGNED(codes, sf, index, total, scratch);
  return launch_pack_index(psy, codes, sf, index, total, scratch, B, F, C, (hipStream_t)stream);
}

int ac_pack(const ac_psy_plan* psy, const int16_t* codes, const int8_t* sf, const int64_t* index, uint8_t* data, int B, int F,
            int C, void* stream) {
  int st = check_quant(psy, B, F, C);
  if (st) return st;
  if (B == 0 || F == 0 || C == 0) return AC_OK;
  AC_REQUIRE(codes != nullptr && sf != nullptr && index != nullptr && data != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(codes, sf, index, data);
  DeviceGuard guard(psy->device);
  return launch_pack(psy, codes, sf, index, data, B, F, C, (hipStream_t)stream);
}

int ac_unpack(const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes, const int64_t* index, int16_t* codes, int8_t* sf,
              int B, int F, int C, void* stream) {
  int st = check_quant(psy, B, F, C);
  if (st) return st;
  AC_REQUIRE(nbytes >= 0, "negative nbytes (%lld)", (long long)nbytes);
  if (B == 0 || F == 0 || C == 0) return AC_OK;
  AC_REQUIRE(index != nullptr && codes != nullptr && sf != nullptr, "NULL tensor pointer");
  AC_REQUIRE(data != nullptr || nbytes == 0, "data is NULL");
  AC_REQUIRE_ALIGNED(data, index, codes, sf);
  DeviceGuard guard(psy->device);
  return launch_unpack(psy, data, nbytes, index, codes, sf, B, F, C, (hipStream_t)stream);
}

// ---- compute_dtype variants ---------------------------------------------------------------------

int ac_mdct_forward_typed(const ac_mdct_plan* p, const void* x, void* X, int dtype, int B, int K, int C, void* stream) {
  AC_REQUIRE_DTYPE_MDCT(dtype);
  if (dtype == AC_F32) return ac_mdct_forward(p, static_cast<const float*>(x), static_cast<float*>(X), B, K, C, stream);
  AC_REQUIRE(p != nullptr, "plan is NULL");
  int st = check_dims(B, K, C);
  if (st) return st;
  if (B == 0 || C == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && (x != nullptr || K == 0), "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(x, X);
  DeviceGuard guard(p->device);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AC_BF16 && wave_level(p, C, 2, K) && C <= 2)   // bfloat16 on the wave-level kernels (stereo / mono)
    return launch_fwd_fast(p, nullptr, x, 2, static_cast<float*>(X), nullptr, nullptr, 0.f, nullptr, B, K, K + 1, C, s);
  return launch_fwd_typed(p, x, X, nullptr, dtype, B, K, K + 1, C, s);
}

int ac_mdct_inverse_typed(const ac_mdct_plan* p, const void* X, void* x, int dtype, int B, int Kp, int C, void* stream) {
  AC_REQUIRE_DTYPE_MDCT(dtype);
  if (dtype == AC_F32) return ac_mdct_inverse(p, static_cast<const float*>(X), static_cast<float*>(x), B, Kp, C, stream);
  AC_REQUIRE(p != nullptr, "plan is NULL");
  int st = check_dims(B, Kp, C);
  if (st) return st;
  if (B == 0 || C == 0) return AC_OK;
  AC_REQUIRE(x != nullptr && (X != nullptr || Kp == 0), "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(x, X);
  DeviceGuard guard(p->device);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AC_BF16 && wave_level(p, C, 2, Kp) && C <= 2)
    return launch_inv_fast(p, static_cast<const float*>(X), x, 2, nullptr, nullptr, B, Kp, Kp + 1, C, s);
  return launch_inv_typed(p, X, x, nullptr, nullptr, dtype, B, Kp, Kp + 1, C, s);
}

int ac_tonality_typed(const ac_psy_plan* p, const void* X, void* t, int dtype, int B, int F, int C, void* stream) {
  AC_REQUIRE_DTYPE(dtype);
  if (dtype == AC_F32) return ac_tonality(p, static_cast<const float*>(X), static_cast<float*>(t), B, F, C, stream);
  AC_REQUIRE(p != nullptr, "plan is NULL");
  int st = check_dims(B, F, C);
  if (st) return st;
  if (B == 0 || C == 0 || F == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && t != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(X);
  DeviceGuard guard(p->device);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AC_BF16 && p->fast && !g_force_generic && C <= 2)
    return launch_psy_fast(p, static_cast<const float*>(X), nullptr, static_cast<float*>(t), nullptr, 0.f, B, F, C, s, 2);
  return launch_tonality_typed(p, X, t, dtype, B, F, C, s);
}

int ac_mask_threshold_typed(const ac_psy_plan* p, const void* X, const void* t, double drown, void* thr, int dtype, int B,
                            int F, int C, void* stream) {
  AC_REQUIRE_DTYPE(dtype);
  if (dtype == AC_F32)
    return ac_mask_threshold(p, static_cast<const float*>(X), static_cast<const float*>(t), (float)drown,
                             static_cast<float*>(thr), B, F, C, stream);
  AC_REQUIRE(p != nullptr, "plan is NULL");
  int st = check_dims(B, F, C);
  if (st) return st;
  if (B == 0 || C == 0 || F == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && t != nullptr && thr != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(X, thr);
  DeviceGuard guard(p->device);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AC_BF16 && p->fast && !g_force_generic && C <= 2)
    return launch_psy_fast(p, static_cast<const float*>(X), static_cast<const float*>(t), nullptr, static_cast<float*>(thr),
                           (float)drown, B, F, C, s, 2);
  return launch_threshold_typed(p, X, t, drown, thr, dtype, B, F, C, s);
}

int ac_amplitude_to_db_typed(const void* a, void* out, size_t n, int norm, int dtype, void* stream) {
  AC_REQUIRE_DTYPE(dtype);
  if (dtype == AC_F32) return ac_amplitude_to_db(static_cast<const float*>(a), static_cast<float*>(out), n, norm, stream);
  AC_REQUIRE(n == 0 || (a != nullptr && out != nullptr), "NULL tensor pointer");
  return launch_db_typed(a, out, n, norm, dtype, (hipStream_t)stream);
}

int ac_tonality_backward_typed(const ac_psy_plan* p, const void* X, const void* grad_t, void* grad_X, int dtype, int B, int F, int C,
                               void* stream) {
  AC_REQUIRE_DTYPE(dtype);
  if (dtype == AC_F32)
    return ac_tonality_backward(p, static_cast<const float*>(X), static_cast<const float*>(grad_t), static_cast<float*>(grad_X), 0, B, F, C, stream);
  AC_REQUIRE(p != nullptr, "plan is NULL");
  int st = check_dims(B, F, C);
  if (st) return st;
  if (B == 0 || C == 0 || F == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && grad_t != nullptr && grad_X != nullptr, "NULL tensor pointer");
  DeviceGuard guard(p->device);
  return launch_tonality_bwd_typed(p, X, grad_t, grad_X, 0, dtype, B, F, C, (hipStream_t)stream);
}

int ac_mask_threshold_backward_typed(const ac_psy_plan* p, const void* X, const void* t, double drown, const void* grad_thr, void* grad_X,
                                     void* grad_t, int dtype, int B, int F, int C, void* stream) {
  AC_REQUIRE_DTYPE(dtype);
  if (dtype == AC_F32)
    return ac_mask_threshold_backward(p, static_cast<const float*>(X), static_cast<const float*>(t), (float)drown,
                                      static_cast<const float*>(grad_thr), static_cast<float*>(grad_X), static_cast<float*>(grad_t), B, F, C, stream);
  AC_REQUIRE(p != nullptr, "plan is NULL");
  int st = check_dims(B, F, C);
  if (st) return st;
  if (B == 0 || C == 0 || F == 0) return AC_OK;
  AC_REQUIRE(X != nullptr && t != nullptr && grad_thr != nullptr && grad_X != nullptr && grad_t != nullptr, "NULL tensor pointer");
  DeviceGuard guard(p->device);
  return launch_threshold_bwd_typed(p, X, t, drown, grad_thr, grad_X, grad_t, dtype, B, F, C, (hipStream_t)stream);
}

int ac_add_noise_typed(const void* X, const void* thr, void* out, size_t n, uint64_t seed, int dtype, void* stream) {
  AC_REQUIRE_DTYPE(dtype);
  if (dtype == AC_F32)
    return ac_add_noise(static_cast<const float*>(X), static_cast<const float*>(thr), static_cast<float*>(out), n, seed, stream);
  AC_REQUIRE(n == 0 || (X != nullptr && thr != nullptr && out != nullptr), "NULL tensor pointer");
  return launch_add_noise_typed(X, thr, out, n, seed, dtype, (hipStream_t)stream);
}

}  // extern "C"
