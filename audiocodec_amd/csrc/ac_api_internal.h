// What the units of the C ABI (ac_api*.hip) share: argument checks, the predicates that say which kernels take a call, and the
// rules that several entry points must state alike.  Each is defined once, in the unit named above it.
#pragma once
#include <new>

#include "ac_internal.h"

#define AC_REQUIRE_PRE(d) AC_REQUIRE((d) == AC_F32 || (d) == AC_F64, "precompute = %d is not AC_F32 or AC_F64", (d))
#define AC_REQUIRE_DTYPE(d) AC_REQUIRE((d) == AC_F32 || (d) == AC_F64 || (d) == AC_BF16, "dtype = %d is not one of AC_F32, AC_F64, AC_BF16", (d))
// the filter bank also takes float16 tensors (mdctransformer.py:327-344); the masking model does not (psychoacoustic.py:42-43)
#define AC_REQUIRE_DTYPE_MDCT(d) AC_REQUIRE((d) == AC_F32 || (d) == AC_F64 || (d) == AC_BF16 || (d) == AC_F16, "dtype = %d is not one of AC_F32, AC_F64, AC_BF16, AC_F16", (d))

namespace ac {

// ---- ac_api.hip
inline bool valid_window(int w) { return w == AC_WINDOW_VORBIS || w == AC_WINDOW_SINE || w == AC_WINDOW_RECT; }
bool env_is_1(const char* name);   // the *_NOFUSE hooks: whether the variable is set to 1, read per call
template <typename T>
T* new_or_error() {   // a value-initialised T for a creation call, or NULL with the error set (the caller returns AC_ENOMEM)
  T* p = new (std::nothrow) T();
  if (!p) set_error("out of host memory");
  return p;
}
// ---- ac_api_plan.hip
hipError_t creation_sync();   // the wait that ends every creation call (see its definition)
int creation_done();
// ---- ac_api_encode.hip
bool wave_level(const ac_mdct_plan* p, int C, int iof, int blocks);
bool psy_mid_serves(const ac_psy_plan* p, int C);
bool psy_fast_serves(const ac_psy_plan* p, int C);
int check_dims(int B, int K, int C);
int check_plan_pair(const ac_mdct_plan* mdct, const ac_psy_plan* psy);
// ... as a bool, for the *_launches queries (they answer 0 and set no error)
inline bool plans_match(const ac_mdct_plan* mdct, const ac_psy_plan* psy) {
  return mdct && psy && mdct->N == psy->N && mdct->device == psy->device;
}
int check_row_bytes(const ac_packed_out& po, const ac_psy_plan* psy);
int check_rows_to_rows(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const float* X, const float* t, const float* thr, int B,
                       int K, int C, const char* flag);
int mdct_inverse(const ac_mdct_plan* p, const float* X, void* x, bool pcm16, int B, int Kp, int C, void* stream);
// Where both plans are wave-level the encode is one fused launch, except at filters_n = 2048 for mono input and for 16-bit
// PCM with 3 or more channels, where the fused kernel would spill registers (7 / 4 at the 256 budget): there two wave-level
// launches, the second computing tonality and threshold in one pass over X.  iof as launch_fwd_fast takes it; the
// bfloat16 callers (iof = 2) serve C <= 2 only, so the PCM clause is inert for them.
inline bool fused_encode_takes_two_launches(int N, int C, int iof) { return N == 2048 && (C == 1 || (iof == 1 && C > 2)); }
bool encode_packed_fuses(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C);
// ---- ac_api_quant.hip
int check_quant(const ac_psy_plan* psy, int B, int F, int C);
int check_packed_rows(const ac_packed_rows& rows, bool need_index, bool others_given);
int quantize_of_plan(const ac_psy_plan* psy, const float* X, const float* thr, int16_t* codes, int8_t* sf, int B, int F, int C,
                     hipStream_t s);
bool decode_packed_fuses(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C);

}  // namespace ac
