// What the units of the generic tiers share (ac_mdct_generic.hip, ac_psy_generic.hip, ac_elementwise.hip): the storage / compute
// type pair of their kernel templates with its loads and stores, the reference's functions in the compute type, and the one
// switch from an AC_* dtype to a C++ type.  gfx950 only.
#pragma once
#include <type_traits>

#include "ac_internal.h"

namespace ac {

static constexpr float kEps = 1e-14f;   // _INTENSITY_EPS, psychoacoustic.py:56

// ---- compute_dtype variants: the kernels of these units are templates over the storage type TIO of the
// tensors -- float (the primary path), double (everything in fp64, constants included: the on-device oracle), bfloat16 and,
// in the filter bank, float16 (storage only: arithmetic in float32).  TC = the type of the arithmetic, of the constant tables
// and of the streaming state.
template <typename TIO> struct Compute { using type = float; };
template <> struct Compute<double> { using type = double; };
__device__ __forceinline__ float ldv(const float* p) { return *p; }
__device__ __forceinline__ double ldv(const double* p) { return *p; }
__device__ __forceinline__ float ldv(const bf16_t* p) { return (float)*p; }
__device__ __forceinline__ float ldv(const f16_t* p) { return (float)*p; }
__device__ __forceinline__ void stv(float* p, float v) { *p = v; }
__device__ __forceinline__ void stv(double* p, double v) { *p = v; }
__device__ __forceinline__ void stv(bf16_t* p, float v) { *p = (bf16_t)v; }   // round to nearest even
__device__ __forceinline__ void stv(f16_t* p, float v) { *p = (f16_t)v; }     // round to nearest even (overflow: infinity, as a cast)

// the reference's functions in the compute type
__device__ __forceinline__ float m_log(float x) { return logf(x); }
__device__ __forceinline__ double m_log(double x) { return log(x); }
__device__ __forceinline__ float m_exp(float x) { return expf(x); }
__device__ __forceinline__ double m_exp(double x) { return exp(x); }
__device__ __forceinline__ float m_pow(float x, float y) { return powf(x, y); }
__device__ __forceinline__ double m_pow(double x, double y) { return pow(x, y); }
__device__ __forceinline__ float m_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double m_sqrt(double x) { return sqrt(x); }
// maximum / minimum as tf.maximum / tf.minimum (psychoacoustic.py:113-116, 205-208, 331): a NaN operand gives NaN (fmax / fmin
// would return the other operand and turn a poisoned frame into finite numbers)
__device__ __forceinline__ float m_max(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }
__device__ __forceinline__ double m_max(double a, double b) { return (a != a || b != b) ? a + b : fmax(a, b); }
__device__ __forceinline__ float m_min(float a, float b) { return (a != a || b != b) ? a + b : fminf(a, b); }
__device__ __forceinline__ double m_min(double a, double b) { return (a != a || b != b) ? a + b : fmin(a, b); }

// ---- the dtype switch: with_dtype<T0, T1, ...>(dtype, f) calls f(TypeTag<T>{}) for the type of the list that `dtype` names.
// The list is what a kernel family admits, and only its types are instantiated.  The C ABI has checked dtype against the same
// list (AC_REQUIRE_DTYPE / AC_REQUIRE_DTYPE_MDCT) before it gets here, so the last type takes what the others do not.
template <typename T> struct TypeTag { using type = T; };
template <typename T> struct DtypeOf;
template <> struct DtypeOf<float> { static constexpr int value = AC_F32; };
template <> struct DtypeOf<double> { static constexpr int value = AC_F64; };
template <> struct DtypeOf<bf16_t> { static constexpr int value = AC_BF16; };
template <> struct DtypeOf<f16_t> { static constexpr int value = AC_F16; };
template <typename T, typename... Ts, typename F>
int with_dtype(int dtype, F&& f) {
  if constexpr (sizeof...(Ts) == 0) {
    return f(TypeTag<T>{});
  } else {
    return dtype == DtypeOf<T>::value ? f(TypeTag<T>{}) : with_dtype<Ts...>(dtype, f);
  }
}

}  // namespace ac
