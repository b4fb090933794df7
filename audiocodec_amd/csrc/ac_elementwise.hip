// The element-wise utilities as stand-alone kernels: amplitude_to_dB with its backward, and add_noise; float32 on 16-byte
// vectors, float64 and bfloat16 tensors element by element.  gfx950 only.
#include <algorithm>

#include "ac_generic_dev.h"

namespace ac {

typedef float f4 __attribute__((ext_vector_type(4)));

// (db_of, normal_pair, noisy_of: ac_internal.h, shared with the fused encode epilogue)
// 16-byte vectors (n4 of them), one per thread, workgroups in address order (4 KB per workgroup: the store pattern the
// memory system rewards most, tools/ubench_write_pattern.hip) + a scalar tail; a, out 16-byte aligned when n4 > 0
static __global__ __launch_bounds__(256) void k_db(const float* __restrict__ a, float* __restrict__ out, size_t n, size_t n4,
                                            int norm) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n4) {
    const f4 v = reinterpret_cast<const f4*>(a)[i];
    __builtin_nontemporal_store(f4{db_of(v.x, norm), db_of(v.y, norm), db_of(v.z, norm), db_of(v.w, norm)},
                                reinterpret_cast<f4*>(out) + i);
  } else {
    const size_t j = 4 * n4 + (i - n4);
    if (j < n) out[j] = db_of(a[j], norm);
  }
}

// d amplitude_to_dB / d a = (20 / ln 10) / a where a^2 > eps, else 0 (the clamp); the normalised form scales by 1 / 140
static __global__ __launch_bounds__(256) void k_db_bwd(const float* __restrict__ a, const float* __restrict__ g,
                                                float* __restrict__ ga, size_t n, int norm) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const float c = norm ? (8.685889638065035f / 140.f) : 8.685889638065035f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float v = a[i];
    ga[i] = (v * v > kEps) ? g[i] * (c / v) : 0.f;
  }
}

// add_noise (psychoacoustic.py:150-167): out = X + thr * Normal(0, 1/6); X == nullptr stands for zeros (the gradient of
// add_noise with respect to the threshold is add_noise(0, grad_out) under the same seed)
static __global__ __launch_bounds__(256) void k_add_noise(const float* __restrict__ X, const float* __restrict__ thr,
                                                   float* __restrict__ out, size_t n, size_t n4, uint64_t seed) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t key = mix64(seed);
  if (i < n4) {
    const f4 x = X ? reinterpret_cast<const f4*>(X)[i] : f4{0.f, 0.f, 0.f, 0.f}, t = reinterpret_cast<const f4*>(thr)[i];
    float g0, g1, g2, g3;
    normal_pair(key, 2 * i, g0, g1);
    normal_pair(key, 2 * i + 1, g2, g3);
    __builtin_nontemporal_store(f4{noisy_of(x.x, t.x, g0), noisy_of(x.y, t.y, g1), noisy_of(x.z, t.z, g2), noisy_of(x.w, t.w, g3)},
                                reinterpret_cast<f4*>(out) + i);
  } else {
    const size_t j = 4 * n4 + (i - n4);
    if (j < n) {
      float g0, g1;
      normal_pair(key, j >> 1, g0, g1);
      out[j] = noisy_of(X ? X[j] : 0.f, thr[j], (j & 1) ? g1 : g0);
    }
  }
}

// the same two utilities for the other storage types (double: fp64 arithmetic; bfloat16: float32 arithmetic), one
// element per thread and iteration; the noise stream is the float32 one (same seed, same normals)
template <typename TIO, typename TC = typename Compute<TIO>::type>
static __global__ __launch_bounds__(256) void k_db_typed(const TIO* __restrict__ a, TIO* __restrict__ out, size_t n, int norm) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const TC v = ldv(a + i);
    TC dB = (TC)10 * m_log(m_max((TC)1e-14, v * v)) / (TC)2.302585092994046 + (TC)120;
    if (norm) dB = (dB + (TC)20) / (TC)140;
    stv(out + i, dB);
  }
}
template <typename TIO, typename TC = typename Compute<TIO>::type>
static __global__ __launch_bounds__(256) void k_add_noise_typed(const TIO* __restrict__ X, const TIO* __restrict__ thr,
                                                         TIO* __restrict__ out, size_t n, uint64_t seed) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const uint64_t key = mix64(seed);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float g0, g1;
    normal_pair(key, i >> 1, g0, g1);
    stv(out + i, (X ? (TC)ldv(X + i) : (TC)0) + (TC)ldv(thr + i) * ((TC)((i & 1) ? g1 : g0) / (TC)6));
  }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// the grid of the two float32 kernels: 16-byte vectors (*n4 of them) when every pointer (their addresses or'ed: addr_bits) allows
// it, else element by element; one thread per vector, then one per tail element
static int vec4_grid(uintptr_t addr_bits, size_t n, size_t* n4, unsigned* grid) {
  *n4 = (addr_bits & 15) == 0 ? n / 4 : 0;
  const size_t nblk = (*n4 + (n - 4 * *n4) + 255) / 256;
  if (nblk > 2147483647ull) {
    set_error("tensor too large for one launch (%zu elements)", n);
    return AC_EINVAL;
  }
  *grid = (unsigned)nblk;
  return AC_OK;
}

template <typename TIO>
static int launch_db_T(const TIO* a, TIO* out, size_t n, int norm, hipStream_t s) {
  if (n == 0) return AC_OK;
  if constexpr (std::is_same<TIO, float>::value) {
    size_t n4 = 0;
    unsigned grid = 0;
    const int st = vec4_grid((uintptr_t)a | (uintptr_t)out, n, &n4, &grid);
    if (st) return st;
    hipLaunchKernelGGL(k_db, dim3(grid), dim3(256), 0, s, a, out, n, n4, norm);
  } else {
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL((k_db_typed<TIO>), dim3(grid), dim3(256), 0, s, a, out, n, norm);
  }
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

int launch_db_bwd(const float* a, const float* g, float* ga, size_t n, int norm, hipStream_t s) {
  if (n == 0) return AC_OK;
  const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 16384);
  hipLaunchKernelGGL(k_db_bwd, dim3(grid), dim3(256), 0, s, a, g, ga, n, norm);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

template <typename TIO>
static int launch_add_noise_T(const TIO* X, const TIO* thr, TIO* out, size_t n, uint64_t seed, hipStream_t s) {
  if (n == 0) return AC_OK;
  if constexpr (std::is_same<TIO, float>::value) {
    size_t n4 = 0;
    unsigned grid = 0;
    const int st = vec4_grid((uintptr_t)X | (uintptr_t)thr | (uintptr_t)out, n, &n4, &grid);
    if (st) return st;
    hipLaunchKernelGGL(k_add_noise, dim3(grid), dim3(256), 0, s, X, thr, out, n, n4, seed);
  } else {
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL((k_add_noise_typed<TIO>), dim3(grid), dim3(256), 0, s, X, thr, out, n, seed);
  }
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

// ---- the entry points of the unit (ac_internal.h): tensors of `dtype`, float32, float64 or bfloat16
int launch_db_typed(const void* a, void* out, size_t n, int norm, int dtype, hipStream_t s) {
  return with_dtype<float, double, bf16_t>(dtype, [&](auto tag) {
    using TIO = typename decltype(tag)::type;
    return launch_db_T((const TIO*)a, (TIO*)out, n, norm, s);
  });
}
int launch_add_noise_typed(const void* X, const void* thr, void* out, size_t n, uint64_t seed, int dtype, hipStream_t s) {
  return with_dtype<float, double, bf16_t>(dtype, [&](auto tag) {
    using TIO = typename decltype(tag)::type;
    return launch_add_noise_T((const TIO*)X, (const TIO*)thr, (TIO*)out, n, seed, s);
  });
}

}  // namespace ac
