// Instance and launch of k_level_p (ac_level_dev.h): the energy of packed rows, and whether a row holds a
// band without a finite scale factor, from the rows themselves in one launch.  An object of its own: k_transrate_p and k_mix_p,
// whose device functions it borrows, keep their registers and their text.
#include "ac_level_dev.h"

namespace ac {
namespace {

// grid: ceil(rows / T_WAVES) workgroups of T_WAVES waves
__global__ __launch_bounds__(T_WAVES * 64) void k_level_p(LevelArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[T_WAVES * L_WAVE_WORDS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long r = (long long)blockIdx.x * T_WAVES + wave;
  if (r >= a.rows) return;   // (no workgroup barrier anywhere: the waves of a workgroup share nothing)
  level_row(a, r, lane, lds + wave * L_WAVE_WORDS);
}

}  // namespace

// float32 plans with 1024 bins in 64 bands, with or without a row budget; any channel count (rows are independent)
bool level_serves(const ac_psy_plan* psy) { return psy->N == 1024 && psy->M == P_M && psy->d_qoff && psy->d_qband; }

int launch_level(const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes, const int64_t* index, float* energy, uint8_t* bad,
                 long long rows, hipStream_t s) {
  if (rows <= 0) return AC_OK;
  if (!level_serves(psy)) {
    set_error("internal: no level kernel for filters_n = %d, %d bands", psy->N, psy->M);
    return AC_EUNSUPPORTED;
  }
  long long groups;
  if (!row_groups(rows, T_WAVES, &groups)) return AC_EINVAL;
  LevelArgs a;
  a.in = plan_rows(psy, data, nbytes, index);
  a.energy = energy;
  a.bad = bad;
  a.rows = rows;
  hipLaunchKernelGGL(k_level_p, dim3((unsigned)groups), dim3(T_WAVES * 64), 0, s, a);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
