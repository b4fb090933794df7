// Instance and launch of k_protect_p (ac_protect_dev.h): packed rows to protected slots -- the row at
// the plan's budget, and behind it the row of the frame before at the redundant budget -- in one launch.  An object of its
// own: k_transrate_p and the kernels whose device functions it borrows keep their registers and their text.
#include "ac_protect_dev.h"

namespace ac {
namespace {

// grid: ceil(rows / T_WAVES) workgroups of T_WAVES waves
__global__ __launch_bounds__(T_WAVES * 64) void k_protect_p(ProtectArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[T_WAVES * T_WAVE_WORDS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long r = (long long)blockIdx.x * T_WAVES + wave;
  if (r >= a.rows) return;   // (no workgroup barrier anywhere: the waves of a workgroup share nothing)
  protect_row(a, r, lane, lds + wave * T_WAVE_WORDS);
}

}  // namespace

// where k_transrate_p serves the plan's budget, and a wave can stage the redundant part too; any channel count
bool protect_serves(const ac_psy_plan* psy, int red_bits) {
  return transrate_serves(psy) && red_bits >= 5 * P_M && red_bits <= kPackRowsMaxBits;
}

int launch_protect(const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes, const int64_t* index, uint8_t* out,
                   int64_t row_bytes, int red_bits, uint8_t* fits, uint8_t* red_fits, int16_t* offset, int16_t* red_offset, int B,
                   int F, int C, hipStream_t s) {
  const long long rows = (long long)B * F * C;
  if (rows <= 0) return AC_OK;
  if (!protect_serves(psy, red_bits) || row_bytes != plan_row_bytes(psy)) {
    set_error("internal: no protecting kernel for filters_n = %d, %d bands, row budget %d, redundant budget %d", psy->N, psy->M,
              psy->row_bits, red_bits);
    return AC_EUNSUPPORTED;
  }
  long long groups;
  if (!row_groups(rows, T_WAVES, &groups)) return AC_EINVAL;
  const ProtectArgs a = protect_args(psy, data, nbytes, index, out, row_bytes, red_bits, fits, red_fits, offset, red_offset, rows,
                                     F, C);
  hipLaunchKernelGGL(k_protect_p, dim3((unsigned)groups), dim3(T_WAVES * 64), 0, s, a);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
