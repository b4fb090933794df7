// Instance and launch of k_transrate_p (ac_transrate_dev.h): packed rows to fixed-stride packed rows at
// the plan's row budget in one launch.  An object of its own: the fused encode and the synthesis whose device functions it
// borrows keep their registers and their text.
#include "ac_transrate_dev.h"

namespace ac {
namespace {

// grid: ceil(rows / T_WAVES) workgroups of T_WAVES waves
__global__ __launch_bounds__(T_WAVES * 64) void k_transrate_p(TransArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[T_WAVES * T_WAVE_WORDS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long r = (long long)blockIdx.x * T_WAVES + wave;
  if (r >= a.rows) return;   // (no workgroup barrier anywhere: the waves of a workgroup share nothing)
  transrate_row(a, r, lane, lds + wave * T_WAVE_WORDS);
}

}  // namespace

// float32 plans with 1024 bins in 64 bands and a budget whose slot a wave can stage; any channel count (rows are independent)
bool transrate_serves(const ac_psy_plan* psy) {
  return psy->N == 1024 && psy->M == P_M && psy->d_qoff && psy->d_qband && psy->row_bits >= 5 * P_M &&
         psy->row_bits <= kPackRowsMaxBits;
}

int launch_transrate(const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes, const int64_t* index, uint8_t* out,
                     int64_t row_bytes, uint8_t* fits, int16_t* offset, long long rows, hipStream_t s) {
  if (rows <= 0) return AC_OK;
  if (!transrate_serves(psy) || row_bytes != plan_row_bytes(psy)) {
    set_error("internal: no transrating kernel for filters_n = %d, %d bands, row budget %d", psy->N, psy->M, psy->row_bits);
    return AC_EUNSUPPORTED;
  }
  long long groups;
  if (!row_groups(rows, T_WAVES, &groups)) return AC_EINVAL;
  TransArgs a;
  a.in = plan_rows(psy, data, nbytes, index);
  a.out.data = out;
  a.out.fits = fits;
  a.out.row_bytes = (int)row_bytes;
  a.offset = offset;
  a.rows = rows;
  a.row_bits = psy->row_bits;
  hipLaunchKernelGGL(k_transrate_p, dim3((unsigned)groups), dim3(T_WAVES * 64), 0, s, a);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
