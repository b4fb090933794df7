// Instances and launch ladder of k_fwd_fast_qb (ac_fast_quant_dev.h): the quantising fused encode at filters_n = 1024 that
// meets the row budget of its plan (ac_psy_plan_with_row_budget) in the same launch.  An object of its
// own, as ac_fast_fwd_q.hip is: k_fwd_fast_q and every other caller of fwd_fast_body keep their registers and their text.
#include "ac_fast_quant_dev.h"

namespace ac {

int launch_fwd_fast_quant_budget(const ac_mdct_plan* p, const ac_psy_plan* psy, const float* x, float* X, float* t, float* thr,
                                 float drown, int row_bits, int kmin, int16_t* codes, int8_t* sf, int B, int Kin, int F, int C,
                                 hipStream_t s) {
  if (B <= 0 || C <= 0 || F <= 0) return AC_OK;
  if (!fast_encode_quant_serves(p, psy, C)) {
    set_error("internal: no quantising fused encode for filters_n = %d, %d channels", p->N, C);
    return AC_EUNSUPPORTED;
  }
  FwdArgs a;
  unsigned grid;
  const int st = prep_fwd_fast(p, psy, x, 0, X, t, thr, drown, nullptr, B, Kin, F, C, nullptr, nullptr, nullptr, 0, a, grid);
  if (st) return st;
  QuantOut q;
  q.codes = codes;
  q.sf = sf;
  q.band = psy->d_qband;
  q.off = psy->d_qoff;
  const dim3 blk(AC_WAVES_PSY * 64);
  if (C == 2) {
    if (psy->spread == 2) hipLaunchKernelGGL((k_fwd_fast_qb<0, 2>), dim3(grid), blk, 0, s, a, q, row_bits, kmin);
    else hipLaunchKernelGGL((k_fwd_fast_qb<0, 0>), dim3(grid), blk, 0, s, a, q, row_bits, kmin);
  } else {
    if (psy->spread == 2) hipLaunchKernelGGL((k_fwd_fast_qb<2, 2>), dim3(grid), blk, 0, s, a, q, row_bits, kmin);
    else hipLaunchKernelGGL((k_fwd_fast_qb<2, 0>), dim3(grid), blk, 0, s, a, q, row_bits, kmin);
  }
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
