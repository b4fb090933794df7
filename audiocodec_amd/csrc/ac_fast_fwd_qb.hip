// Instances and launcher of k_fwd_fast_qb (ac_fast_quant_dev.h): the quantising fused encode at filters_n = 1024 that
// meets the row budget of its plan (ac_psy_plan_with_row_budget) in the same launch.  An object of its
// own, as ac_fast_fwd_q.hip is: k_fwd_fast_q and every other caller of fwd_fast_body keep their registers and their text.
#include "ac_fast_quant_dev.h"

namespace ac {

int launch_fwd_fast_quant_budget(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float* X, float* t, float* thr,
                                 float drown, int16_t* codes, int8_t* sf, int B, int Kin, int F, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || F <= 0) return AC_OK;
  if (!fast_encode_quant_serves(p, psy, C)) {
    set_error("internal: no quantising fused encode for filters_n = %d, %d channels", p->N, C);
    return AC_EUNSUPPORTED;
  }
  if (!psy->row_bits) {
    set_error("internal: the budgeted quantising fused encode on a plan without a row budget");
    return AC_EUNSUPPORTED;
  }
  const int row_bits = psy->row_bits, kmin = psy->kmin;
  return launch_fwd_fast_quant_family<kEveryInstance>(
      p, psy, x, 0, X, t, thr, drown, codes, sf, nullptr, nullptr, B, Kin, F, C,
      [&](auto cmode, auto spread, dim3 grid, dim3 blk, const FwdArgs& a, const QuantOut& q) {
        hipLaunchKernelGGL((k_fwd_fast_qb<cmode, spread>), grid, blk, 0, s, a, q, row_bits, kmin);
      });
}

}  // namespace ac
