// Instances and launcher of k_fwd_fast_q (ac_fast_quant_dev.h): the fused encode at filters_n = 1024 with the quantiser
// as its last stage -- int16 codes and int8 scale factors in one launch, X / t / thr only where the caller asks for them.
// An object of its own: fwd_fast_body and psy_stage have internal linkage, and sharing a module with their other callers
// would change those kernels' register allocation (DESIGN_LOG.md 9).
#include "ac_fast_quant_dev.h"

namespace ac {

// float32 PCM, filters_n = 1024, mono / stereo, the f32 or split-bf16 spreading product, 64 scale-factor bands
bool fast_encode_quant_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C) {
  return p && psy && p->fast && psy->fast && p->N == Geo<8>::FN && psy->N == p->N && psy->M == 64 && (C == 1 || C == 2) &&
         psy->spread != 1 && psy->d_qoff && psy->d_qband;
}

int launch_fwd_fast_quant(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float* X, float* t, float* thr,
                          float drown, int16_t* codes, int8_t* sf, int B, int Kin, int F, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || F <= 0) return AC_OK;
  if (!fast_encode_quant_serves(p, psy, C)) {
    set_error("internal: no quantising fused encode for filters_n = %d, %d channels", p->N, C);
    return AC_EUNSUPPORTED;
  }
  return launch_fwd_fast_quant_family<kEveryInstance>(
      p, psy, x, 0, X, t, thr, drown, codes, sf, nullptr, nullptr, B, Kin, F, C,
      [&](auto cmode, auto spread, dim3 grid, dim3 blk, const FwdArgs& a, const QuantOut& q) {
        hipLaunchKernelGGL((k_fwd_fast_q<cmode, spread>), grid, blk, 0, s, a, q);
      });
}

}  // namespace ac
