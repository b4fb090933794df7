// Instances and launch ladder of k_fwd_fast_q (ac_fast_quant_dev.h): the fused encode at filters_n = 1024 with the quantiser
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

int launch_fwd_fast_quant(const ac_mdct_plan* p, const ac_psy_plan* psy, const float* x, float* X, float* t, float* thr,
                          float drown, int16_t* codes, int8_t* sf, int B, int Kin, int F, int C, hipStream_t s) {
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
    if (psy->spread == 2) hipLaunchKernelGGL((k_fwd_fast_q<0, 2>), dim3(grid), blk, 0, s, a, q);
    else hipLaunchKernelGGL((k_fwd_fast_q<0, 0>), dim3(grid), blk, 0, s, a, q);
  } else {
    if (psy->spread == 2) hipLaunchKernelGGL((k_fwd_fast_q<2, 2>), dim3(grid), blk, 0, s, a, q);
    else hipLaunchKernelGGL((k_fwd_fast_q<2, 0>), dim3(grid), blk, 0, s, a, q);
  }
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
