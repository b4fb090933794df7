// k_fwd_fast_q16: k_fwd_fast_q (ac_fast_quant_dev.h) on 16-bit PCM -- fwd_fast_body with IOF = 1, so the row loads read
// int16 and convert (x = pcm / 32768, Pcm16Fmt::dec), and QuantStage behind it unchanged: codes and sf equal k_fwd_fast_q on
// pcm.to(float32) / 32768 bit for bit.  A kernel name and an object of its own, as ac_fast_fwd_qb.hip
// is: k_fwd_fast_q and every other caller of fwd_fast_body keep their registers and their text.
#include "ac_fast_quant_dev.h"

namespace ac {
namespace {

template <int CMODE, int SPREAD>
__global__ __launch_bounds__(AC_WAVES_PSY * 64, 2) void k_fwd_fast_q16(FwdArgs a, QuantOut q) {
  __shared__ __attribute__((aligned(16))) char lds[fwd_lds_bytes<8, true, AC_WAVES_PSY, SPREAD>()];
  QuantStage<8, CMODE, SPREAD> qz;
  qz.q = q;
  qz.pp = a.psy;
  a.C = CMODE == 0 ? 2 : 1;
  a.prev_block = nullptr;
  a.state_out = nullptr;
  a.noisy = a.dbn = nullptr;
  fwd_fast_body<8, CMODE, true, AC_WAVES_PSY, 1, SPREAD, false, QuantStage<8, CMODE, SPREAD>>(a, lds, (int)blockIdx.x, (int)gridDim.x, qz);
}

}  // namespace

// Served where k_fwd_fast_q serves: every instance passed the register gate of DESIGN.md section 8a -- 2 waves per SIMD and no
// more scratch than the k_fwd_fast_q instance of the same parameters (profiles/pack/kernel_resources_pcm16.txt).
int launch_fwd_fast_quant_pcm16(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float* X, float* t, float* thr,
                                float drown, int16_t* codes, int8_t* sf, int B, int Kin, int F, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || F <= 0) return AC_OK;
  if (!fast_encode_quant_serves(p, psy, C)) {
    set_error("internal: no quantising fused encode of 16-bit PCM for filters_n = %d, %d channels", p->N, C);
    return AC_EUNSUPPORTED;
  }
  return launch_fwd_fast_quant_family<kEveryInstance>(
      p, psy, x, 1, X, t, thr, drown, codes, sf, nullptr, nullptr, B, Kin, F, C,
      [&](auto cmode, auto spread, dim3 grid, dim3 blk, const FwdArgs& a, const QuantOut& q) {
        hipLaunchKernelGGL((k_fwd_fast_q16<cmode, spread>), grid, blk, 0, s, a, q);
      });
}

}  // namespace ac
