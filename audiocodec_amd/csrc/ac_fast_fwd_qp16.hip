// k_fwd_fast_qp16: k_fwd_fast_qp (ac_fast_fwd_qp_dev.h) on 16-bit PCM -- fwd_fast_body with IOF = 1 in front of PackStage:
// the packed rows equal k_fwd_fast_qp's on pcm.to(float32) / 32768 byte for byte.  A kernel name and
// an object of its own: every other caller of fwd_fast_body keeps its registers and its text.
#include "ac_fast_fwd_qp_dev.h"

namespace ac {
namespace {

template <int CMODE, int SPREAD>
__global__ __launch_bounds__(AC_WAVES_PSY * 64, 2) void k_fwd_fast_qp16(FwdArgs a, QuantOut q, PackOut po, int row_bits, int kmin) {
  __shared__ __attribute__((aligned(16))) char lds[fwd_lds_bytes<8, true, AC_WAVES_PSY, SPREAD>()];
  PackStage<8, CMODE, SPREAD> qz;
  q.codes = nullptr;
  q.sf = nullptr;
  qz.q = q;
  qz.po = po;
  qz.pp = a.psy;
  qz.row_bits = row_bits;
  qz.kmin = kmin;
  a.C = CMODE == 0 ? 2 : 1;
  a.X = a.t = a.thr = nullptr;
  a.prev_block = nullptr;
  a.state_out = nullptr;
  a.noisy = a.dbn = nullptr;
  fwd_fast_body<8, CMODE, true, AC_WAVES_PSY, 1, SPREAD, false, PackStage<8, CMODE, SPREAD>>(a, lds, (int)blockIdx.x, (int)gridDim.x, qz);
}

}  // namespace

// Served where k_fwd_fast_qp serves: every instance passed the register gate of DESIGN.md section 8b -- 2 waves per SIMD and no
// more scratch than the k_fwd_fast_qp instance of the same parameters (profiles/pack/kernel_resources_pcm16.txt).
int launch_fwd_fast_pack_rows_pcm16(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float drown, uint8_t* data,
                                    int64_t row_bytes, uint8_t* fits, int B, int Kin, int F, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || F <= 0) return AC_OK;
  if (!fast_encode_pack_serves(p, psy, C) || row_bytes != plan_row_bytes(psy)) {
    set_error("internal: no packing fused encode of 16-bit PCM for filters_n = %d, %d channels, row budget %d", p->N, C,
              psy->row_bits);
    return AC_EUNSUPPORTED;
  }
  const PackOut po{data, fits, (int)row_bytes};
  const int row_bits = psy->row_bits, kmin = psy->kmin;
  return launch_fwd_fast_quant_family<kEveryInstance>(
      p, psy, x, 1, nullptr, nullptr, nullptr, drown, nullptr, nullptr, nullptr, nullptr, B, Kin, F, C,
      [&](auto cmode, auto spread, dim3 grid, dim3 blk, const FwdArgs& a, const QuantOut& q) {
        hipLaunchKernelGGL((k_fwd_fast_qp16<cmode, spread>), grid, blk, 0, s, a, q, po, row_bits, kmin);
      });
}

}  // namespace ac
