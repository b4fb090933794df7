// Instances and launcher of k_fwd_fast_qp (ac_fast_fwd_qp_dev.h): the fused encode at filters_n = 1024 that meets the row
// budget of its plan and writes fixed-stride packed rows in the same launch.  An object of its own,
// as ac_fast_fwd_qb.hip is: k_fwd_fast_qb and every other caller of fwd_fast_body keep their registers and their text.
#include "ac_fast_fwd_qp_dev.h"

namespace ac {

// where k_fwd_fast_qb serves, with 64 bands (a band per lane) and a budget whose slot the wave can stage
bool fast_encode_pack_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C) {
  return fast_encode_quant_serves(p, psy, C) && psy->row_bits >= 5 * 64 && psy->row_bits <= kPackRowsMaxBits;
}

int launch_fwd_fast_pack_rows(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float drown, uint8_t* data,
                              int64_t row_bytes, uint8_t* fits, int B, int Kin, int F, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || F <= 0) return AC_OK;
  if (!fast_encode_pack_serves(p, psy, C) || row_bytes != plan_row_bytes(psy)) {
    set_error("internal: no packing fused encode for filters_n = %d, %d channels, row budget %d", p->N, C, psy->row_bits);
    return AC_EUNSUPPORTED;
  }
  const PackOut po{data, fits, (int)row_bytes};
  const int row_bits = psy->row_bits, kmin = psy->kmin;
  return launch_fwd_fast_quant_family<kEveryInstance>(
      p, psy, x, 0, nullptr, nullptr, nullptr, drown, nullptr, nullptr, nullptr, nullptr, B, Kin, F, C,
      [&](auto cmode, auto spread, dim3 grid, dim3 blk, const FwdArgs& a, const QuantOut& q) {
        hipLaunchKernelGGL((k_fwd_fast_qp<cmode, spread>), grid, blk, 0, s, a, q, po, row_bits, kmin);
      });
}

}  // namespace ac
