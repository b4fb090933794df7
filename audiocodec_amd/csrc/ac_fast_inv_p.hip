// Instances and launch of k_inv_fast_p: synthesis at filters_n = 1024 straight from rows of the packed bitstream
// (ac_fast_inv_p_dev.h).  Its own object, so that k_inv_fast and k_inv_fast_q keep their registers.
#include "ac_fast_inv_dev.h"

namespace ac {

bool fast_inv_packed_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C) {
  return p->fast && p->N == Geo<8>::FN && psy->N == p->N && psy->M == P_M && psy->d_qoff && psy->d_qband && (C == 1 || C == 2);
}

template <int IOF>
static void launch_inv_p(const InvArgs& a, const PackedRows& pr, int C, unsigned grid, hipStream_t s) {
  const dim3 blk(AC_WAVES * 64);
  if (C == 2) hipLaunchKernelGGL((k_inv_fast_p<8, 0, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a, pr);
  else hipLaunchKernelGGL((k_inv_fast_p<8, 2, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a, pr);
}

int launch_inv_fast_packed(const ac_mdct_plan* p, const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes,
                           const int64_t* index, void* x, bool pcm16, const float* tail_in, float* tail_out, int B, int Kp,
                           int nblk, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || Kp <= 0) return AC_OK;
  if (!fast_inv_packed_serves(p, psy, C) || (nblk != Kp && nblk != Kp + 1)) {
    set_error("internal: no synthesis from packed rows for filters_n = %d, %d bands, %d channels", p->N, psy->M, C);
    return AC_EUNSUPPORTED;
  }
  InvArgs a;
  PackedRows pr;
  unsigned grid;
  const int st = prep_inv_fast_packed(p, psy, data, nbytes, index, x, pcm16, tail_in, tail_out, B, Kp, nblk, C, a, pr, grid);
  if (st) return st;
  if (pcm16) launch_inv_p<6>(a, pr, C, grid, s);
  else launch_inv_p<5>(a, pr, C, grid, s);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
