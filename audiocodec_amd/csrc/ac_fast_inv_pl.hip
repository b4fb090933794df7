// k_inv_fast_pl: the synthesis from packed rows (k_inv_fast_p, ac_fast_inv_p.hip) that conceals rows which did not arrive
// (parse_strip_p<true>, ac_fast_inv_p_dev.h).  Its own object and its own kernel, so that k_inv_fast_p
// keeps its arguments and registers.
#include "ac_fast_inv_dev.h"

namespace ac {
namespace {

// IOF 7 / 8: float32 / 16-bit PCM out, as 5 / 6 of k_inv_fast_p
template <int R, int CMODE, int NW, int IOF>
__global__ __launch_bounds__(NW * 64, 2) void k_inv_fast_pl(InvArgs a, PackedRows pr, ConcealRows cl) {
  static_assert(R == 8 && (IOF == 7 || IOF == 8), "packed rows, concealed");
  __shared__ __attribute__((aligned(16))) char lds[NW * WAVE_LDS + Geo<R>::TAB_LDS + NW * P_REC_BYTES];
  inv_fast_body<R, CMODE, NW, IOF>(a, lds, (int)blockIdx.x, (int)gridDim.x, nullptr, &pr, &cl);
}

}  // namespace

template <int IOF>
static void launch_inv_pl(const InvArgs& a, const PackedRows& pr, const ConcealRows& cl, int C, unsigned grid, hipStream_t s) {
  const dim3 blk(AC_WAVES * 64);
  if (C == 2) hipLaunchKernelGGL((k_inv_fast_pl<8, 0, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a, pr, cl);
  else hipLaunchKernelGGL((k_inv_fast_pl<8, 2, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a, pr, cl);
}

int launch_inv_fast_packed_conceal(const ac_mdct_plan* p, const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes,
                                   const int64_t* index, const uint8_t* lost, int max_age, void* x, bool pcm16, int B, int Kp,
                                   int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || Kp <= 0) return AC_OK;
  if (!fast_inv_packed_serves(p, psy, C) || lost == nullptr || max_age < 0 || max_age > 31) {
    set_error("internal: no concealing synthesis from packed rows for filters_n = %d, %d bands, %d channels, max_age %d", p->N,
              psy->M, C, max_age);
    return AC_EUNSUPPORTED;
  }
  InvArgs a;
  PackedRows pr;
  unsigned grid;
  const int st = prep_inv_fast_packed(p, psy, data, nbytes, index, x, pcm16, nullptr, nullptr, B, Kp, Kp + 1, C, a, pr, grid);
  if (st) return st;
  ConcealRows cl;
  cl.lost = lost;
  cl.max_age = max_age;
  if (pcm16) launch_inv_pl<8>(a, pr, cl, C, grid, s);
  else launch_inv_pl<7>(a, pr, cl, C, grid, s);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
