// k_inv_fast_plr: the concealing synthesis from packed rows (k_inv_fast_pl, ac_fast_inv_pl.hip) that first recovers a lost row
// from the redundant copy its successor's slot carries (parse_strip_p<true, false, true>, ac_fast_inv_p_dev.h; DESIGN.md
// section 8g).  Its own object and its own kernel, so that k_inv_fast_pl keeps its arguments and registers.
#include "ac_fast_inv_dev.h"

namespace ac {
namespace {

// IOF 11 / 12: float32 / 16-bit PCM out, as 7 / 8 of k_inv_fast_pl
template <int R, int CMODE, int NW, int IOF>
__global__ __launch_bounds__(NW * 64, 2) void k_inv_fast_plr(InvArgs a, PackedRows pr, ConcealRows cl, RedundRows rd) {
  static_assert(R == 8 && (IOF == 11 || IOF == 12), "packed rows, concealed, lost rows recovered");
  __shared__ __attribute__((aligned(16))) char lds[NW * WAVE_LDS + Geo<R>::TAB_LDS + NW * P_REC_BYTES];
  inv_fast_body<R, CMODE, NW, IOF>(a, lds, (int)blockIdx.x, (int)gridDim.x, nullptr, &pr, &cl, nullptr, &rd);
}

}  // namespace

template <int IOF>
static void launch_inv_plr(const InvArgs& a, const PackedRows& pr, const ConcealRows& cl, const RedundRows& rd, int C,
                           unsigned grid, hipStream_t s) {
  const dim3 blk(AC_WAVES * 64);
  if (C == 2) hipLaunchKernelGGL((k_inv_fast_plr<8, 0, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a, pr, cl, rd);
  else hipLaunchKernelGGL((k_inv_fast_plr<8, 2, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a, pr, cl, rd);
}

// every instance passed the gate (profiles/pack/kernel_resources_protect.txt): wherever k_inv_fast_p serves
int launch_inv_fast_packed_recover(const ac_mdct_plan* p, const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes,
                                   const int64_t* index, const uint8_t* lost, int max_age, int64_t redundant_at, void* x,
                                   bool pcm16, int B, int Kp, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || Kp <= 0) return AC_OK;
  if (!fast_inv_packed_serves(p, psy, C) || lost == nullptr || max_age < 0 || max_age > 31 || redundant_at < 1 ||
      redundant_at > 2147483647ll) {
    set_error("internal: no recovering synthesis from packed rows for filters_n = %d, %d bands, %d channels, max_age %d, "
              "redundant_at %lld", p->N, psy->M, C, max_age, (long long)redundant_at);
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
  RedundRows rd;
  rd.at = redundant_at;
  if (pcm16) launch_inv_plr<12>(a, pr, cl, rd, C, grid, s);
  else launch_inv_plr<11>(a, pr, cl, rd, C, grid, s);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
