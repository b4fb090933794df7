// k_inv_fast_pls: the concealing synthesis from packed rows (k_inv_fast_pl, ac_fast_inv_pl.hip) launched as one chunk of a
// stream: the overlap comes from and goes to the stream's tails, and the last row that arrived before the chunk is a source
// (parse_strip_p<true, true>, carry_state_p, ac_fast_inv_p_dev.h; DESIGN.md section 8f, "Streams").  Its own object and its
// own kernel, so that k_inv_fast_p and k_inv_fast_pl keep their arguments and registers.
#include "ac_fast_inv_dev.h"

namespace ac {
namespace {

// IOF 9 / 10: float32 / 16-bit PCM out, as 7 / 8 of k_inv_fast_pl
template <int R, int CMODE, int NW, int IOF>
__global__ __launch_bounds__(NW * 64, 2) void k_inv_fast_pls(InvArgs a, PackedRows pr, ConcealRows cl, ConcealState cs) {
  static_assert(R == 8 && (IOF == 9 || IOF == 10), "packed rows, concealed, in a stream");
  __shared__ __attribute__((aligned(16))) char lds[NW * WAVE_LDS + Geo<R>::TAB_LDS + NW * P_REC_BYTES];
  inv_fast_body<R, CMODE, NW, IOF>(a, lds, (int)blockIdx.x, (int)gridDim.x, nullptr, &pr, &cl, &cs);
}

}  // namespace

template <int IOF>
static void launch_inv_pls(const InvArgs& a, const PackedRows& pr, const ConcealRows& cl, const ConcealState& cs, int C,
                           unsigned grid, hipStream_t s) {
  const dim3 blk(AC_WAVES * 64);
  if (C == 2) hipLaunchKernelGGL((k_inv_fast_pls<8, 0, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a, pr, cl, cs);
  else hipLaunchKernelGGL((k_inv_fast_pls<8, 2, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a, pr, cl, cs);
}

// every instance passed the gate (profiles/pack/kernel_resources_conceal_stream.txt): wherever k_inv_fast_p serves
bool fast_inv_packed_conceal_stream_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C) {
  return fast_inv_packed_serves(p, psy, C);
}

size_t conceal_state_row_bytes(int B, int C) { return (size_t)B * (size_t)C * (size_t)P_CARRY_STRIDE; }

int launch_inv_fast_packed_conceal_stream(const ac_mdct_plan* p, const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes,
                                          const int64_t* index, const uint8_t* lost, int max_age, void* x, bool pcm16,
                                          const float* tail_in, float* tail_out, const uint8_t* gap_in, const uint8_t* row_in,
                                          uint8_t* gap_out, uint8_t* row_out, bool stale, int B, int k, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || k <= 0) return AC_OK;
  if (!fast_inv_packed_conceal_stream_serves(p, psy, C) || lost == nullptr || max_age < 0 || max_age > 31) {
    set_error("internal: no concealing synthesis of a chunk of packed rows for filters_n = %d, %d bands, %d channels, max_age %d",
              p->N, psy->M, C, max_age);
    return AC_EUNSUPPORTED;
  }
  InvArgs a;
  PackedRows pr;
  unsigned grid;
  const int st = prep_inv_fast_packed(p, psy, data, nbytes, index, x, pcm16, tail_in, tail_out, B, k, k, C, a, pr, grid);
  if (st) return st;
  ConcealRows cl;
  cl.lost = lost;
  cl.max_age = max_age;
  ConcealState cs;
  cs.gap = gap_in;
  cs.row = row_in;
  cs.gap_out = gap_out;
  cs.row_out = row_out;
  cs.row_bytes = (int64_t)conceal_state_row_bytes(B, C);
  cs.stale = stale ? 1 : 0;
  if (pcm16) launch_inv_pls<10>(a, pr, cl, cs, C, grid, s);
  else launch_inv_pls<9>(a, pr, cl, cs, C, grid, s);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
