// k_inv_fast_plsr: the concealing synthesis of a chunk of a stream (k_inv_fast_pls, ac_fast_inv_pls.hip) that first recovers a
// lost row from the redundant copy its successor's slot carries, as k_inv_fast_plr does one-shot (parse_strip_p<true, true, true>,
// ac_fast_inv_p_dev.h; DESIGN.md section 8g, "Streams").  The chunk is synthesised one frame behind its rows: block n of the
// launch is the frame of row n - 1, row -1 being the deferred last row of the chunk before, so the successor of every frame is in
// the chunk in hand.  Tails, strips and carry_state_p are k_inv_fast_pls's.  Its own object and its own kernel, so that the other
// forms keep their arguments and registers.
#include "ac_fast_inv_dev.h"

namespace ac {
namespace {

// IOF 13 / 14: float32 / 16-bit PCM out, as 9 / 10 of k_inv_fast_pls
template <int R, int CMODE, int NW, int IOF>
__global__ __launch_bounds__(NW * 64, 2) void k_inv_fast_plsr(InvArgs a, PackedRows pr, ConcealRows cl, ConcealState cs,
                                                              RedundRows rd) {
  static_assert(R == 8 && (IOF == 13 || IOF == 14), "packed rows, concealed and recovered, in a stream");
  __shared__ __attribute__((aligned(16))) char lds[NW * WAVE_LDS + Geo<R>::TAB_LDS + NW * P_REC_BYTES];
  inv_fast_body<R, CMODE, NW, IOF>(a, lds, (int)blockIdx.x, (int)gridDim.x, nullptr, &pr, &cl, &cs, &rd);
}

}  // namespace

template <int IOF>
static void launch_inv_plsr(const InvArgs& a, const PackedRows& pr, const ConcealRows& cl, const ConcealState& cs,
                            const RedundRows& rd, int C, unsigned grid, hipStream_t s) {
  const dim3 blk(AC_WAVES * 64);
  if (C == 2) hipLaunchKernelGGL((k_inv_fast_plsr<8, 0, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a, pr, cl, cs, rd);
  else hipLaunchKernelGGL((k_inv_fast_plsr<8, 2, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a, pr, cl, cs, rd);
}

// every instance passed the gate (profiles/pack/kernel_resources_protect_stream.txt): wherever k_inv_fast_p serves
bool fast_inv_packed_recover_stream_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C) {
  return fast_inv_packed_serves(p, psy, C);
}

int launch_inv_fast_packed_recover_stream(const ac_mdct_plan* p, const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes,
                                          const int64_t* index, const uint8_t* lost, int max_age, int64_t redundant_at, void* x,
                                          bool pcm16, const float* tail_in, float* tail_out, const uint8_t* gap_in,
                                          const uint8_t* row_in, uint8_t* gap_out, uint8_t* row_out, bool stale, int B, int k,
                                          int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || k <= 0) return AC_OK;
  if (!fast_inv_packed_recover_stream_serves(p, psy, C) || lost == nullptr || max_age < 0 || max_age > 31 || redundant_at < 1 ||
      redundant_at > 2147483647ll) {
    set_error("internal: no recovering synthesis of a chunk of packed rows for filters_n = %d, %d bands, %d channels, max_age %d, "
              "redundant_at %lld", p->N, psy->M, C, max_age, (long long)redundant_at);
    return AC_EUNSUPPORTED;
  }
  InvArgs a;
  PackedRows pr;
  unsigned grid;
  // k blocks from k synthesis frames: the deferred row and rows 0 .. k-2; index and lost hold the chunk's k rows
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
  RedundRows rd;
  rd.at = redundant_at;
  if (pcm16) launch_inv_plsr<14>(a, pr, cl, cs, rd, C, grid, s);
  else launch_inv_plsr<13>(a, pr, cl, cs, rd, C, grid, s);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
