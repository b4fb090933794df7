// k_fwd_fast_qps16: k_fwd_fast_qps (ac_fast_fwd_qp_dev.h) on 16-bit PCM -- a chunk of a stream to fixed-stride packed rows
// ("Packed rows in a stream").  fwd_fast_body with IOF = 1 under a QUANT reads block -1 of every
// signal from the stream's float32 state (as the bfloat16 form does) and the wave that loads block Kin - 1 stores the
// converted block (pcm / 32768, exact in float32) as the next state: an int16 chunk leaves the state the float32 chunk of
// pcm / 32768 leaves, and chunk calls of every form keep following each other.  A kernel name and an object of its own.
#include "ac_fast_fwd_qp_dev.h"

namespace ac {
namespace {

template <int CMODE, int SPREAD>
__global__ __launch_bounds__(AC_WAVES_PSY * 64, 2) void k_fwd_fast_qps16(FwdArgs a, QuantOut q, PackOut po, int row_bits, int kmin) {
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
  a.noisy = a.dbn = nullptr;
  fwd_fast_body<8, CMODE, true, AC_WAVES_PSY, 1, SPREAD, false, PackStage<8, CMODE, SPREAD>>(a, lds, (int)blockIdx.x, (int)gridDim.x, qz);
}

}  // namespace

// The register gate of k_fwd_fast_qps: built only where the instance runs 2 waves per SIMD with no
// more scratch than the k_fwd_fast_qp instance of the same parameters (profiles/pack/kernel_resources_pcm16.txt).
// [mono][split-bf16 spreading].  With the f32 spreading product stereo spills 20 bytes per lane and mono 12 where k_fwd_fast_qp
// spills nothing: not built, their int16 chunks take the composition (ac_stream_packed_launches_pcm16 says so).
// -DAC_QPS16_BUILD_ALL builds all four, to take the gate's figures again
// (python tools/kernel_resources.py audiocodec_amd/csrc/ac_fast_fwd_qps16.hip "" -DAC_QPS16_BUILD_ALL).
#ifdef AC_QPS16_BUILD_ALL
constexpr bool kStreamRows16Gate[2][2] = {{true, true}, {true, true}};
#else
constexpr bool kStreamRows16Gate[2][2] = {{false, true}, {false, true}};
#endif

bool fast_encode_pack_stream_pcm16_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C) {
  return fast_encode_pack_serves(p, psy, C) && kStreamRows16Gate[C == 1][psy->spread == 2];
}

int launch_fwd_fast_pack_rows_stream_pcm16(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float drown,
                                           uint8_t* data, int64_t row_bytes, uint8_t* fits, const float* prev_block,
                                           float* state_out, int B, int k, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || k <= 0) return AC_OK;
  if (!fast_encode_pack_stream_pcm16_serves(p, psy, C) || row_bytes != plan_row_bytes(psy) || !prev_block || !state_out ||
      prev_block == state_out) {
    set_error("internal: no packing fused encode of 16-bit PCM with streaming state for filters_n = %d, %d channels, row budget %d",
              p->N, C, psy->row_bits);
    return AC_EUNSUPPORTED;
  }
  const PackOut po{data, fits, (int)row_bytes};
  const int row_bits = psy->row_bits, kmin = psy->kmin;
  return launch_fwd_fast_quant_family<kStreamRows16Gate>(
      p, psy, x, 1, nullptr, nullptr, nullptr, drown, nullptr, nullptr, prev_block, state_out, B, k, k, C,
      [&](auto cmode, auto spread, dim3 grid, dim3 blk, const FwdArgs& a, const QuantOut& q) {
        hipLaunchKernelGGL((k_fwd_fast_qps16<cmode, spread>), grid, blk, 0, s, a, q, po, row_bits, kmin);
      });
}

}  // namespace ac
