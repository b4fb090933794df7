// Instances and launcher of k_fwd_fast_qps (ac_fast_fwd_qp_dev.h): k_fwd_fast_qp on a chunk of a stream -- the fused
// encode at filters_n = 1024 that writes fixed-stride packed rows ("Packed rows in a stream"), with block
// -1 of every signal read from the stream's state and the chunk's last block stored as the next state.  An object of its own,
// as ac_fast_fwd_qp.hip is: the one-shot instances and every other caller of fwd_fast_body keep their registers and their text.
#include "ac_fast_fwd_qp_dev.h"

namespace ac {

// The register gate of DESIGN.md section 8b: an instance is built only where it runs 2 waves per SIMD with no more scratch
// than the k_fwd_fast_qp instance of the same parameters (profiles/pack/kernel_resources_stream_rows.txt holds the figures).
// [mono][split-bf16 spreading].  Stereo with the f32 spreading product spills 12 bytes per lane where k_fwd_fast_qp<0, 0> spills
// nothing: not built, its chunks take the composition (ac_stream_packed_launches says so).  -DAC_QPS_BUILD_ALL builds all four,
// to take the gate's figures again (python tools/kernel_resources.py audiocodec_amd/csrc/ac_fast_fwd_qps.hip "" -DAC_QPS_BUILD_ALL).
#ifdef AC_QPS_BUILD_ALL
constexpr bool kStreamRowsGate[2][2] = {{true, true}, {true, true}};
#else
constexpr bool kStreamRowsGate[2][2] = {{false, true}, {true, true}};
#endif

bool fast_encode_pack_stream_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C) {
  return fast_encode_pack_serves(p, psy, C) && kStreamRowsGate[C == 1][psy->spread == 2];
}

int launch_fwd_fast_pack_rows_stream(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float drown, uint8_t* data,
                                     int64_t row_bytes, uint8_t* fits, const float* prev_block, float* state_out, int B, int k,
                                     int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || k <= 0) return AC_OK;
  if (!fast_encode_pack_stream_serves(p, psy, C) || row_bytes != plan_row_bytes(psy) || !prev_block || !state_out ||
      prev_block == state_out) {
    set_error("internal: no packing fused encode with streaming state for filters_n = %d, %d channels, row budget %d", p->N, C,
              psy->row_bits);
    return AC_EUNSUPPORTED;
  }
  const PackOut po{data, fits, (int)row_bytes};
  const int row_bits = psy->row_bits, kmin = psy->kmin;
  return launch_fwd_fast_quant_family<kStreamRowsGate>(
      p, psy, x, 0, nullptr, nullptr, nullptr, drown, nullptr, nullptr, prev_block, state_out, B, k, k, C,
      [&](auto cmode, auto spread, dim3 grid, dim3 blk, const FwdArgs& a, const QuantOut& q) {
        hipLaunchKernelGGL((k_fwd_fast_qps<cmode, spread>), grid, blk, 0, s, a, q, po, row_bits, kmin);
      });
}

}  // namespace ac
