// Instances and launch ladder of k_fwd_fast_qps (ac_fast_fwd_qp_dev.h): k_fwd_fast_qp on a chunk of a stream -- the fused
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

template <int CMODE, int SPREAD>
static void launch_qps(const FwdArgs& a, const QuantOut& q, const PackOut& po, int row_bits, int kmin, unsigned grid, hipStream_t s) {
  if constexpr (kStreamRowsGate[CMODE == 2][SPREAD == 2])
    hipLaunchKernelGGL((k_fwd_fast_qps<CMODE, SPREAD>), dim3(grid), dim3(AC_WAVES_PSY * 64), 0, s, a, q, po, row_bits, kmin);
}

int launch_fwd_fast_pack_rows_stream(const ac_mdct_plan* p, const ac_psy_plan* psy, const float* x, float drown, uint8_t* data,
                                     int64_t row_bytes, uint8_t* fits, const float* prev_block, float* state_out, int B, int k,
                                     int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || k <= 0) return AC_OK;
  if (!fast_encode_pack_stream_serves(p, psy, C) || row_bytes != (int64_t)((psy->row_bits + 31) / 32) * 4 || !prev_block ||
      !state_out || prev_block == state_out) {
    set_error("internal: no packing fused encode with streaming state for filters_n = %d, %d channels, row budget %d", p->N, C,
              psy->row_bits);
    return AC_EUNSUPPORTED;
  }
  FwdArgs a;
  unsigned grid;
  const int st = prep_fwd_fast(p, psy, x, 0, nullptr, nullptr, nullptr, drown, prev_block, B, k, k, C, state_out, nullptr, nullptr,
                               0, a, grid);
  if (st) return st;
  QuantOut q;
  q.codes = nullptr;
  q.sf = nullptr;
  q.band = psy->d_qband;
  q.off = psy->d_qoff;
  PackOut po;
  po.data = data;
  po.fits = fits;
  po.row_bytes = (int)row_bytes;
  const int row_bits = psy->row_bits, kmin = psy->kmin;
  if (C == 2) {
    if (psy->spread == 2) launch_qps<0, 2>(a, q, po, row_bits, kmin, grid, s);
    else launch_qps<0, 0>(a, q, po, row_bits, kmin, grid, s);
  } else {
    if (psy->spread == 2) launch_qps<2, 2>(a, q, po, row_bits, kmin, grid, s);
    else launch_qps<2, 0>(a, q, po, row_bits, kmin, grid, s);
  }
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
