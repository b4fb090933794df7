// Instance and launch of k_protect_ps (ac_protect_dev.h; DESIGN.md section 8g, "Streams"): k_protect_p on one chunk of a stream
// -- the frame-0 slots take the copy the chunk before left in the carry, the copy of the chunk's last row goes into the carry's
// other half.  An object of its own: k_protect_p keeps its registers and its text.
#include "ac_protect_dev.h"

namespace ac {
namespace {

// grid: ceil(rows / T_WAVES) workgroups of T_WAVES waves
__global__ __launch_bounds__(T_WAVES * 64) void k_protect_ps(ProtectArgs a, ProtectCarry pc) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[T_WAVES * T_WAVE_WORDS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long r = (long long)blockIdx.x * T_WAVES + wave;
  if (r >= a.rows) return;   // (no workgroup barrier anywhere: the waves of a workgroup share nothing)
  protect_row<true>(a, r, lane, lds + wave * T_WAVE_WORDS, &pc);
}

}  // namespace

int launch_protect_stream(const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes, const int64_t* index, uint8_t* out,
                          int64_t row_bytes, int red_bits, uint8_t* fits, uint8_t* red_fits, int16_t* offset, int16_t* red_offset,
                          const uint8_t* row_in, const uint8_t* fits_in, const int16_t* offset_in, uint8_t* row_out,
                          uint8_t* fits_out, int16_t* offset_out, int B, int F, int C, hipStream_t s) {
  const long long rows = (long long)B * F * C;
  if (rows <= 0) return AC_OK;
  if (!protect_serves(psy, red_bits) || row_bytes != plan_row_bytes(psy) || row_out == nullptr || fits_out == nullptr ||
      offset_out == nullptr || (row_in != nullptr && (fits_in == nullptr || offset_in == nullptr))) {
    set_error("internal: no protecting kernel for a chunk at filters_n = %d, %d bands, row budget %d, redundant budget %d", psy->N,
              psy->M, psy->row_bits, red_bits);
    return AC_EUNSUPPORTED;
  }
  long long groups;
  if (!row_groups(rows, T_WAVES, &groups)) return AC_EINVAL;
  const ProtectArgs a = protect_args(psy, data, nbytes, index, out, row_bytes, red_bits, fits, red_fits, offset, red_offset, rows,
                                     F, C);
  ProtectCarry pc;
  pc.row_in = row_in;
  pc.fits_in = fits_in;
  pc.offset_in = offset_in;
  pc.row_out = row_out;
  pc.fits_out = fits_out;
  pc.offset_out = offset_out;
  hipLaunchKernelGGL(k_protect_ps, dim3((unsigned)groups), dim3(T_WAVES * 64), 0, s, a, pc);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
