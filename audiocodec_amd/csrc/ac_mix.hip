// Instance and launch of k_mix_p (ac_mix_dev.h): the packed rows of up to AC_MIX_MAX_SOURCES sources summed
// bin by bin into fixed-stride packed rows at the plan's row budget in one launch.  An object of its own: k_transrate_p, whose
// device functions it borrows, keeps its registers and its text.
#include "ac_mix_dev.h"

namespace ac {
namespace {

// grid: ceil(rows / T_WAVES) workgroups of T_WAVES waves
__global__ __launch_bounds__(T_WAVES * 64) void k_mix_p(MixArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[T_WAVES * X_WAVE_WORDS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long r = (long long)blockIdx.x * T_WAVES + wave;
  if (r >= a.rows) return;   // (no workgroup barrier anywhere: the waves of a workgroup share nothing)
  mix_row(a, r, lane, lds + wave * X_WAVE_WORDS);
}

}  // namespace

// where k_transrate_p serves, for 1 .. AC_MIX_MAX_SOURCES sources; any channel count (rows are independent)
bool mix_serves(const ac_psy_plan* psy, int sources_n) {
  return transrate_serves(psy) && sources_n >= 1 && sources_n <= AC_MIX_MAX_SOURCES;
}

int launch_mix(const ac_psy_plan* psy, int sources_n, const ac_packed_rows* src, const int32_t* gain, const uint8_t* active,
               uint8_t* out, int64_t row_bytes, uint8_t* fits, int16_t* offset, long long rows, hipStream_t s) {
  if (rows <= 0) return AC_OK;
  if (!mix_serves(psy, sources_n) || row_bytes != plan_row_bytes(psy)) {
    set_error("internal: no mixing kernel for filters_n = %d, %d bands, row budget %d, %d sources", psy->N, psy->M, psy->row_bits,
              sources_n);
    return AC_EUNSUPPORTED;
  }
  long long groups;
  if (!row_groups(rows, T_WAVES, &groups)) return AC_EINVAL;
  MixArgs a = {};
  for (int i = 0; i < sources_n; ++i) {
    a.data[i] = src[i].data;
    a.nbytes[i] = src[i].nbytes;
    a.index[i] = src[i].index;
    a.gain[i] = gain ? gain[i] : 0;
  }
  a.active = active;
  a.sources_n = sources_n;
  a.band32 = reinterpret_cast<const uint32_t*>(psy->d_qband);
  a.off = psy->d_qoff;
  a.out.data = out;
  a.out.fits = fits;
  a.out.row_bytes = (int)row_bytes;
  a.offset = offset;
  a.rows = rows;
  a.row_bits = psy->row_bits;
  hipLaunchKernelGGL(k_mix_p, dim3((unsigned)groups), dim3(T_WAVES * 64), 0, s, a);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
