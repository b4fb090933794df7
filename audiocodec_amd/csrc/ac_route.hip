// Instance and launch of k_route_p (ac_route_dev.h): the packed rows of up to AC_ROUTE_MAX_SOURCES sources
// routed into up to AC_ROUTE_MAX_OUTPUTS mixes at the plan's row budget in one launch.  An object of its own: k_mix_p, whose
// device functions it borrows, keeps its registers and its text.
#include "ac_route_dev.h"

namespace ac {
namespace {

// grid: ceil(rows / R_WAVES) workgroups of R_WAVES waves; LDS: R_WAVES slices of r_wave_words(sources_n) words, set by the launch
__global__ __launch_bounds__(R_WAVES * 64) void k_route_p(RouteArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t route_lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long r = (long long)blockIdx.x * R_WAVES + wave;
  if (r >= a.rows) return;   // (no workgroup barrier anywhere: the waves of a workgroup share nothing)
  route_row(a, r, lane, route_lds + wave * r_wave_words(a.sources_n));
}

}  // namespace

// where k_mix_p serves, for 1 .. AC_ROUTE_MAX_SOURCES sources and 1 .. AC_ROUTE_MAX_OUTPUTS outputs; any channel count (rows are independent)
bool route_serves(const ac_psy_plan* psy, int sources_n, int outputs_n) {
  return transrate_serves(psy) && sources_n >= 1 && sources_n <= AC_ROUTE_MAX_SOURCES && outputs_n >= 1 &&
         outputs_n <= AC_ROUTE_MAX_OUTPUTS;
}

int launch_route(const ac_psy_plan* psy, int sources_n, int outputs_n, const ac_packed_rows* src, const int32_t* gain,
                 const uint8_t* active, uint8_t* out, int64_t row_bytes, uint8_t* fits, int16_t* offset, long long rows,
                 hipStream_t s) {
  if (rows <= 0) return AC_OK;
  if (!route_serves(psy, sources_n, outputs_n) || row_bytes != plan_row_bytes(psy)) {
    set_error("internal: no routing kernel for filters_n = %d, %d bands, row budget %d, %d sources, %d outputs", psy->N, psy->M,
              psy->row_bits, sources_n, outputs_n);
    return AC_EUNSUPPORTED;
  }
  long long groups;
  if (!row_groups(rows, R_WAVES, &groups)) return AC_EINVAL;
  RouteArgs a = {};
  for (int i = 0; i < sources_n; ++i) {
    a.data[i] = src[i].data;
    a.nbytes[i] = src[i].nbytes;
    a.index[i] = src[i].index;
  }
  for (int o = 0; o < outputs_n; ++o)
    for (int i = 0; i < sources_n; ++i) {
      const int32_t g = gain[o * sources_n + i];
      if (g == AC_ROUTE_MUTE) continue;
      a.gain[o * sources_n + i] = g;
      a.heard[o] |= 1u << i;
      a.heard_any |= 1u << i;
    }
  a.active = active;
  a.sources_n = sources_n;
  a.outputs_n = outputs_n;
  a.band32 = reinterpret_cast<const uint32_t*>(psy->d_qband);
  a.off = psy->d_qoff;
  a.out.data = out;
  a.out.fits = fits;
  a.out.row_bytes = (int)row_bytes;
  a.offset = offset;
  a.rows = rows;
  a.row_bits = psy->row_bits;
  const size_t lds_bytes = (size_t)R_WAVES * r_wave_words(sources_n) * 4;
  hipLaunchKernelGGL(k_route_p, dim3((unsigned)groups), dim3(R_WAVES * 64), lds_bytes, s, a);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
