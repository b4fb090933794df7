// What the files of the wave-level masking model for general band layouts share: ac_psy_mid.hip (k_psy_mid, k_psy_runs),
// ac_psy_runs_team_dev.h (k_psy_runs_c) and the table builders of ac_psy_mid_plan.hip -- the size classes, the arguments of the
// run-structured kernels and the one launch path of the three kernel families.  Internal linkage throughout, as InvArgs in
// ac_fast_inv_dev.h: an argument struct is part of its kernels' names, so no function can pass one between objects.
#pragma once
#include <type_traits>

#include "ac_fast.h"
#include "ac_psy_runs_dev.h"

// Granule registers per lane from which the W_inv entries are read from global memory instead of the LDS image: from 8 (frames
// above 512 bins), where the table is 15 ... 64 KB and keeping it out of LDS doubles the resident waves (B = 256 stereo, the
// un-fused encode: 960 0.912 -> 0.843 ms, 1000 0.921 -> 0.829, 768 unchanged; mono 960 0.736 -> 0.560).
#ifndef AC_MID_WI_GLOBAL_R
#define AC_MID_WI_GLOBAL_R 8
#endif

namespace ac {
namespace {

typedef float v2u __attribute__((ext_vector_type(2), aligned(4)));   // two floats on the 4-byte grid

constexpr int mid_r(int N) { return N <= 128 ? 1 : N <= 256 ? 2 : N <= 512 ? 4 : N <= 1024 ? 8 : N <= 2048 ? 16 : 32; }   // granule registers per lane
// frames a wave handles side by side: as many as keep the frames' registers (4 R each) within the budget
constexpr int psy_fb(int R) { return R >= 8 ? 1 : R == 4 ? 2 : 4; }

// ---- the run-structured form (ac_psy_runs_dev.h) -----------------------------------------------------------------------
struct RunsArgs {
  const float* X;
  const float* t_in;
  float* t_out;
  float* thr;
  const uint32_t* img;   // ac_psy_plan::d_runs
  runs::RunsParams p;
  int C, F;
  int T;                 // frames per wave, as in MidArgs
  long long nsig, ntasks;
};

// The head MidArgs and RunsArgs share: t_out != null: tonality (from X); thr != null: threshold (from t_out when given, else
// from t_in).  ntasks: pairs of rows x frames -- stereo: the clips; mono: pairs of clips; else the channel pairs of every clip
template <class Args>
void fill_psy_args(Args& a, const float* X, const float* t_in, float* t_out, float* thr, const uint32_t* img, int B, int F, int C) {
  a.X = X;
  a.t_in = t_in;
  a.t_out = t_out;
  a.thr = thr;
  a.img = img;
  a.C = C;
  a.F = F;
  a.nsig = (long long)B * C;
  a.ntasks = (C == 2 ? (long long)B : C == 1 ? (a.nsig + 1) / 2 : (long long)B * ((C + 1) / 2)) * F;
}

// frames per wave (per workgroup: the team form), `most` halved down to `least`: as many as keep every CU supplied with a few
// workgroups of `per` tasks a round (the image copy is paid per workgroup)
inline int psy_frames_per_wave(const ac_psy_plan* p, long long ntasks, int per, int most, int least) {
  const int cus = p->cus > 0 ? p->cus : 256;
  int T = most;
  while (T > least && ntasks < (long long)per * T * cus * 6) T >>= 1;
  return T;
}

// one launch with `lds` bytes of dynamic LDS (above 64 KB a kernel has to be told)
template <class Kernel, class Args>
int launch_psy_lds(Kernel kernel, unsigned grid, int waves, size_t lds, hipStream_t s, const Args& a) {
  if (lds > 64 * 1024)
    AC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, s, a);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

// ---- the compile-time side of a launch, in the manner of with_dtype (ac_generic_dev.h): only what is named here is instantiated
template <int V> using Int = std::integral_constant<int, V>;
// f(Int<R>, Int<CMODE>) for the granule registers per lane r in {1, 2, 4, 8, 16, 32} (mid_r) and the row layout of C channels:
// CMODE 0 stereo, 1 the channel pairs of three or more channels, 2 mono (two signals side by side)
template <int R = 1, class F>
int with_r_cmode(int r, int C, F&& f) {
  if constexpr (R < 32)
    if (r != R) return with_r_cmode<2 * R>(r, C, f);
  return C > 2 ? f(Int<R>{}, Int<1>{}) : C == 2 ? f(Int<R>{}, Int<0>{}) : f(Int<R>{}, Int<2>{});
}
// the instance of a kernel family for the outputs a call wants: family(WANT_T, WANT_THR), two std::bool_constant, names the
// kernel -- both, the threshold from a given tonality, or (neither pointer decides otherwise) the tonality alone
template <class Family, class Args>
int launch_psy_outputs(Family family, unsigned grid, int waves, size_t lds, hipStream_t s, const Args& a) {
  if (a.t_out && a.thr) return launch_psy_lds(family(std::true_type{}, std::true_type{}), grid, waves, lds, s, a);
  if (a.thr) return launch_psy_lds(family(std::false_type{}, std::true_type{}), grid, waves, lds, s, a);
  return launch_psy_lds(family(std::true_type{}, std::false_type{}), grid, waves, lds, s, a);
}

}  // namespace
}  // namespace ac
