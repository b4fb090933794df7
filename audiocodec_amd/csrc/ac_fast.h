// Host-side declarations the objects of the wave-level kernels (ac_fast_*.hip) need from each other and that
// ac_internal.h does not carry.  Internal to the library: none of these is exported.
#pragma once
#include "ac_internal.h"

namespace ac {

// ac_fast_plan.hip: workgroups of a launch of ntasks wave tasks, nw per workgroup (AC_EINVAL: too many for one launch) ...
int grid_for(long long ntasks, int nw, unsigned* grid);
// ... and of a persistent launch: enough to fill every CU at the kernel's occupancy, a multiple of 8 (XCDs)
unsigned persistent_grid(int cus, int wg_per_cu, long long ntasks, int nw);

// ac_fast_inv.hip: output blocks per synthesis strip (AC_SEGLEN overrides `preferred`)
int pick_seglen(long long pairs, int frames, int preferred);

// ac_fast_multi.hip: the several-frames-per-wave kernels (filters_n 512 ... 64), where fast_multi_serves();
// psy (may be null): the plan of the masking model for general band layouts, fused into the launch (fast_multi_fuses())
int launch_fwd_multi(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, int iof, float* X, float* t, float* thr,
                     float drown, const float* prev_block, float* state_out, int B, int Kin, int F, int C, hipStream_t s);
int launch_inv_multi(const ac_mdct_plan* p, const float* X, void* x, int iof, const float* tail_in, float* tail_out,
                     int B, int Kp, int nblk, int C, hipStream_t s);

}  // namespace ac
