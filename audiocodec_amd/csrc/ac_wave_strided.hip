// The 16-byte kernels of the LDS-FFT tier (ac_wave_v.h, k_fwd_wave_v / k_inv_wave_v) instantiated for channel pairs of any
// channel count and rows anywhere on the 4-byte grid (LAY = 2), with their launchers.  gfx950 only.
#include "ac_wave_v.h"

namespace ac {

int launch_fwd_wave_strided(const ac_mdct_plan* p, const float* x, float* X, const float* prev_block, int B, int Kin, int F,
                            int C, hipStream_t s) {
  return launch_fwd_wave_v<2>(p, x, X, prev_block, B, Kin, F, C, s);
}
int launch_inv_wave_strided(const ac_mdct_plan* p, const float* X, float* x, const float* tail_in, float* tail_out, int B,
                            int Kp, int nblk, int C, hipStream_t s) {
  return launch_inv_wave_v<2>(p, X, x, tail_in, tail_out, B, Kp, nblk, C, s);
}

}  // namespace ac
