// The 16-byte kernels of the LDS-FFT tier (ac_wave_v.h, k_fwd_wave_v / k_inv_wave_v) instantiated for the two channels of a
// stereo signal (LAY = 0) -- on float32 and 16-bit PCM, with their launchers.  gfx950 only.
#include "ac_wave_v.h"

namespace ac {

int launch_fwd_wave_stereo(const ac_mdct_plan* p, const float* x, float* X, const float* prev_block, int B, int Kin, int F,
                           hipStream_t s) {
  return launch_fwd_wave_v<0>(p, x, X, prev_block, B, Kin, F, 2, s);
}
int launch_inv_wave_stereo(const ac_mdct_plan* p, const float* X, float* x, const float* tail_in, float* tail_out, int B, int Kp,
                           int nblk, hipStream_t s) {
  return launch_inv_wave_v<0>(p, X, x, tail_in, tail_out, B, Kp, nblk, 2, s);
}
int launch_fwd_wave_stereo_pcm16(const ac_mdct_plan* p, const int16_t* x, float* X, int B, int Kin, int F, hipStream_t s) {
  return launch_fwd_wave_v<0, int16_t>(p, x, X, nullptr, B, Kin, F, 2, s);
}
int launch_inv_wave_stereo_pcm16(const ac_mdct_plan* p, const float* X, int16_t* x, int B, int Kp, int nblk, hipStream_t s) {
  return launch_inv_wave_v<0, int16_t>(p, X, x, nullptr, nullptr, B, Kp, nblk, 2, s);
}

}  // namespace ac
