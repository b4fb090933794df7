// Instances and launch ladders of k_inv_fast / k_inv_fast_q: synthesis at filters_n = 1024 / 2048.
#include "ac_fast_inv_dev.h"

namespace ac {

// synthesis strips: short, so that the strips in flight cover a nearly contiguous window of memory (HBM rewards that:
// 0.42 ms at 15 blocks per strip, 0.38 ms at 4 with an extra DCT-IV per strip, 0.355-0.365 ms at 3 with the hand-over
// between the waves of a workgroup; B = 256, K = 468)
// (re-measured on well-placed tensors, DESIGN_LOG.md 9a: stereo N = 1024 0.343 ms at 2 blocks per strip against 0.352 at 3;
// N = 2048 0.373 at 3 against 0.396 at 2; mono N = 1024 0.190 at 3 against 0.197 at 2)
int pick_seglen(long long pairs, int frames, int preferred) {
  static const int fixed = [] {
    const char* e = getenv("AC_SEGLEN");   // tuning hook
    return e ? atoi(e) : 0;
  }();
  int s = fixed > 0 ? fixed : preferred;
  if (s > frames) s = frames;
  if (s < 1) s = 1;
  return s;
}

template <int R, int IOF>
static void launch_inv_R(const InvArgs& a, int C, unsigned grid, hipStream_t s) {
  const dim3 blk(AC_WAVES * 64);
  if (C == 2) hipLaunchKernelGGL((k_inv_fast<R, 0, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a);
  else if (C == 1) hipLaunchKernelGGL((k_inv_fast<R, 2, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a);
  else if constexpr (IOF != 2) hipLaunchKernelGGL((k_inv_fast<R, 1, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a);
}

int launch_inv_fast(const ac_mdct_plan* p, const float* X, void* x, int iof, const float* tail_in, float* tail_out,
                    int B, int Kp, int nblk, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || nblk <= 0) return AC_OK;
  if (fast_mdct_frames_per_wave(p->N) > 1) {
    if (!fast_multi_serves(p, C, iof, Kp)) {
      set_error("internal: no wave-level synthesis kernel for filters_n = %d, %d channels, io format %d here", p->N, C, iof);
      return AC_EUNSUPPORTED;
    }
    return launch_inv_multi(p, X, x, iof, tail_in, tail_out, B, Kp, nblk, C, s);
  }
  InvArgs a;
  unsigned grid;
  const int st = prep_inv_fast(p, X, x, iof, tail_in, tail_out, B, Kp, nblk, C, a, grid);
  if (st) return st;
  if (p->N == Geo<8>::FN) {
    if (iof == 2) launch_inv_R<8, 2>(a, C, grid, s);
    else if (iof == 1) launch_inv_R<8, 1>(a, C, grid, s);
    else launch_inv_R<8, 0>(a, C, grid, s);
  } else if (iof == 2) launch_inv_R<16, 2>(a, C, grid, s);
  else if (iof == 1) launch_inv_R<16, 1>(a, C, grid, s);
  else launch_inv_R<16, 0>(a, C, grid, s);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

// ---- synthesis from quantised spectra (k_inv_fast_q): filters_n 1024 / 2048, mono / stereo ----
bool fast_inv_quant_serves(const ac_mdct_plan* p, int C) {
  return p->fast && fast_mdct_frames_per_wave(p->N) == 1 && (C == 1 || C == 2);
}

template <int R, int IOF>
static void launch_inv_q_R(const InvArgs& a, const QuantRows& qr, int C, unsigned grid, hipStream_t s) {
  const dim3 blk(AC_WAVES * 64);
  if (C == 2) hipLaunchKernelGGL((k_inv_fast_q<R, 0, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a, qr);
  else hipLaunchKernelGGL((k_inv_fast_q<R, 2, AC_WAVES, IOF>), dim3(grid), blk, 0, s, a, qr);
}

int launch_inv_fast_quant(const ac_mdct_plan* p, const ac_psy_plan* psy, const int16_t* codes, const int8_t* sf, void* x,
                          bool pcm16, int B, int Kp, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || Kp <= 0) return AC_OK;
  if (!fast_inv_quant_serves(p, C) || psy->N != p->N) {
    set_error("internal: no synthesis from quantised spectra for filters_n = %d, %d channels", p->N, C);
    return AC_EUNSUPPORTED;
  }
  InvArgs a;
  unsigned grid;
  // (the spectrum pointer addresses the codes: the kernel reads it as int16)
  const int st = prep_inv_fast(p, reinterpret_cast<const float*>(codes), x, pcm16 ? 1 : 0, nullptr, nullptr, B, Kp, Kp + 1, C,
                               a, grid);
  if (st) return st;
  QuantRows qr;
  qr.sf = sf;
  qr.band32 = reinterpret_cast<const uint32_t*>(psy->d_qband);
  qr.M = psy->M;
  if (p->N == Geo<8>::FN) {
    if (pcm16) launch_inv_q_R<8, 4>(a, qr, C, grid, s);
    else launch_inv_q_R<8, 3>(a, qr, C, grid, s);
  } else if (pcm16) launch_inv_q_R<16, 4>(a, qr, C, grid, s);
  else launch_inv_q_R<16, 3>(a, qr, C, grid, s);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
