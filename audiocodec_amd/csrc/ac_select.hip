// The N loudest of S sources per clip and frame (k_select_loudest; DESIGN.md section 8j, "The selector"): energy and valid
// [S,B,F,C] -> active [S,B,F,C], the mask AC_IN_MIX and AC_IN_ROUTE take.  One wave owns one clip b and lane s holds source s, so
// the peak-hold chain along the frames runs in a register and a rank is S wave-uniform readlane compares.
//
// Per batch of SEL_AHEAD frames (one frame: see the constant):
//   fetch   E[s,b,f] = ((E'_0 + E'_1) + ...) over the channels, E'_c the energy where valid is non-zero and the energy > 0,
//           else +0 (NaN, negatives and -0 add +0; +Inf stays).  These loads do not depend on the chain: a batch's are all in
//           flight before its first chain step.
//   chain   d = fp32(P release); P = d > E ? d : E (a NaN d -- Inf times 0 -- gives E).  Source s is selected where P > gate and
//           fewer than n sources t have P_t > P_s or (P_t == P_s and t < s).
//   store   active = selected and valid != 0, one byte per channel.
// state [S,B] is read at entry and written at exit: in place, a wave owns its entries.
#include "ac_internal.h"

namespace ac {
namespace {

// frames whose loads are issued ahead of the chain.  Measured at B = 256, F = 469, stereo: 1 / 2 / 4 / 8 frames
// take 0.237 / 0.245 / 0.249 / 0.246 ms at S = 4 and 0.313 / 0.320 / 0.325 / 0.325 ms at S = 8, 1.38 / 1.38 / 1.38 / 1.42 ms at S = 64:
// batching as written here buys nothing, so a batch is one frame (about 0.5 us a frame: a clip's chain waits for its loads)
constexpr int SEL_AHEAD = 1;

struct SelectArgs {
  const float* energy;    // [S,B,F,C]
  const uint8_t* valid;   // [S,B,F,C] or null: all ones
  uint8_t* active;        // [S,B,F,C]
  float* state;           // [S,B] or null: zeros, nothing kept
  int S, B, F, C, n;
  float release, gate;
};

// grid: B workgroups of one wave
__global__ __launch_bounds__(64) void k_select_loudest(SelectArgs a) {
  const int lane = threadIdx.x, b = blockIdx.x;
  const bool on = lane < a.S;   // (lanes behind the last source load and store nothing and are never ranked)
  const size_t base = ((size_t)(on ? lane : 0) * (size_t)a.B + (size_t)b) * (size_t)a.F * (size_t)a.C;   // of frame 0
  float P = -1.f;
  if (on) P = a.state ? a.state[(size_t)lane * (size_t)a.B + (size_t)b] : 0.f;

#pragma unroll 1
  for (int f0 = 0; f0 < a.F; f0 += SEL_AHEAD) {
    float E[SEL_AHEAD];
#pragma unroll
    for (int d = 0; d < SEL_AHEAD; ++d) {
      E[d] = 0.f;
      if (on && f0 + d < a.F) {
        const size_t p = base + (size_t)(f0 + d) * (size_t)a.C;
        for (int c = 0; c < a.C; ++c) {
          const float e = a.energy[p + c];
          const bool ok = (!a.valid || a.valid[p + c] != 0) && e > 0.f;
          E[d] = E[d] + (ok ? e : 0.f);   // (+0 + x = x for every x >= +0: the sum starts at E'_0)
        }
      }
    }
    uint32_t sel = 0;
#pragma unroll
    for (int d = 0; d < SEL_AHEAD; ++d) {
      if (f0 + d < a.F) {   // (wave-uniform)
        const float dk = P * a.release;
        const float Pn = dk > E[d] ? dk : E[d];
        P = on ? Pn : P;
        int above = 0;
        for (int t = 0; t < a.S; ++t) {
          const float pt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(P), t));
          above += (pt > P || (pt == P && t < lane)) ? 1 : 0;
        }
        if (P > a.gate && above < a.n) sel |= 1u << d;
      }
    }
#pragma unroll
    for (int d = 0; d < SEL_AHEAD; ++d) {
      if (on && f0 + d < a.F) {
        const size_t p = base + (size_t)(f0 + d) * (size_t)a.C;
        const bool s = (sel >> d) & 1u;
        for (int c = 0; c < a.C; ++c) a.active[p + c] = (s && (!a.valid || a.valid[p + c] != 0)) ? 1 : 0;
      }
    }
  }
  if (on && a.state) a.state[(size_t)lane * (size_t)a.B + (size_t)b] = P;
}

}  // namespace

int launch_select(const float* energy, const uint8_t* valid, uint8_t* active, float* state, int S, int B, int F, int C, int n,
                  float release, float gate, hipStream_t s) {
  if (B <= 0 || S <= 0 || F <= 0 || C <= 0) return AC_OK;   // (no frame: state stays as it is)
  if (S > AC_SELECT_MAX_SOURCES) {
    set_error("internal: no selecting kernel for %d sources", S);
    return AC_EUNSUPPORTED;
  }
  SelectArgs a;
  a.energy = energy;
  a.valid = valid;
  a.active = active;
  a.state = state;
  a.S = S;
  a.B = B;
  a.F = F;
  a.C = C;
  a.n = n;
  a.release = release;
  a.gate = gate;
  hipLaunchKernelGGL(k_select_loudest, dim3((unsigned)B), dim3(64), 0, s, a);
  AC_HIP_CHECK(hipGetLastError());
  return AC_OK;
}

}  // namespace ac
