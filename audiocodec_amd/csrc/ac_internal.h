// Internal declarations shared by the translation units of libaudiocodec_amd.so.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/audiocodec_amd.h"
#include "../../include/audiocodec_amd_testing.h"
#include "ac_tables.h"

namespace ac {

void set_error(const char* fmt, ...);

#define AC_HIP_CHECK(expr)                                                                   \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      ac::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return AC_EHIP;                                                                        \
    }                                                                                        \
  } while (0)

#define AC_REQUIRE(cond, ...)      \
  do {                             \
    if (!(cond)) {                 \
      ac::set_error(__VA_ARGS__);  \
      return AC_EINVAL;            \
    }                              \
  } while (0)

// The kernels move rows with 16-byte (8-byte: mono, 16-bit PCM) vector accesses: tensor base addresses must be 16-byte
// aligned (any allocation is; a view that starts inside one may not be).
#define AC_REQUIRE_ALIGNED(...)                                                                                  \
  do {                                                                                                           \
    const void* ac_ptrs_[] = {__VA_ARGS__};                                                                      \
    for (const void* ac_p_ : ac_ptrs_)                                                                           \
      if ((reinterpret_cast<uintptr_t>(ac_p_) & 15) != 0) {                                                      \
        ac::set_error("tensor address %p is not 16-byte aligned (pass the start of an allocation or an aligned view)", ac_p_); \
        return AC_EINVAL;                                                                                        \
      }                                                                                                          \
  } while (0)

// Makes `device` current for the lifetime of the guard (no-op when it already is).
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) == hipSuccess && prev != device) {
      switched = (hipSetDevice(device) == hipSuccess);
    }
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

extern int g_force_generic;

// The device memory of a plan.  Every table goes up through upload(), which records what it allocates; release() frees all
// of it, so a plan's destroy needs no list of its own.
struct DeviceTables {
  std::vector<void*> owned;
  DeviceTables() = default;
  DeviceTables(const DeviceTables&) = delete;   // (one owner: a copied plan would free its tables twice)
  template <typename T>
  int upload(const std::vector<T>& h, T** d) {
    *d = nullptr;
    const size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
    AC_HIP_CHECK(hipMalloc((void**)d, bytes));
    owned.push_back(*d);
    if (!h.empty()) AC_HIP_CHECK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return AC_OK;
  }
  void release() {
    for (void* d : owned) (void)hipFree(d);
    owned.clear();
  }
};

// ---- element-wise pieces shared by the stand-alone utilities (ac_elementwise.hip) and the fused encode epilogue (ac_fast_psy_dev.h):
// one definition, so that fused and un-fused results agree bit for bit
// counter-based generator: a 64-bit mix (splitmix64) of (seed, pair index) -> Box-Muller, both outputs used:
// elements 2p and 2p+1 of the flattened tensor take R cos(theta) and R sin(theta)
__host__ __device__ inline uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
#ifdef __HIPCC__
__device__ __forceinline__ void normal_pair(uint64_t key, uint64_t pair, float& g0, float& g1) {
  const uint64_t r = mix64(key ^ pair);
  const float u1 = ((float)(uint32_t)(r >> 40) + 1.0f) * (1.0f / 16777216.0f);   // (0, 1]
  const float u2 = (float)(uint32_t)((r >> 8) & 0xFFFFFFu) * (1.0f / 16777216.0f);   // [0, 1): one revolution
  const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));   // sqrt(-2 ln u1)
  g0 = rad * __builtin_amdgcn_cosf(u2);   // v_cos_f32 / v_sin_f32 take revolutions
  g1 = rad * __builtin_amdgcn_sinf(u2);
}
// add_noise (psychoacoustic.py:150-167): x + thr * Normal(0, 1/6), g a standard normal
__device__ __forceinline__ float noisy_of(float x, float thr, float g) { return __builtin_fmaf(thr, g * (1.0f / 6.0f), x); }
// amplitude_to_dB (psychoacoustic.py:83-85) and its [0, 1] normalisation (:98-100): 10 log10 = 3.0103 log2 (v_log_f32)
__device__ __forceinline__ float db_of(float v, int norm) {
  float dB = __builtin_fmaf(3.0102999566398120f, __builtin_amdgcn_logf(fmaxf(1e-14f, v * v)), 120.f);
  // (the reference subtracts _dB_MIN = amplitude_to_dB(eps), the same expression, so its normalised scale starts at
  // exactly 0: the clamp keeps that under the rounding of the multiply-add above)
  if (norm) dB = fmaxf((dB + 20.f) * (1.0f / 140.f), 0.f);
  return dB;
}
// the 16-bit PCM store of every synthesis kernel (ac_fast_dev.h, ac_wave_v.h):
// pcm = 0 if x is NaN else clamp(rint(fp32(32768 x)), -32768, 32767), rint = round half to even; +-Inf and products that
// overflow float32 go to the rail of their sign.  (fmaxf(NaN, -32768) is -32768: without the select a NaN sample would
// store full-scale negative; the select leaves every other result as it was)
__device__ __forceinline__ short to_pcm16(float v) {
  const float r = fminf(fmaxf(v * 32768.0f, -32768.0f), 32767.0f);
  return (short)__float2int_rn(v != v ? 0.0f : r);
}
#endif

typedef __bf16 bf16_t;   // storage type of the AC_BF16 tensors (device code converts with v_cvt_pk_bf16_f32)
typedef _Float16 f16_t;  // storage type of the AC_F16 tensors (filter bank only)

// layout of the run-structured masking-model image and of its per-frame LDS slot (build_runs in ac_psy_mid_plan.hip; the fields
// are those of runs::RunsParams, ac_psy_runs_dev.h)
struct RunsLayout {
  int words = 0;
  int lw = 0, kb = 0, n4 = 0, n16 = 0, n64 = 0, o4 = 0, o16 = 0, o64 = 0, oz = 0, slot = 0;
  int off_S = 0, off_bc = 0, off_bd = 0, off_lst = 0, off_bw = 0, off_idx = 0;
};

}  // namespace ac

// ---- plan objects ---------------------------------------------------------------------------

struct ac_mdct_plan {
  int N = 0, window = 0, device = 0;
  ac::DeviceTables tables;     // owns every d_* below
  int cus = 0;                // compute units of the device (sizes the persistent launches)
  int fast = 0;                // 1: wave-level FFT kernels available for this N
  int pre = AC_F64;            // arithmetic type the constants were computed in (the reference's precompute_dtype)
  int fold4 = 0;               // 1: the wave-level kernels run their FOLD4 form (fold blocks that are not rotations)
  int adjoint = 0;             // 1: a plan made by ac_mdct_plan_adjoint (the transposed filter bank of another plan)
  ac::FoldCoef coef;           // the plan's fold coefficients (host copy)
  float* d_coef = nullptr;     // [8][N/2]  a1 a2 a3 a4 s1 s2 s3 s4
  float* d_coefv = nullptr;    // the same coefficients in the order of the 16-byte wave kernels (k_fwd_wave_v / k_inv_wave_v), N % 4 == 0
  float* d_ctab = nullptr;     // [8N]      cos(pi i / (4N)), generic kernels
  double* d_coef64 = nullptr;  // the same two tables in float64 (AC_F64 entry points)
  double* d_ctab64 = nullptr;
  // fast-path tables (ac_fast_plan.hip): per-FFT-element fold coefficients and twiddles
  float* d_fast = nullptr;
  size_t fast_bytes = 0;
};

struct ac_psy_plan {
  int N = 0, M = 0, device = 0;
  ac::DeviceTables tables;     // owns every d_* below
  double sample_rate = 0, alpha = 0;
  int fast = 0;                // 1: the fused wave-level epilogue supports this (N, M, table shape)
  int pre = AC_F64;            // arithmetic type the constants were computed in (the reference's precompute_dtype)
  int spread = 0;              // AC_SPREAD_*: form of the band x band spreading product in the wave-level kernels
  ac::PsyTables host;
  int32_t* d_wb_ptr = nullptr; int32_t* d_wb_idx = nullptr; float* d_wb_val = nullptr; int wb_max = 0;
  int32_t* d_wi_ptr = nullptr; int32_t* d_wi_idx = nullptr; float* d_wi_val = nullptr; int wi_max = 0;
  // transposed walks for the backward pass: W by bin, W_inv by band
  int32_t* d_wf_ptr = nullptr; int32_t* d_wf_idx = nullptr; float* d_wf_val = nullptr;
  int32_t* d_vb_ptr = nullptr; int32_t* d_vb_idx = nullptr; float* d_vb_val = nullptr;
  float* d_S = nullptr;        // [M, M]
  float* d_quiet = nullptr;    // [M]
  float* d_beta = nullptr;     // [M]
  // float64 constants (AC_F64 entry points): CSR values, S, quiet, beta = linspace(0, max_bark, M) in float64
  double* d_wb_val64 = nullptr; double* d_wi_val64 = nullptr;
  double* d_wf_val64 = nullptr; double* d_vb_val64 = nullptr;   // ... of the transposed walks (backward in float64)
  double* d_S64 = nullptr; double* d_quiet64 = nullptr; double* d_beta64 = nullptr;
  // fast-path tables (ac_fast_plan.hip)
  float* d_fast = nullptr;
  size_t fast_bytes = 0;
  // wave-level masking model for general band layouts (ac_psy_mid.hip): any even filter_bands_n <= 1024, <= 64 bands
  int mid = 0;
  uint32_t* d_mid = nullptr;
  int mid_words = 0;
  int mid_wi_w = 0, mid_off_S = 0, mid_off_band = 0, mid_off_wbe = 0, mid_off_wi = 0;   // layout of the image (build_mid, ac_psy_mid_plan.hip)
  // ... in its run-structured form (ac_psy_runs_dev.h): the form every kernel of that tier runs when the plan's tables have
  // the structure (runs = 1; the band walk above stays for tables that do not)
  int runs = 0;
  uint32_t* d_runs = nullptr;
  ac::RunsLayout runs_lay;
  int cus = 0;                 // compute units of the device (sizes the launches)
  // quantiser (ac_quant.hip): scale-factor band offsets [M+1] (ac::scale_bands) and the band of every bin [N] (uint16,
  // read as one 32-bit word per bin pair by the fused synthesis from codes)
  int32_t* d_qoff = nullptr;
  uint16_t* d_qband = nullptr;
  // row budget of a plan made by ac_psy_plan_with_row_budget (row_bits = 0: none): what ac_quantize and the quantising
  // encode meet, as ac_quantize_budget(row_bits, NULL, kmin) does
  int row_bits = 0, kmin = 0;
};

struct ac_stream {
  const ac_mdct_plan* plan = nullptr;
  int B = 0, C = 0;
  int N = 0, device = 0;           // copies of the plan's (the stream may outlive the plan object on teardown)
  float* d_prev_block = nullptr;   // analysis state  [B, N, C]
  float* d_prev_tmp = nullptr;     // double buffer for the analysis state (written by the kernel that reads the other)
  float* d_tail = nullptr;         // synthesis state [B, C, N/2]  (u_last[h .. N-1])
  float* d_tail_tmp = nullptr;     // double buffer for the synthesis state
  // the buffers swap roles with every chunk; "home" = the pair the state is moved back to by ac_stream_settle (and by
  // ac_stream_run on entry and exit, and by ac_stream_reset), so that launches captured into a HIP graph address the
  // state where a later replay will find it
  float* d_prev_home = nullptr;
  float* d_tail_home = nullptr;
  // float64 streams (AC_F64 through ac_stream_*_typed): the same state in double, allocated by the first float64 call
  double* d_prev64 = nullptr;      // [B, N, C]
  double* d_tail64 = nullptr;      // [B, C, N/2]
  double* d_tail64_tmp = nullptr;
  // concealment across chunks (AC_PACKED | AC_CONCEAL), allocated by the first concealing call: one
  // buffer holding the carried rows twice, then the gaps twice; half conceal_cur is current.  conceal_stale: the last call that
  // advanced d_tail did not conceal (or the stream is new or was reset), so the next concealing call reads every gap as 32
  uint8_t* d_conceal = nullptr;
  int conceal_cur = 0;
  bool conceal_stale = true;
  // the recovering decode of chunks ("Streams") synthesises one frame behind its rows.  delayed: a
  // recovering chunk has run since creation or the last reset, and every other call that advances the synthesis is refused;
  // advanced: such a call has run since then, and a recovering chunk is refused
  bool delayed = false;
  bool advanced = false;
};

// ---- kernel launchers (each returns an AC_* status) -----------------------------------------
namespace ac {

int check_grid(long long n);   // ac_mdct_generic.hip.  0: launch, 1: nothing to do, < 0: error (too many workgroups)
// ---- the tiers below the wave-level kernels: any even N, any C, any M.  One function per kernel family; `dtype` (AC_*) is the
// element type of the tensors behind the void pointers.  The C ABI checks it before it calls (AC_REQUIRE_DTYPE*).
// Filter bank (ac_mdct_generic.hip), AC_F32 / AC_F64 / AC_BF16 / AC_F16: the LDS-FFT tier where it serves, else the O(N^2)
// kernels.  The streaming state may be null: prev_block [B,N,C] of the tensors' type, block -1 of every signal; tail_in / tail_out
// [B,C,N/2], float (double for AC_F64): the aliased half of the frame before frame 0 in, of the last one out
int launch_fwd_typed(const ac_mdct_plan* p, const void* x, void* X, const void* prev_block, int dtype, int B, int Kin, int F, int C,
                     hipStream_t s);
int launch_inv_typed(const ac_mdct_plan* p, const void* X, void* x, const void* tail_in, void* tail_out, int dtype, int B, int Kp,
                     int nblk, int C, hipStream_t s);
int lds_fft_tier_of(const ac_mdct_plan* p, int C);   // ac_mdct_generic.hip: 2 / 1 / 0, see ac_mdct_plan_tier
// Masking model and its backward (ac_psy_generic.hip), AC_F32 / AC_F64 / AC_BF16; float64: everything in double on the float64
// tables, bfloat16: float32 arithmetic and tables
int launch_tonality_typed(const ac_psy_plan* p, const void* X, void* t, int dtype, int B, int F, int C, hipStream_t s);
int launch_threshold_typed(const ac_psy_plan* p, const void* X, const void* t, double drown, void* thr, int dtype, int B, int F,
                           int C, hipStream_t s);
int launch_tonality_bwd_typed(const ac_psy_plan* p, const void* X, const void* gt, void* gX, int accumulate, int dtype, int B, int F,
                              int C, hipStream_t s);
int launch_threshold_bwd_typed(const ac_psy_plan* p, const void* X, const void* t, double drown, const void* gthr, void* gX, void* gt,
                               int dtype, int B, int F, int C, hipStream_t s);
// Element-wise utilities (ac_elementwise.hip), AC_F32 / AC_F64 / AC_BF16; the backward of amplitude_to_dB is float32 only
int launch_db_typed(const void* a, void* out, size_t n, int norm, int dtype, hipStream_t s);
int launch_db_bwd(const float* a, const float* g, float* ga, size_t n, int norm, hipStream_t s);
int launch_add_noise_typed(const void* X, const void* thr, void* out, size_t n, uint64_t seed, int dtype, hipStream_t s);
// the 16-byte kernels of the LDS-FFT tier (ac_wave_v.h) on stereo rows (ac_wave_stereo.hip) ...
int launch_fwd_wave_stereo(const ac_mdct_plan* p, const float* x, float* X, const float* prev_block, int B, int Kin, int F,
                           hipStream_t s);
int launch_inv_wave_stereo(const ac_mdct_plan* p, const float* X, float* x, const float* tail_in, float* tail_out, int B, int Kp,
                           int nblk, hipStream_t s);
// ... on mono rows (ac_wave_mono.hip)
int launch_fwd_wave_mono(const ac_mdct_plan* p, const float* x, float* X, const float* prev_block, int B, int Kin, int F,
                         hipStream_t s);
int launch_inv_wave_mono(const ac_mdct_plan* p, const float* X, float* x, const float* tail_in, float* tail_out, int B, int Kp,
                         int nblk, hipStream_t s);
// 16-bit PCM at the boundary of the LDS-FFT tier (filters_n 120 / 240 / 480 / 960 / 1920 / 576 / 1152, mono / stereo)
bool lds_fft_serves_pcm16(const ac_mdct_plan* p, int C);
int launch_fwd_lds_pcm16(const ac_mdct_plan* p, const int16_t* x, float* X, int B, int K, int C, hipStream_t s);
int launch_inv_lds_pcm16(const ac_mdct_plan* p, const float* X, int16_t* x, int B, int Kp, int C, hipStream_t s);
int launch_fwd_wave_stereo_pcm16(const ac_mdct_plan* p, const int16_t* x, float* X, int B, int Kin, int F, hipStream_t s);
int launch_inv_wave_stereo_pcm16(const ac_mdct_plan* p, const float* X, int16_t* x, int B, int Kp, int nblk, hipStream_t s);
int launch_fwd_wave_mono_pcm16(const ac_mdct_plan* p, const int16_t* x, float* X, int B, int Kin, int F, hipStream_t s);
int launch_inv_wave_mono_pcm16(const ac_mdct_plan* p, const float* X, int16_t* x, int B, int Kp, int nblk, hipStream_t s);
// the fused encode of the LDS-FFT tier (ac_wave_enc.hip): the 16-byte analysis kernels with the run-structured masking model
// on the frame while it is in LDS; filters_n 108 ... 4096 with an instance, float32 mono / stereo
bool wave_encode_fuses(const ac_mdct_plan* p, const ac_psy_plan* psy, int C, const void* x, const void* X, const void* thr);
int launch_enc_wave(const ac_mdct_plan* p, const ac_psy_plan* psy, const float* x, float* X, float* t, float* thr, float drown,
                    const float* prev_block, int B, int Kin, int F, int C, hipStream_t s);
// ... and on channel pairs of three or more channels: whole rows through LDS where the shape has that form (ac_wave_team.hip;
// kTeamDeclined: it has not), the strided channel pairs elsewhere and on rows off the 16-byte grid (ac_wave_strided.hip)
constexpr int kTeamDeclined = -12346;
int launch_fwd_wave_team(const ac_mdct_plan* p, const float* x, float* X, const float* prev_block, int B, int Kin, int F, int C,
                         hipStream_t s);
int launch_inv_wave_team(const ac_mdct_plan* p, const float* X, float* x, const float* tail_in, float* tail_out, int B, int Kp,
                         int nblk, int C, hipStream_t s);
int launch_fwd_wave_strided(const ac_mdct_plan* p, const float* x, float* X, const float* prev_block, int B, int Kin, int F,
                            int C, hipStream_t s);
int launch_inv_wave_strided(const ac_mdct_plan* p, const float* X, float* x, const float* tail_in, float* tail_out, int B,
                            int Kp, int nblk, int C, hipStream_t s);

// wave-level FFT kernels (ac_fast_*.hip; what they share among themselves: ac_fast.h)
bool fast_mdct_supported(int N, const FoldCoef& c);
// filters_n 512 / 256 run several frames per wave (2 / 4); those kernels serve float32 mono / stereo tensors with at least
// one block (streaming state included) -- everything else at these sizes takes the LDS-FFT tier
int fast_mdct_frames_per_wave(int N);
bool fast_multi_serves(const ac_mdct_plan* p, int C, int iof, int blocks);
// ... and whether the masking model of `psy` (general band layouts, ac_psy_mid_dev.h) rides in the same launch
bool fast_multi_fuses(const ac_mdct_plan* p, const ac_psy_plan* psy, int C, int iof, int blocks);
bool fast_psy_supported(const ac_psy_plan* p);
int fast_mdct_plan_init(ac_mdct_plan* p);
int fast_psy_plan_init(ac_psy_plan* p);
// psy may be null (plain transform).  X/t/thr as in ac_encode_fused.
// iof: 0 = float32 tensors; 1 = int16 PCM on the PCM side (x), spectra float32; 2 = bfloat16 tensors throughout (every
// pointer then addresses 2-byte elements; C = 1 or 2 only).  prev_block / tail state must be null unless iof == 0
// state_out (iof == 0 only): receives block Kin-1 of every signal, the next chunk's prev_block (must not alias prev_block)
int launch_fwd_fast(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, int iof, float* X, float* t,
                    float* thr, float drown, const float* prev_block, int B, int Kin, int F, int C, hipStream_t s,
                    float* state_out = nullptr, float* noisy = nullptr, float* dbn = nullptr, uint64_t seed = 0);
// noisy / dbn (either may be null): the element-wise epilogues of ac_encode_fused_ex, where fast_epilogue_supported()
bool fast_epilogue_supported(const ac_mdct_plan* p, const ac_psy_plan* psy, int iof, int C);
// The fused encode at filters_n = 1024 that quantises in the same launch (ac_fast_quant_dev.h, ac_fast_fwd_qp_dev.h): float32
// or 16-bit PCM, mono / stereo, f32 or split-bf16 spreading, 64 bands.  Eight kernels, a unit each (ac_fast_fwd_q*.hip), one
// host launcher (launch_fwd_fast_quant_family).  x is float32, in the *_pcm16 forms int16, read as pcm / 32768 in the row
// loads: their outputs equal the float32 launch's on pcm.to(float32) / 32768 bit for bit.  A call the unit does not serve is
// refused with an "internal:" error.
//   quant           k_fwd_fast_q / q16: codes int16 [B,F,N,C] and sf int8 [B,F,M,C] equal launch_quantize on launch_fwd_fast's
//                   X and thr bit for bit; X, t and thr may each be null (not written)
//   quant_budget    k_fwd_fast_qb / qb16, a plan with a row budget: ... equal launch_quantize_budget(psy->row_bits, nullptr,
//                   psy->kmin) on them
//   pack_rows       k_fwd_fast_qp / qp16, a budget of at most kPackRowsMaxBits: data [B F C row_bytes] and fits [B,F,C] are all
//                   it writes; row r = (b F + f) C + c at byte r row_bytes, row_bytes = plan_row_bytes(psy), holds what
//                   launch_pack writes for quant_budget's codes and sf, zero-padded, or the marked row (every width 31) where
//                   that is longer than the slot
//   pack_rows_stream  k_fwd_fast_qps / qps16, a chunk of k blocks of a stream: k frames per signal, frame 0 pairs block 0 with
//                   prev_block [B,N,C] (float32 whatever x is); state_out (another buffer) receives block k - 1.  Serves where
//                   pack_rows does and its own instance passed the register gate
constexpr int kPackRowsMaxBits = AC_PACK_ROWS_MAX_BITS;
inline int64_t plan_row_bytes(const ac_psy_plan* psy) { return (int64_t)((psy->row_bits + 31) / 32) * 4; }   // ceil(row_bits / 32) * 4
bool fast_encode_quant_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C);   // quant, quant_budget, their pcm16 forms
bool fast_encode_pack_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C);    // pack_rows, pack_rows_pcm16
bool fast_encode_pack_stream_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C);
bool fast_encode_pack_stream_pcm16_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C);
int launch_fwd_fast_quant(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float* X, float* t, float* thr,
                          float drown, int16_t* codes, int8_t* sf, int B, int Kin, int F, int C, hipStream_t s);
int launch_fwd_fast_quant_budget(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float* X, float* t, float* thr,
                                 float drown, int16_t* codes, int8_t* sf, int B, int Kin, int F, int C, hipStream_t s);
int launch_fwd_fast_pack_rows(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float drown, uint8_t* data,
                              int64_t row_bytes, uint8_t* fits, int B, int Kin, int F, int C, hipStream_t s);
int launch_fwd_fast_pack_rows_stream(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float drown, uint8_t* data,
                                     int64_t row_bytes, uint8_t* fits, const float* prev_block, float* state_out, int B, int k,
                                     int C, hipStream_t s);
int launch_fwd_fast_quant_pcm16(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float* X, float* t, float* thr,
                                float drown, int16_t* codes, int8_t* sf, int B, int Kin, int F, int C, hipStream_t s);
int launch_fwd_fast_quant_budget_pcm16(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float* X, float* t,
                                       float* thr, float drown, int16_t* codes, int8_t* sf, int B, int Kin, int F, int C,
                                       hipStream_t s);
int launch_fwd_fast_pack_rows_pcm16(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float drown, uint8_t* data,
                                    int64_t row_bytes, uint8_t* fits, int B, int Kin, int F, int C, hipStream_t s);
int launch_fwd_fast_pack_rows_stream_pcm16(const ac_mdct_plan* p, const ac_psy_plan* psy, const void* x, float drown,
                                           uint8_t* data, int64_t row_bytes, uint8_t* fits, const float* prev_block,
                                           float* state_out, int B, int k, int C, hipStream_t s);
int launch_inv_fast(const ac_mdct_plan* p, const float* X, void* x, int iof, const float* tail_in, float* tail_out,
                    int B, int Kp, int nblk, int C, hipStream_t s);
// synthesis straight from quantised spectra (codes int16 [B,Kp,N,C], sf int8 [B,Kp,M,C]; ac_quant.hip), filters_n 1024 /
// 2048, mono / stereo: the frames are dequantised in the loads, bit-equal to launch_inv_fast on launch_dequantize's output
bool fast_inv_quant_serves(const ac_mdct_plan* p, int C);
int launch_inv_fast_quant(const ac_mdct_plan* p, const ac_psy_plan* psy, const int16_t* codes, const int8_t* sf, void* x,
                          bool pcm16, int B, int Kp, int C, hipStream_t s);
// ... and from rows of the packed bitstream (k_inv_fast_p, ac_fast_inv_p.hip): filters_n = 1024 with 64 bands, mono / stereo;
// data [nbytes], index [B,Kp,C]; bit-equal to launch_inv_fast_quant on launch_unpack's output, damaged rows included.
// nblk = Kp + 1 with null tails: the one-shot synthesis; nblk = Kp with the stream's tail buffers: a chunk of a stream
bool fast_inv_packed_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C);
int launch_inv_fast_packed(const ac_mdct_plan* p, const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes,
                           const int64_t* index, void* x, bool pcm16, const float* tail_in, float* tail_out, int B, int Kp,
                           int nblk, int C, hipStream_t s);
// ... with the rows marked in lost [B,Kp,C] (nonzero: did not arrive) concealed (k_inv_fast_pl, ac_fast_inv_pl.hip; DESIGN.md
// section 8f), where fast_inv_packed_serves(); the one-shot synthesis only.  max_age in [0, AC_CONCEAL_MAX_AGE]
int launch_inv_fast_packed_conceal(const ac_mdct_plan* p, const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes,
                                   const int64_t* index, const uint8_t* lost, int max_age, void* x, bool pcm16, int B, int Kp,
                                   int C, hipStream_t s);
// ... and a lost row whose successor arrived read from index[b,f+1,c] + redundant_at, the redundant copy of a protected slot
// (k_inv_fast_plr, ac_fast_inv_plr.hip), where fast_inv_packed_serves(); redundant_at in [1, 2^31)
int launch_inv_fast_packed_recover(const ac_mdct_plan* p, const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes,
                                   const int64_t* index, const uint8_t* lost, int max_age, int64_t redundant_at, void* x,
                                   bool pcm16, int B, int Kp, int C, hipStream_t s);
// ... as one chunk of k frames of a stream (k_inv_fast_pls, ac_fast_inv_pls.hip): tails as launch_inv_fast_packed takes them,
// and the concealment state -- gap [B,C] and carried rows [B,C] at conceal_state_row_bytes(1, 1) bytes each -- read from
// gap_in / row_in (stale: every gap reads as 32, nothing is read) and written to gap_out / row_out, other buffers
bool fast_inv_packed_conceal_stream_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C);
size_t conceal_state_row_bytes(int B, int C);
int launch_inv_fast_packed_conceal_stream(const ac_mdct_plan* p, const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes,
                                          const int64_t* index, const uint8_t* lost, int max_age, void* x, bool pcm16,
                                          const float* tail_in, float* tail_out, const uint8_t* gap_in, const uint8_t* row_in,
                                          uint8_t* gap_out, uint8_t* row_out, bool stale, int B, int k, int C, hipStream_t s);
// ... recovering first, as launch_inv_fast_packed_recover does one-shot (k_inv_fast_plsr, ac_fast_inv_plsr.hip; DESIGN.md section
// 8g, "Streams"): the k blocks are the frames of the deferred row -- the last row of the chunk before, which the state carries
// where gap_in is 0 -- and of rows 0 .. k-2; the state written is the one launch_inv_fast_packed_conceal_stream writes
bool fast_inv_packed_recover_stream_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int C);
int launch_inv_fast_packed_recover_stream(const ac_mdct_plan* p, const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes,
                                          const int64_t* index, const uint8_t* lost, int max_age, int64_t redundant_at, void* x,
                                          bool pcm16, const float* tail_in, float* tail_out, const uint8_t* gap_in,
                                          const uint8_t* row_in, uint8_t* gap_out, uint8_t* row_out, bool stale, int B, int k,
                                          int C, hipStream_t s);
int launch_psy_fast(const ac_psy_plan* p, const float* X, const float* t_in, float* t_out, float* thr, float drown,
                    int B, int F, int C, hipStream_t s, int iof = 0);
// streaming duplex: the analysis of a chunk of k_fwd blocks (psy: with the fused masking model) and the synthesis of a
// chunk of k_inv frames in one launch, where fast_duplex_serves() -- small float32 mono / stereo launches
bool fast_duplex_serves(const ac_mdct_plan* p, const ac_psy_plan* psy, int B, int C, int k_fwd, int k_inv);
int launch_duplex_fast(const ac_mdct_plan* p, const ac_psy_plan* psy, const float* x, float* X, float* t, float* thr,
                       float drown, const float* prev_block, float* state_out, int k_fwd, const float* X_inv, float* x_inv,
                       const float* tail_in, float* tail_out, int k_inv, int B, int C, hipStream_t s);

// wave-level masking model for general band layouts; float32, any channel count.  The plan's side (ac_psy_mid_plan.hip) ...
bool mid_psy_supported(const ac_psy_plan* p);
int mid_psy_plan_init(ac_psy_plan* p);
// the run-structured image of a model's tables, built on the host (no device needed): false when the tables lack the
// structure (ac_psy_runs_dev.h); runs_psy_plan_init uploads it
bool build_runs(const PsyTables& t, std::vector<uint32_t>* out, RunsLayout* lay);
int runs_psy_plan_init(ac_psy_plan* p);
// ... and the launch (ac_psy_mid.hip): the run-structured form where the plan has its image, else the band walk.
// t_out != null: tonality (from X); thr != null: threshold (from t_out when given, else from t_in)
int launch_psy_mid(const ac_psy_plan* p, const float* X, const float* t_in, float* t_out, float* thr, float drown, int B,
                   int F, int C, hipStream_t s);

// wave-level backward: tonality backward when g_thr is null, else threshold backward
int launch_psy_bwd_fast(const ac_psy_plan* p, const float* X, const float* t, float drown, const float* g_thr,
                        const float* g_t, float* g_X, float* g_t_out, int accumulate, int B, int F, int C,
                        hipStream_t s);
// Launch geometry of the quantiser, pack and rate kernels: grid (B*F rows, channel groups), a block of whole waves.
constexpr int kRowThreads = 256;   // the most threads of a block: the __launch_bounds__ of every kernel row_launch serves
struct RowLaunch {
  long long rows;   // B * F
  int threads;      // the row's bins rounded up to whole waves, at most kRowThreads
  int CG, groups;   // channels per workgroup, workgroups per row
  int cgt;          // the kernels' CGT: C where one group is the whole of one or two channels, else 0
  dim3 grid() const { return dim3((unsigned)rows, (unsigned)groups); }
};
// as many channels per group as lds_budget bytes hold at lds_per_channel bytes each, at least one
inline int lds_group(int C, int lds_budget, int lds_per_channel) {
  return std::max(1, std::min(C, lds_budget / lds_per_channel));
}
// Fills *out for [B,F,N,C] in groups of CG channels.  rows_per_clip >= 0 is checked and reported with the rows.
inline int row_launch(const ac_psy_plan* p, int B, int F, int C, int CG, RowLaunch* out, long long rows_per_clip = -1) {
  out->rows = (long long)B * F;
  if (out->rows > 2147483647ll || rows_per_clip > 2147483647ll) {
    char per_clip[48] = "";
    if (rows_per_clip >= 0) snprintf(per_clip, sizeof per_clip, ", %lld rows per clip", rows_per_clip);
    set_error("problem too large for one launch (%lld rows%s)", out->rows, per_clip);
    return AC_EINVAL;
  }
  out->threads = std::min(kRowThreads, (p->N + 63) / 64 * 64);
  out->CG = CG;
  out->groups = (C + CG - 1) / CG;
  out->cgt = (CG == C && C <= 2) ? C : 0;
  return AC_OK;
}

// quantiser (ac_quant.hip): X, thr [B,F,N,C] -> codes int16 [B,F,N,C], sf int8 [B,F,M,C], and back
int launch_quantize(const ac_psy_plan* p, const float* X, const float* thr, int16_t* codes, int8_t* sf, int B, int F, int C,
                    hipStream_t s);
int launch_dequantize(const ac_psy_plan* p, const int16_t* codes, const int8_t* sf, float* X, int B, int F, int C, hipStream_t s);
// rate control (ac_rate.hip): the quantiser at the smallest offset in [kmin, 254] whose packed row fits the row's budget
// (row_budget [B,F,C] int32, or the scalar budget where it is NULL) -> codes, sf, offset int16 [B,F,C] (or NULL), row_bits (or NULL)
int launch_quantize_budget(const ac_psy_plan* p, const float* X, const float* thr, int budget, const int32_t* row_budget,
                           int kmin, int16_t* codes, int8_t* sf, int16_t* offset, int32_t* row_bits, int B, int F, int C,
                           hipStream_t s);
// the requantiser (ac_requant.hip): launch_quantize_budget's search on rows that are already quantised
// -- the stored sf for sf0, fp32(code * step(sf)) for X; kmin in [0, 254]; the inputs must not overlap the outputs
int launch_requantize_budget(const ac_psy_plan* p, const int16_t* codes_in, const int8_t* sf_in, int budget,
                             const int32_t* row_budget, int kmin, int16_t* codes, int8_t* sf, int16_t* offset,
                             int32_t* row_bits, int B, int F, int C, hipStream_t s);
// ... from packed rows to fixed-stride packed rows at the plan's row budget in one launch (k_transrate_p, ac_transrate.hip):
// rows of data [nbytes] at index [rows] -> out [rows row_bytes], fits [rows], offset [rows] (or NULL); the bytes of
// launch_unpack, launch_requantize_budget(row_bits, nullptr, 0), rows longer than the slot marked, launch_pack at
// r row_bytes into zero-filled data.  Serves float32 plans with N = 1024, M = 64 and a budget of at most kPackRowsMaxBits
bool transrate_serves(const ac_psy_plan* psy);
int launch_transrate(const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes, const int64_t* index, uint8_t* out,
                     int64_t row_bytes, uint8_t* fits, int16_t* offset, long long rows, hipStream_t s);
// ... of several sources summed bin by bin (k_mix_p, ac_mix.hip): src [sources_n] (host) holds data, nbytes
// and index [rows] of every source, gain [sources_n] (host, or NULL: zeros) its scale-factor units, active [sources_n][rows]
// (device, or NULL) which rows are read; out, fits, offset as launch_transrate's.  Where transrate_serves() and sources_n in
// [1, AC_MIX_MAX_SOURCES]
bool mix_serves(const ac_psy_plan* psy, int sources_n);
int launch_mix(const ac_psy_plan* psy, int sources_n, const ac_packed_rows* src, const int32_t* gain, const uint8_t* active,
               uint8_t* out, int64_t row_bytes, uint8_t* fits, int16_t* offset, long long rows, hipStream_t s);
// ... and routed into outputs_n mixes, every source row read once (k_route_p, ac_route.hip): gain
// [outputs_n * sources_n] (host) holds AC_ROUTE_MUTE where output o does not hear source i; out [outputs_n][rows row_bytes], fits
// and offset (or NULL) [outputs_n][rows].  Where transrate_serves(), sources_n in [1, AC_ROUTE_MAX_SOURCES] and outputs_n in
// [1, AC_ROUTE_MAX_OUTPUTS]
bool route_serves(const ac_psy_plan* psy, int sources_n, int outputs_n);
int launch_route(const ac_psy_plan* psy, int sources_n, int outputs_n, const ac_packed_rows* src, const int32_t* gain,
                 const uint8_t* active, uint8_t* out, int64_t row_bytes, uint8_t* fits, int16_t* offset, long long rows,
                 hipStream_t s);
// ... and to protected slots (k_protect_p, ac_protect.hip): slot r of out [rows (row_bytes + red_bytes)]
// holds launch_transrate's slot of row r, then -- for f >= 1 -- its slot of row r - C at the budget red_bits (zeros at f = 0);
// fits, red_fits [rows], offset, red_offset [rows] (or NULL).  Where transrate_serves() and red_bits in [5 M, kPackRowsMaxBits]
bool protect_serves(const ac_psy_plan* psy, int red_bits);
int launch_protect(const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes, const int64_t* index, uint8_t* out,
                   int64_t row_bytes, int red_bits, uint8_t* fits, uint8_t* red_fits, int16_t* offset, int16_t* red_offset, int B,
                   int F, int C, hipStream_t s);
// ... as one chunk of F frames of a stream (k_protect_ps, ac_protect_s.hip; DESIGN.md section 8g, "Streams"): the frame-0 slots
// take the copy, fits and offset the chunk before left in row_in [B,C,red_bytes], fits_in, offset_in [B,C] (row_in NULL: a fresh
// stream, zeros as above), and the copy of frame F - 1 goes to row_out, fits_out, offset_out, other buffers
int launch_protect_stream(const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes, const int64_t* index, uint8_t* out,
                          int64_t row_bytes, int red_bits, uint8_t* fits, uint8_t* red_fits, int16_t* offset, int16_t* red_offset,
                          const uint8_t* row_in, const uint8_t* fits_in, const int16_t* offset_in, uint8_t* row_out,
                          uint8_t* fits_out, int16_t* offset_out, int B, int F, int C, hipStream_t s);
// The level of packed rows (k_level_p, ac_level.hip): energy [rows] = the sum of X^ squared over the row's
// bins in the section's arithmetic, bad [rows] (or NULL) = 1 where a band of the row has sf = -128.  Where N = 1024 and M = 64,
// with or without a row budget
bool level_serves(const ac_psy_plan* psy);
int launch_level(const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes, const int64_t* index, float* energy, uint8_t* bad,
                 long long rows, hipStream_t s);
// ... and the n loudest of S <= AC_SELECT_MAX_SOURCES sources per clip and frame (k_select_loudest, ac_select.hip): energy, valid
// (or NULL: all ones) and active [S,B,F,C], state [S,B] (or NULL) read and written in place
int launch_select(const float* energy, const uint8_t* valid, uint8_t* active, float* state, int S, int B, int F, int C, int n,
                  float release, float gate, hipStream_t s);
// rate control per clip (ac_clip_rate.hip): one budget for the F*C rows of a clip (clip_budget [B] int64,
// or the scalar budget where it is NULL); row_bits, clip_offset and clip_bits may be NULL; scratch of
// clip_budget_scratch_bytes(p, B, F*C) bytes
size_t clip_budget_scratch_bytes(const ac_psy_plan* p, long long B, long long rows_per_clip);
int launch_quantize_clip_budget(const ac_psy_plan* p, const float* X, const float* thr, int64_t budget,
                                const int64_t* clip_budget, int kmin, int16_t* codes, int8_t* sf, int16_t* offset,
                                int32_t* row_bits, int16_t* clip_offset, int64_t* clip_bits, void* scratch, int B, int F, int C,
                                hipStream_t s);
// packed bitstream (ac_pack.hip): codes, sf -> index [B,F,C] (row byte offsets) + total, data; and back
size_t pack_scratch_bytes(long long rows);
int launch_pack_index(const ac_psy_plan* p, const int16_t* codes, const int8_t* sf, int64_t* index, int64_t* total,
                      void* scratch, int B, int F, int C, hipStream_t s);
int launch_pack(const ac_psy_plan* p, const int16_t* codes, const int8_t* sf, const int64_t* index, uint8_t* data, int B,
                int F, int C, hipStream_t s);
int launch_unpack(const ac_psy_plan* p, const uint8_t* data, int64_t nbytes, const int64_t* index, int16_t* codes, int8_t* sf,
                  int B, int F, int C, hipStream_t s);

}  // namespace ac
