/*
 * audiocodec_amd.h -- C ABI of the MI355X (gfx950) MDCT + psychoacoustic-masking library.
 *
 * The reference (korneelvdbroek/audiocodec) has no FFI: its boundary is the Python API of
 * audiocodec/mdctransformer.py and audiocodec/psychoacoustic.py, whose arithmetic is delegated to
 * TensorFlow ops.  Each entry point below replaces the TensorFlow op sequence of one reference
 * method (cited as file:line into the reference tree); INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add to bind them.
 *
 * Conventions
 *  - plain C types only; device pointers are raw HIP device addresses owned by the caller;
 *  - tensor layouts are exactly the reference's, contiguous, float32, channels innermost:
 *        PCM        x   [B, S, C]        S = K * N samples        (mdctransformer.py:104)
 *        spectrum   X   [B, F, N, C]     F frames of N filters    (mdctransformer.py:105-107)
 *        tonality   t   [B, F, 1, C]                              (psychoacoustic.py:110)
 *        threshold  thr [B, F, N, C]                              (psychoacoustic.py:134-135)
 *    PCM, spectrum and threshold tensors start at 16-byte aligned addresses (any allocation does; a view that starts
 *    inside one may not): the kernels move rows with 16- and 8-byte vector accesses.  AC_EINVAL otherwise;
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call only
 *    enqueues work and returns without synchronising; the library never allocates, frees or
 *    synchronises caller memory and never changes the current device outside *_create;
 *  - return value 0 = AC_OK, negative = error; ac_last_error() gives a thread-local message;
 *  - plans are immutable after creation and may be shared between host threads and streams.
 *
 * Performance note (MI355X): the kernels stream their tensors at the device's copy rate, and that rate depends on where
 * the caller's buffers live -- when the two tensors a kernel streams side by side (X and thr for ac_encode_fused, X
 * and x for ac_mdct_inverse) sit in stretches of VRAM of the same class, the kernel runs up to 15 % slower.
 * ac_workspace_create (below) hands out buffers placed by timing the encode kernel on a few candidate allocations; the
 * Python package draws the tensors its encode() / decode() return from such a workspace (audiocodec_amd/placement.py).
 */
#ifndef AUDIOCODEC_AMD_H
#define AUDIOCODEC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared in this header (and the test hook of
 * audiocodec_amd_testing.h) are its only dynamic symbols. */
#ifndef AC_API
#define AC_API __attribute__((visibility("default")))
#endif

#define AC_VERSION 171 /* 0.1.8 + the quantiser (int16 codes, int8 per-band scale factors: ac_quantize, ac_dequantize,
                          * ac_decode_quantized[_launches], ac_psy_scale_bands_host), its packed bitstream (ac_pack_index,
                          * ac_pack, ac_unpack, ac_pack_scratch_bytes; decoded in one launch: ac_packed_rows,
                          * ac_decode_packed_launches) and its rate control (ac_quantize_budget, per clip
                          * ac_quantize_clip_budget, ac_clip_budget_scratch_bytes; in the plan: ac_psy_plan_with_row_budget,
                          * ac_psy_plan_row_budget; packed rows in a stream: AC_PACKED, ac_stream_packed_in,
                          * ac_stream_packed_launches; 16-bit PCM into the quantising encodes: AC_IN_PCM16,
                          * ac_*_launches_pcm16; rows to a lower budget without decoding: ac_quantized_rows, AC_IN_PACKED,
                          * ac_transrate_launches; lost rows concealed in a stream: AC_CONCEAL,
                          * ac_stream_packed_lost_in; protected rows and the decode that recovers from them:
                          * AC_EMIT_REDUNDANT, ac_protected_out, ac_protect_launches, AC_CONCEAL_REDUNDANT,
                          * ac_conceal_redundant; the recovering decode chunk by chunk: ac_stream_packed_recover_in,
                          * and protecting chunk by chunk: AC_EMIT_CARRY, ac_protect_carry, ac_protect_chunk_launches; rows
                          * of several sources mixed without decoding: AC_IN_MIX, ac_mix_rows, ac_mix_launches; and routed
                          * to several mixes: AC_IN_ROUTE, ac_route_rows, ac_route_launches; the level of packed rows and
                          * the loudest sources: AC_EMIT_LEVEL, ac_level_launches, AC_SELECT_ACTIVE, ac_select_rows);
                          * additions only, so the number stays.
                          * 0.1.8: ac_mdct_plan_tier; 16-bit PCM at the Opus / MP3 frame lengths; the LDS-FFT tier on 16-byte kernels with compile-time instances (filters_n % 4 == 0
                          * with a 5-smooth half up to 8192, float32); masking model for general band layouts up to 4096 bins.
                          * 0.1.7: only the ac_* entry points are exported; ac_stream_settle (home buffers for the streaming state);
                          * float32 precompute (ac_*_create_pre, ac_*_host_pre); fused encode at filters_n 64 ... 512; ac_workspace_*.
                          * (0.1.6: ac_stream_run replayable as a HIP graph, duplex launches; filters_n 64 / 128 and 16-bit PCM on the
                          * several-frames-per-wave kernels; mixed-radix FFT tier; masking model for any even filter_bands_n <= 1024) */

enum {
  AC_OK = 0,
  AC_EINVAL = -1,  /* bad shape / size / argument                                   */
  AC_EHIP = -2,    /* a HIP runtime call failed (message carries hipGetErrorString)  */
  AC_ENOMEM = -3,  /* host or device allocation failed                               */
  AC_ENODEV = -4,  /* no usable gfx950 device                                        */
  AC_EUNSUPPORTED = -5
};

/* window_type of MDCTransformer.__init__ (mdctransformer.py:13,199-211) */
enum { AC_WINDOW_VORBIS = 0, AC_WINDOW_SINE = 1, AC_WINDOW_RECT = 2 };

/* element types: `dtype` of the *_typed entry points (compute_dtype) and `precompute` of the *_pre ones (precompute_dtype) */
enum { AC_F32 = 0, AC_F64 = 1, AC_BF16 = 2, AC_F16 = 3 };   /* AC_F16: ac_mdct_forward_typed / ac_mdct_inverse_typed only */

typedef struct ac_mdct_plan ac_mdct_plan;
typedef struct ac_psy_plan ac_psy_plan;
typedef struct ac_stream ac_stream;

AC_API int ac_version(void);
AC_API const char* ac_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Host-only constant builders (fp64 precompute, no GPU needed).
 * ---------------------------------------------------------------------------------------- */

/* Non-zeros of the folding matrix F and of F^-1: replaces _filter_window_matrix / _polyphase_matrix /
 * _inv_polyphase_matrix incl. tf.linalg.inv (mdctransformer.py:155-229).  Eight vectors of N/2 doubles
 * written to coef[8*N/2] in the order a1 a2 a3 a4 s1 s2 s3 s4:
 *   analysis   v[h+j] = a1[j] xc[j] + a2[j] xc[N-1-j],   v[j]       = a3[j] xp[h-1-j] + a4[j] xp[h+j]
 *   synthesis  out[j] = s1[j] u_n[h-1-j] + s2[j] u_{n-1}[h+j],   out[N-1-j] = s3[j] u_n[h-1-j] + s4[j] u_{n-1}[h+j] */
AC_API int ac_mdct_fold_coefficients_host(int N, int window, double* coef);

/* Dense polyphase matrices exactly as the reference stores them: H, H_inv [2,N,N] float32
 * (mdctransformer.py:58-59).  Never used by the kernels; for the Python attributes only. */
AC_API int ac_mdct_dense_matrices_host(int N, int window, float* H, float* H_inv);

/* Constants of PsychoacousticModel.__init__ (psychoacoustic.py:52-69): W [N,M], W_inv [M,N],
 * spreading_matrix [M,M], quiet_threshold_intensity [M] as float32 (any pointer may be NULL) and
 * scalars[4] = {max_frequency, max_bark, bark_band_width, dB_MIN} as double. */
AC_API int ac_psy_tables_host(int N, int M, double sample_rate, double alpha,
                       float* W, float* W_inv, float* S, float* quiet, double* scalars);
/* the same constants unrounded, as PsychoacousticModel holds them with compute_dtype = float64 */
AC_API int ac_psy_tables_host_f64(int N, int M, double sample_rate, double alpha,
                           double* W, double* W_inv, double* S, double* quiet, double* scalars);

/* The same builders in the arithmetic type of the reference's `precompute_dtype` (mdctransformer.py:13-14,31-35,58-59;
 * psychoacoustic.py:14-15,61-69): precompute = AC_F64 (what the functions above compute: the reference's default) or AC_F32
 * -- every constant and operation rounded to float32, in the reference's order, including the cancellation
 * (1 - w[N+j] w[N-1-j]) / w[j] of mdctransformer.py:218-221 (exactly 0 for j = 0 at filters_n = 64 in float32) and the
 * float32 Bark mapping.  The reference's one TensorFlow-generated known-answer vector (tests/test_mdctransformer.py:51-52)
 * stems from a float32-precompute revision.  Values are returned as doubles (exact) / float32 matrices. */
AC_API int ac_mdct_fold_coefficients_host_pre(int N, int window, int precompute, double* coef);
AC_API int ac_mdct_dense_matrices_host_pre(int N, int window, int precompute, float* H, float* H_inv);
AC_API int ac_psy_tables_host_pre(int N, int M, double sample_rate, double alpha, int precompute,
                                  double* W, double* W_inv, double* S, double* quiet, double* scalars);

/* Scale-factor bands of the quantiser (extension, no counterpart in the reference): offsets[M+1] of contiguous bin ranges
 * [offsets[j], offsets[j+1]).  Bin i belongs to band min(M-1, floor(bark(f_i) / w)), f_i = (i + 1/2) (sample_rate/2) / N,
 * bark(f) = 6 asinh(f / 600), w = bark(sample_rate/2) / M, in float64.  Bands may be empty. */
AC_API int ac_psy_scale_bands_host(double sample_rate, int filter_bands_n, int bark_bands_n, int32_t* offsets);

/* ------------------------------------------------------------------------------------------
 * Plans (own the device copies of the constant tables).
 * ---------------------------------------------------------------------------------------- */

/* MDCTransformer.__init__ (mdctransformer.py:13-59).  N even, >= 2. */
AC_API int ac_mdct_plan_create(int N, int window, int device, ac_mdct_plan** out);
AC_API int ac_mdct_plan_destroy(ac_mdct_plan* plan);

/* PsychoacousticModel.__init__ (psychoacoustic.py:14-69). */
AC_API int ac_psy_plan_create(int N, int M, double sample_rate, double alpha, int device, ac_psy_plan** out);
AC_API int ac_psy_plan_destroy(ac_psy_plan* plan);

/* Plans whose constants are computed in `precompute` = AC_F64 (as the plain *_create) or AC_F32 (see the *_host_pre
 * builders).  With float32 constants the 2x2 fold blocks of F are no longer exact rotations, so the MDCT runs kernels
 * that carry all four coefficients per block: the several-frames-per-wave kernels at filters_n 64 ... 512 (mono / stereo,
 * float32), the LDS-FFT / O(N^2) tiers elsewhere.  ac_psy_plan_create_pre: spreading = AC_SPREAD_* or -1 for the default
 * of ac_psy_plan_create. */
AC_API int ac_mdct_plan_create_pre(int N, int window, int precompute, int device, ac_mdct_plan** out);
/* The transposed filter bank of `plan` as a plan of its own (same size, device, kernels): with T the analysis bank and S the
 * synthesis bank of `plan`, ac_mdct_inverse(adjoint, g)[:, N:-N] = 4 N T^T g and ac_mdct_forward(adjoint, g)[:, 1:-1] =
 * S^T g / (4 N) -- what the backward passes of transform / inverse_transform need (the reference is differentiated by
 * TensorFlow, mdctransformer.py:62-153).  The DCT-IV is symmetric, so only the O(N) fold transposes.  For Princen-Bradley
 * windows computed in float64 the adjoint equals the plan itself; for the rectangular window (mdctransformer.py:209-229)
 * and float32-precomputed constants it does not. */
AC_API int ac_mdct_plan_adjoint(const ac_mdct_plan* plan, ac_mdct_plan** out);
AC_API int ac_psy_plan_create_pre(int N, int M, double sample_rate, double alpha, int device, int spreading, int precompute,
                                  ac_psy_plan** out);

/* Form of the band x band product with the spreading matrix (psychoacoustic.py:205-207: sum_i max(eps, P_i)^alpha S[i,j])
 * in the wave-level kernels -- BASELINE configs[3] "Bark spreading cast as band x band MFMA contraction, bf16":
 *   AC_SPREAD_F32          float32 multiply-adds on the vector ALU;
 *   AC_SPREAD_BF16_MFMA    operands rounded to bfloat16, v_mfma_f32_4x4x4_16b_bf16, float32 accumulation: thresholds
 *                          within 5e-3 relative of the float32 form (bfloat16 has 8 mantissa bits);
 *   AC_SPREAD_BF16X2_MFMA  both operands split into bfloat16 hi + lo parts, four partial products on the matrix cores:
 *                          thresholds within 1e-5 of the float32 form, i.e. inside the 1e-4 parity bar.  This is what
 *                          ac_psy_plan_create builds where the wave-level kernels serve the plan (2 % faster fused
 *                          encode); everywhere else it builds AC_SPREAD_F32.
 * Served for stereo input (float32 or 16-bit PCM) by ac_encode_fused* and ac_mask_threshold; other channel counts and
 * the bfloat16 tensors of the *_typed entry points keep the float32 product.  AC_EUNSUPPORTED unless the plan runs the wave-level kernels. */
enum { AC_SPREAD_F32 = 0, AC_SPREAD_BF16_MFMA = 1, AC_SPREAD_BF16X2_MFMA = 2 };
AC_API int ac_psy_plan_create_ex(int N, int M, double sample_rate, double alpha, int device, int spreading, ac_psy_plan** out);
AC_API int ac_psy_plan_spreading(const ac_psy_plan* plan);

/* 1 when the plan runs the wave-level kernels (filters_n 1024 / 2048, Princen-Bradley window; 64 Bark bands), 0 when it
 * runs the LDS-FFT middle tier (filters_n from 16 to 4096 with a 5-smooth half: 2^a 3^b 5^c; up to 8192 for float32
 * tensors with filters_n % 4 == 0) or the generic O(N^2) kernels. */
AC_API int ac_mdct_plan_is_fast(const ac_mdct_plan* plan);
/* Which kernels serve float32 tensors of `channels_n` channels: 3 = the wave-level kernels (mono / stereo); 2 = a compile-time instance of the
 * LDS-FFT tier's 16-byte kernels (filters_n % 4 == 0 with a 5-smooth half, up to 8192); 1 = the tier's run-time forms;
 * 0 = the O(N^2) kernels; -1 = bad argument. */
AC_API int ac_mdct_plan_tier(const ac_mdct_plan* plan, int channels_n);
AC_API int ac_psy_plan_is_fast(const ac_psy_plan* plan);
/* Which kernels serve the masking model of a plan: 2 = the wave-level kernels fused into the encode (filter_bands_n 1024 /
 * 2048, 64 Bark bands, every bin in at most two adjacent bands); 1 = the wave-level kernels for general band layouts
 * (any even filter_bands_n up to 4096, up to 64 bands; any channel count);
 * 0 = the generic kernels (one workgroup per channel-frame). */
AC_API int ac_psy_plan_tier(const ac_psy_plan* plan);

/* (The test hook that forces the generic kernels is declared in audiocodec_amd_testing.h, not here.) */

/* ------------------------------------------------------------------------------------------
 * Hot path.
 * ---------------------------------------------------------------------------------------- */

/* MDCTransformer.transform (mdctransformer.py:62-125):  x [B, K*N, C] -> X [B, K+1, N, C]. */
AC_API int ac_mdct_forward(const ac_mdct_plan* plan, const float* x, float* X, int B, int K, int C, void* stream);

/* MDCTransformer.inverse_transform (mdctransformer.py:128-153):  X [B, Kp, N, C] -> x [B, (Kp+1)*N, C]. */
AC_API int ac_mdct_inverse(const ac_mdct_plan* plan, const float* X, float* x, int B, int Kp, int C, void* stream);

/* PsychoacousticModel.tonality (psychoacoustic.py:102-120):  X [B, F, N, C] -> t [B, F, 1, C]. */
AC_API int ac_tonality(const ac_psy_plan* plan, const float* X, float* t, int B, int F, int C, void* stream);

/* PsychoacousticModel.global_masking_threshold (psychoacoustic.py:122-148, with 169-210, 301-331):
 * X [B,F,N,C], t [B,F,1,C], drown in [0,1] -> thr [B,F,N,C]. */
AC_API int ac_mask_threshold(const ac_psy_plan* plan, const float* X, const float* t, float drown, float* thr,
                      int B, int F, int C, void* stream);

/* Backward passes of the masking model (the reference is differentiated by TensorFlow when it is used inside a
 * training graph -- see the gradient remark at psychoacoustic.py:311; here the adjoints are explicit kernels).
 * ac_tonality_backward: grad_t [B,F,1,C] -> grad_X [B,F,N,C] (d tonality / d X, psychoacoustic.py:102-120);
 *   accumulate != 0 adds into grad_X instead of overwriting it.
 * ac_mask_threshold_backward: grad_thr [B,F,N,C] -> grad_X [B,F,N,C] and grad_t [B,F,1,C]
 *   (d threshold / d X and d threshold / d tonality, psychoacoustic.py:122-148 with 169-210, 301-331). */
AC_API int ac_tonality_backward(const ac_psy_plan* plan, const float* X, const float* grad_t, float* grad_X, int accumulate,
                         int B, int F, int C, void* stream);
AC_API int ac_mask_threshold_backward(const ac_psy_plan* plan, const float* X, const float* t, float drown,
                               const float* grad_thr, float* grad_X, float* grad_t, int B, int F, int C, void* stream);

/* Fused encode = transform -> tonality -> global_masking_threshold in one pass over the PCM
 * (the composition of tests/test_psychoacoustic.py:38-41 + psychoacoustic.py:130-131).
 * x [B,K*N,C] -> X [B,K+1,N,C], t [B,K+1,1,C], thr [B,K+1,N,C].  mdct N must equal psy N. */
AC_API int ac_encode_fused(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const float* x, float* X, float* t,
                    float* thr, float drown, int B, int K, int C, void* stream);

/* How ac_encode_fused serves (mdct, psy) on tensors of C channels: 1 = ONE launch (filters_n 1024 / 2048 with the fused
 * wave-level epilogue; filters_n 64 ... 512, mono / stereo, with the masking model for general band layouts in the
 * several-frames-per-wave kernels; the LDS-FFT sizes where one launch measured faster than two on an MI355X -- 33 sizes
 * 540 ... 4096, 960 among them -- mono / stereo float32), 2 = the transform, then tonality + threshold in one pass over X,
 * 3 = three launches (generic kernels).  0 for inconsistent plans.  The results do not depend on it: the fused launches
 * return what the separate calls return, bit for bit (filters_n 1024 / 2048: within 1e-5). */
AC_API int ac_encode_launches(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C);

/* The fused encode with its element-wise tail (psychoacoustic.py:150-167 and :87-100 on the frames just computed), so
 * that a caller who wants them does not pay another pass over X and thr:
 *   AC_EMIT_NOISY    noisy   [B,K+1,N,C] = X + thr * Normal(0, 1/6): the values ac_add_noise(X, thr, seed) gives, bit for bit;
 *   AC_EMIT_DB_NORM  db_norm [B,K+1,N,C] = amplitude_to_dB_norm(X): the values ac_amplitude_to_db(X, norm = 1) gives.
 * One launch for stereo float32 input on the wave-level kernels at filters_n = 1024; elsewhere the encode followed by
 * the two element-wise kernels.  flags = 0 is ac_encode_fused.
 *   AC_EMIT_CODES    the quantising encode; exclusive with the other two flags.  The two output arguments are then read as
 *     int16_t* codes [B,K+1,N,C] and int8_t* sf [B,K+1,M,C] (seed is ignored): what ac_quantize gives on the X and thr of
 *     ac_encode_fused, bit for bit.  X, t and thr are each optional: NULL = not produced.  Where
 *     ac_encode_quantized_launches returns 1 this is ONE launch that quantises the frame while it is in registers and writes
 *     no float tensor the caller did not ask for; where it returns 2 the call runs the encode followed by the quantiser and
 *     needs X, t and thr as its intermediates (AC_EINVAL when one of them is NULL).
 *   AC_EMIT_PACKED   the encode at the plan's row budget (ac_psy_plan_with_row_budget) straight to fixed-stride packed rows,
 *     in ONE launch; exclusive with the other three flags.  out0 addresses one ac_packed_out (a host struct of device
 *     pointers, read during the call); out1, X, t and thr must be NULL and seed is ignored.  With row_bytes =
 *     ceil(row_bits / 32) * 4 (the struct's row_bytes must be that, else AC_EINVAL), row r = (b (K+1) + f) C + c takes bytes
 *     [r row_bytes, (r + 1) row_bytes) of data: the bytes ac_pack writes for the row's codes and sf under AC_EMIT_CODES, then
 *     zero bytes to the end of the slot, and fits[r] = 1.  A row that is longer than its slot -- offset 254 reached with
 *     the budget unmet -- is stored as the marked row: every width field 31, then zero bits, fits[r] = 0; it reads as a row
 *     of bands with sf = -128.  Every byte of data is written.  ac_unpack and ac_decode_quantized's packed form read data
 *     with index[r] = r row_bytes.  A plan without a row budget is AC_EINVAL.  Served where ac_encode_packed_launches
 *     returns 1; AC_EUNSUPPORTED elsewhere: compose it from ac_encode_fused, ac_quantize_budget (row_bits_out > 8 row_bytes
 *     marks a row that does not fit: fill its sf with -128) and ac_pack at those row starts into zero-filled data.
 *   AC_IN_PCM16      beside AC_EMIT_CODES or AC_EMIT_PACKED only: x is read as const int16_t* [B,K*N,C], x = pcm / 32768 (exact
 *     in float32), and the outputs are what the same call gives on that float32 tensor, bit for bit.  Alone, or with
 *     AC_EMIT_NOISY / AC_EMIT_DB_NORM, it is AC_EINVAL: the encode of 16-bit PCM to X, t and thr is ac_encode_fused_pcm16.
 *     AC_EMIT_CODES | AC_IN_PCM16: ONE launch where ac_encode_quantized_launches_pcm16 returns 1, under the X / t / thr rules
 *     above (each equals ac_encode_fused_pcm16's where given); where it returns 2, ac_encode_fused_pcm16's encode followed
 *     by the quantiser (the budgeted one at a plan with a row budget), X, t and thr required, and AC_EUNSUPPORTED where
 *     16-bit PCM has no encode.  AC_EMIT_PACKED | AC_IN_PCM16: ONE launch where ac_encode_packed_launches_pcm16 returns 1,
 *     AC_EUNSUPPORTED elsewhere.
 *   AC_IN_PACKED     transrating, valid only as AC_IN_PACKED | AC_EMIT_PACKED: packed rows in, fixed-
 *     stride packed rows at the plan's (lower) row budget out, in ONE launch that never decodes.  x addresses one
 *     ac_packed_rows (a host struct of device pointers, read during the call) whose index is [B,K+1,C] -- any int64 row
 *     starts, read as ac_unpack reads them, damaged rows included; out0 addresses one ac_packed_out as under AC_EMIT_PACKED;
 *     out1 is NULL or int16_t* offset [B,K+1,C]; X, t and thr must be NULL; drown and seed are ignored.  The mdct plan is
 *     checked as in every other form (same filters_n and device) and not used.  Slot r of data holds what this composition
 *     writes: ac_unpack, ac_quantize_budget in its thr == NULL form at the plan's row_bits with kmin 0 (the plan's own kmin is
 *     not used: it is relative to a threshold the rows no longer carry), sf = -128 in rows with row_bits_out > 8 row_bytes,
 *     ac_pack at r row_bytes into zero-filled data.  fits[r] reports only whether this call's row fitted: a marked input row
 *     (every width 31) comes out as the same marked bytes with fits[r] = 1.  offset[r] is the row's offset of that
 *     ac_quantize_budget call.  Any other combination with the bit, or a plan without a row budget, is AC_EINVAL; a refused
 *     call writes nothing.  Served where ac_transrate_launches returns 1; AC_EUNSUPPORTED elsewhere (run the composition).
 *     The input and output buffers must not overlap.
 *   AC_EMIT_REDUNDANT  protecting, valid only as AC_IN_PACKED | AC_EMIT_PACKED | AC_EMIT_REDUNDANT: the
 *     transrating call above into slots that also carry a low-bitrate copy of the frame before.  x and the plans as under
 *     AC_IN_PACKED; out0 addresses one ac_protected_out; out1, X, t and thr must be NULL.  With red_bytes =
 *     ceil(red_bits / 32) * 4 and slot_bytes = row_bytes + red_bytes, slot r = (b (K+1) + f) C + c takes bytes
 *     [r slot_bytes, (r + 1) slot_bytes) of data: first the row_bytes bytes the AC_IN_PACKED call writes for row (b,f,c) at
 *     the plan's budget, with fits[r] and offset[r]; then, for f >= 1, the red_bytes bytes that call writes for the INPUT row
 *     (b,f-1,c) at a budget of red_bits, with red_fits[r] and red_offset[r]; for f = 0, zero bytes, red_fits[r] = 1 and
 *     red_offset[r] = 0.  Every byte of data is written.  The struct's row_bytes must be the plan's and red_bits at least
 *     5 * bark_bands_n, else AC_EINVAL, as is any other combination with the bit; a refused call writes nothing.  Served
 *     where ac_protect_launches returns 1; AC_EUNSUPPORTED elsewhere (run the composition).
 * out0 / out1: float* noisy, float* db_norm under AC_EMIT_NOISY / AC_EMIT_DB_NORM; int16_t* codes, int8_t* sf under
 * AC_EMIT_CODES; ac_packed_out*, NULL under AC_EMIT_PACKED (NULL or int16_t* offset with AC_IN_PACKED). */
/*   AC_EMIT_CARRY  protecting chunk by chunk ("Streams"), valid only beside AC_IN_PACKED | AC_EMIT_PACKED |
 *     AC_EMIT_REDUNDANT: the rows are the K+1 frames of one chunk of a stream and out1 addresses one ac_protect_carry.  As
 *     the call above, but the redundant part, red_fits and red_offset of frame 0 are the copy at red_bits of the chunk before's
 *     last INPUT row, read from row_in [B,C,red_bytes], fits_in [B,C], offset_in [B,C] (row_in == NULL: a fresh stream, the
 *     f = 0 values above), and the copy of this chunk's last input row is written to row_out, fits_out, offset_out for the
 *     next call.  in and out must be distinct buffers (the carry is double buffered: the caller flips them), else
 *     AC_EINVAL.  So for any split into chunks the slots, flags and offsets, put together along frames, are those of the
 *     one-shot call on all rows.  Served where ac_protect_chunk_launches returns 1 (where ac_protect_launches does);
 *     AC_EUNSUPPORTED elsewhere, nothing written. */
/*   AC_IN_MIX  mixing, valid only as AC_IN_PACKED | AC_EMIT_PACKED | AC_IN_MIX: the packed rows of
 *     sources_n sources of the same codec and frame grid summed bin by bin in the spectral domain into fixed-stride packed
 *     rows at the plan's row budget, in ONE launch that never decodes.  x addresses one ac_mix_rows (a host struct, read
 *     during the call) whose src is a host array of sources_n ac_packed_rows, each with an index [B,K+1,C] of any int64 row
 *     starts, read as ac_unpack reads them, damaged rows included; out0 addresses one ac_packed_out as under AC_IN_PACKED; out1
 *     is NULL or int16_t* offset [B,K+1,C]; X, t and thr must be NULL.  gain (NULL: zeros) holds sources_n host ints in
 *     [-254, 254] in scale-factor units of 2^(1/4); active (NULL: all ones) is a device uint8 [sources_n,B,K+1,C], 0 = the
 *     row is never read and adds nothing.  With (q_i, s_i) the codes and scale factors ac_unpack returns for source i's row:
 *     X_i = fp32(q_i * step(g_i)), g_i = -128 where s_i = -128 (X_i is NaN there), else clamp(s_i + gain[i], -127, 127); the sum
 *     is ((X_0 + X_1) + X_2) + ... in float32; s0 of a band is -128 where any active source has it at -128, else the largest
 *     g_i over the active sources that hold a non-zero code in it, else 0.  Slot r of data holds what ac_quantize_budget at
 *     the plan's row_bits with kmin 0 gives for that sum under the threshold fp32(step(s0) * fp32(sqrt 3)) throughout each
 *     band (its scale factor at offset 0 is then s0), sf = -128 in rows with row_bits_out > 8 row_bytes, ac_pack at r row_bytes
 *     into zero-filled data; fits[r] and offset[r] as under AC_IN_PACKED.  A sum whose code passes +-32767 at offset 0 clamps
 *     there, and the 16-bit widths make the search raise the offset.  With one source and gain 0 the bytes are those of the
 *     AC_IN_PACKED call.  AC_EINVAL: any other combination with the bit, sources_n < 1, a gain outside [-254, 254], a NULL src
 *     or source, a plan without a row budget; a refused call writes nothing.  Served where ac_mix_launches returns 1;
 *     AC_EUNSUPPORTED elsewhere (run the composition).  Inputs and output must not overlap. */
enum { AC_EMIT_NOISY = 1, AC_EMIT_DB_NORM = 2, AC_EMIT_CODES = 4, AC_EMIT_PACKED = 8, AC_IN_PCM16 = 32, AC_IN_PACKED = 64,
       AC_EMIT_REDUNDANT = 256, AC_EMIT_CARRY = 512 };
enum { AC_IN_MIX = 1024 };   /* a flag of the same argument (above) */
/*   AC_IN_ROUTE  routing, valid only as AC_IN_PACKED | AC_EMIT_PACKED | AC_IN_ROUTE: the packed rows of
 *     sources_n sources mixed into outputs_n outputs (a bridge's mix-minus, monitor mixes) in ONE launch that reads every
 *     source row once and never decodes.  x addresses one ac_route_rows (a host struct, read during the call): src and active
 *     as ac_mix_rows', gain a host array [outputs_n * sources_n], gain[o * sources_n + i] in [-254, 254] or AC_ROUTE_MUTE:
 *     output o does not hear source i.  out0 addresses one ac_packed_out whose data is [outputs_n][B (K+1) C row_bytes] and
 *     fits [outputs_n][B,K+1,C]; out1 is NULL or int16_t* offset [outputs_n][B,K+1,C]; X, t and thr must be NULL.  Output o
 *     is, byte for byte, flags and offsets included, what AC_IN_MIX gives for the sources it hears, in source order, at its
 *     gains, with their rows of active; an output that hears nothing is the slot of a mix whose sources are all inactive.
 *     A row that no output hears, or that is inactive, is never read.  AC_EINVAL: any other combination with the bit,
 *     sources_n < 1, outputs_n < 1, a gain outside [-254, 254] that is not AC_ROUTE_MUTE, a NULL src, gain or source, a plan
 *     without a row budget; a refused call writes nothing.  Served where ac_route_launches returns 1; AC_EUNSUPPORTED
 *     elsewhere (run AC_IN_MIX, or its composition, per output).  Inputs and output must not overlap. */
enum { AC_IN_ROUTE = 2048 };   /* a flag of the same argument (above) */
/*   AC_EMIT_LEVEL  the level of packed rows, valid only as AC_IN_PACKED | AC_EMIT_LEVEL: the energy of
 *     every row from the row's own fields, in ONE launch that never decodes.  x addresses one ac_packed_rows with an index
 *     [B,K+1,C] of any int64 row starts, read as ac_unpack reads them, damaged rows included; out0 is float* energy [B,K+1,C];
 *     out1 is NULL or uint8_t* bad [B,K+1,C]; X, t and thr must be NULL; a plan without a row budget is accepted.  With
 *     (q, s) the codes and scale factors ac_unpack returns for a row: band j is bad where s_j = -128; Q_j is the exact integer
 *     sum of q_n^2 over band j (0 in a bad band); w(s) = fp32(step(s) step(s)); e_j = fp32(fp32(Q_j) w(s_j)), the conversion of
 *     the 64-bit Q_j rounding to nearest even, +0 in a bad band; energy is the fold tree over v[0 .. 64) = e: for d = 32, 16,
 *     ..., 1, v[i] = fp32(v[i] + v[i+d]) for i < d, then v[0].  bad is 1 where any band of the row is bad (marked rows, widths
 *     17 .. 30, a stored sf of -128), else 0.  energy is finite and >= +0 always.  AC_EINVAL: any other combination with the
 *     bit, a NULL struct or energy; a refused call writes nothing.  Served where ac_level_launches returns 1;
 *     AC_EUNSUPPORTED elsewhere (run the composition: ac_unpack, then the sums above).
 *   AC_SELECT_ACTIVE  the n loudest sources, valid only alone: levels of S sources -> the active mask
 *     AC_IN_MIX and AC_IN_ROUTE take.  x addresses one ac_select_rows (a host struct, read during the call); out0 is uint8_t*
 *     active [S,B,K+1,C]; out1, X, t and thr must be NULL; the plans are checked as in every other form and not used.  With
 *     E'_c = energy[s,b,f,c] where valid (NULL: all ones) is non-zero and the energy > 0, else +0 (NaN, negatives and -0 count
 *     as +0; +Inf stays): E[s,b,f] = ((E'_0 + E'_1) + ...) in float32; d = fp32(P[s,b,f-1] release), P[s,b,f] = d where d >
 *     E[s,b,f], else E[s,b,f] (peak hold with exponential release; a NaN d, Inf times 0, gives E), P[s,b,-1] = state[s,b]
 *     (NULL: 0).  Source s is selected at (b,f) where P[s,b,f] > gate and fewer than n sources t have P[t,b,f] > P[s,b,f] or
 *     (P[t,b,f] == P[s,b,f] and t < s).  active[s,b,f,c] = selected and valid[s,b,f,c] != 0; afterwards state[s,b] =
 *     P[s,b,K] (updated in place), so any split of the frames with state carried equals the one-shot call.  AC_EINVAL: any
 *     other combination with the bit, a NULL struct, energy or output, sources_n < 1, n outside [0, sources_n], release
 *     outside [0, 1] or NaN, gate negative or NaN; AC_EUNSUPPORTED: sources_n > AC_SELECT_MAX_SOURCES.  A refused call
 *     writes nothing. */
enum { AC_EMIT_LEVEL = 4096, AC_SELECT_ACTIVE = 8192 };   /* flags of the same argument (above) */
#define AC_SELECT_MAX_SOURCES 64 /* the most sources AC_SELECT_ACTIVE ranks: a lane of a wave each */
typedef struct ac_select_rows {
  int32_t sources_n;     /* S >= 1 */
  const float* energy;   /* [S,B,K+1,C] (device) */
  const uint8_t* valid;  /* [S,B,K+1,C] (device) 0 = the row does not count and is never active, or NULL: all ones */
  int32_t n;             /* at most n sources are selected per clip and frame, in [0, S] */
  float release;         /* in [0, 1]: what a frame keeps of the peak before it */
  float gate;            /* >= 0: a source is selected only above it */
  float* state;          /* [S,B] (device) the peaks carried from chunk to chunk, updated in place, or NULL: zeros */
} ac_select_rows;
/* The largest row budget the one launch of AC_EMIT_PACKED serves: a wave stages both rows of its frame pair in the 4 KB of
 * its LDS buffer that the masking model has left, 2 KB = 16384 bits each. */
#define AC_PACK_ROWS_MAX_BITS 16384
typedef struct ac_packed_out {
  uint8_t* data;     /* [B (K+1) C row_bytes] the packed rows (device) */
  int64_t row_bytes; /* ceil(row_bits / 32) * 4 of the plan's budget */
  uint8_t* fits;     /* [B,K+1,C] 1 = the row's codes are in its slot, 0 = the marked row (device) */
} ac_packed_out;
typedef struct ac_protected_out {
  uint8_t* data;       /* [B (K+1) C (row_bytes + red_bytes)] the protected slots (device) */
  int64_t row_bytes;   /* ceil(row_bits / 32) * 4 of the plan's budget: the primary part of a slot */
  uint8_t* fits;       /* [B,K+1,C] of the primary part, as ac_packed_out's (device) */
  int32_t red_bits;    /* the redundant budget, >= 5 * bark_bands_n; red_bytes = ceil(red_bits / 32) * 4 */
  uint8_t* red_fits;   /* [B,K+1,C] of the redundant part of the slot; 1 at f = 0 (device) */
  int16_t* offset;     /* [B,K+1,C] offsets of the primary search (device), or NULL */
  int16_t* red_offset; /* [B,K+1,C] offsets of the redundant search, by the slot that holds the copy; 0 at f = 0; or NULL */
} ac_protected_out;
typedef struct ac_protect_carry {
  const uint8_t* row_in;     /* [B,C,red_bytes] the copies the chunk before left, or NULL: a fresh stream (device) */
  const uint8_t* fits_in;    /* [B,C] */
  const int16_t* offset_in;  /* [B,C] */
  uint8_t* row_out;          /* the same three for the next chunk: other buffers */
  uint8_t* fits_out;
  int16_t* offset_out;
} ac_protect_carry;
#define AC_MIX_MAX_SOURCES 8 /* the most sources the one launch of AC_IN_MIX reads */
struct ac_packed_rows;
typedef struct ac_mix_rows {
  int32_t sources_n;                 /* >= 1 */
  const struct ac_packed_rows* src;  /* [sources_n] (host): data, nbytes, index [B,K+1,C] of every source */
  const int32_t* gain;               /* [sources_n] (host) scale-factor units in [-254, 254], or NULL: zeros */
  const uint8_t* active;             /* [sources_n,B,K+1,C] (device) 0 = the row is never read, or NULL: all ones */
} ac_mix_rows;
#define AC_ROUTE_MAX_SOURCES 4 /* the most sources and ... */
#define AC_ROUTE_MAX_OUTPUTS 8 /* ... outputs the one launch of AC_IN_ROUTE serves (section 8i: beyond four sources the
                                * staged rows leave too few waves on a CU, and one AC_IN_MIX call per output is faster) */
#define AC_ROUTE_MUTE (-32768) /* in ac_route_rows' gain: the output does not hear the source */
typedef struct ac_route_rows {
  int32_t sources_n;                 /* >= 1 */
  int32_t outputs_n;                 /* >= 1 */
  const struct ac_packed_rows* src;  /* [sources_n] (host): data, nbytes, index [B,K+1,C] of every source */
  const int32_t* gain;               /* [outputs_n * sources_n] (host): [-254, 254] or AC_ROUTE_MUTE */
  const uint8_t* active;             /* [sources_n,B,K+1,C] (device) 0 = the row is never read, or NULL: all ones */
} ac_route_rows;
AC_API int ac_encode_fused_ex(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const float* x, float* X, float* t, float* thr,
                       float drown, int flags, void* out0, void* out1, uint64_t seed, int B, int K, int C,
                       void* stream);
/* Launches of ac_encode_fused_ex with AC_EMIT_CODES on tensors of C channels: 1 = the fused kernel (filters_n = 1024 on the
 * wave-level kernels, mono / stereo float32, the f32 or split-bf16 spreading product), 2 = encode + quantiser (everything
 * else, and every configuration while AC_ENCODE_QUANT_NOFUSE=1 is set in the environment: read per call).  0 for NULL or
 * inconsistent plans.  The results do not depend on it. */
AC_API int ac_encode_quantized_launches(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C);
/* Library launches of an encode to fixed-stride packed rows on tensors of C channels: 1 = ac_encode_fused_ex with
 * AC_EMIT_PACKED serves it (where ac_encode_quantized_launches returns 1, bark_bands_n = 64 and the plan's row budget is at
 * most AC_PACK_ROWS_MAX_BITS), else ac_encode_launches + 2: the encode, ac_quantize_budget and ac_pack of the composition
 * above (also everywhere while AC_ENCODE_PACKED_NOFUSE=1 is set in the environment: read per call).  0 for NULL or
 * mismatched plans, C < 1, or a plan without a row budget.  The bytes do not depend on it. */
AC_API int ac_encode_packed_launches(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C);
/* The two queries above for int16 input (AC_IN_PCM16), with the same return conventions: 1 = the fused kernel reads the 16-bit
 * PCM itself (k_fwd_fast_q16 / qb16 / qp16: every instance passed its register gate, so wherever the float32 query returns
 * 1), else the launches of the composition.  AC_ENCODE_QUANT_NOFUSE=1 / AC_ENCODE_PACKED_NOFUSE=1 apply (read per call). */
AC_API int ac_encode_quantized_launches_pcm16(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C);
AC_API int ac_encode_packed_launches_pcm16(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C);
/* Library launches of transrating rows of C channels to the plan's row budget: 1 = ac_encode_fused_ex with AC_IN_PACKED |
 * AC_EMIT_PACKED serves it (float32 plans with filters_n = 1024, bark_bands_n = 64 and a row budget of at most
 * AC_PACK_ROWS_MAX_BITS; any C, rows being independent), else 3: ac_unpack, ac_quantize_budget's thr == NULL form and ac_pack
 * of the composition above (also everywhere while AC_TRANSRATE_NOFUSE=1 is set in the environment: read per call).  0 for a
 * NULL plan, C < 1, or a plan without a row budget.  The bytes do not depend on it. */
AC_API int ac_transrate_launches(const ac_psy_plan* psy, int C);
/* Library launches of mixing the rows of S sources of C channels to the plan's row budget: 1 = ac_encode_fused_ex with
 * AC_IN_PACKED | AC_EMIT_PACKED | AC_IN_MIX serves it (where ac_transrate_launches returns 1 and S <= AC_MIX_MAX_SOURCES), else
 * 2 S + 2: S ac_unpack, S ac_dequantize, ac_quantize_budget and ac_pack of the composition above (also everywhere while
 * AC_MIX_NOFUSE=1 is set in the environment: read per call).  0 for a NULL plan, C < 1, S < 1 or a plan without a row budget.
 * The bytes do not depend on it. */
AC_API int ac_mix_launches(const ac_psy_plan* psy, int C, int S);
/* Library launches of routing the rows of S sources of C channels to O outputs that hear all of them: 1 = ac_encode_fused_ex
 * with AC_IN_PACKED | AC_EMIT_PACKED | AC_IN_ROUTE serves it (where ac_mix_launches returns 1 for S, S <= AC_ROUTE_MAX_SOURCES and O <=
 * AC_ROUTE_MAX_OUTPUTS), else O ac_mix_launches(psy, C, S), the AC_IN_MIX calls of the composition (an output that hears
 * fewer sources takes ac_mix_launches of its count; also everywhere while AC_ROUTE_NOFUSE=1 is set in the environment: read
 * per call -- with O = 1 that count is 1 too, and the call is refused all the same while the variable is set).  0 for a NULL
 * plan, C < 1, S < 1, O < 1 or a plan without a row budget.  The bytes do not depend on it. */
AC_API int ac_route_launches(const ac_psy_plan* psy, int C, int S, int O);
/* Library launches of the level of rows of C channels: 1 = ac_encode_fused_ex with AC_IN_PACKED | AC_EMIT_LEVEL serves it
 * (float32 plans with filters_n = 1024 and bark_bands_n = 64, with or without a row budget; any C, rows being independent),
 * 0 = the library has no launch of its own for it: ac_unpack and the caller's sums are the composition (also everywhere
 * while AC_LEVEL_NOFUSE=1 is set in the environment: read per call).  0 too for a NULL plan or C < 1.  The values do not
 * depend on it. */
AC_API int ac_level_launches(const ac_psy_plan* psy, int C);
/* Library launches of protecting rows of C channels with a redundant budget of red_bits: 1 = ac_encode_fused_ex with
 * AC_IN_PACKED | AC_EMIT_PACKED | AC_EMIT_REDUNDANT serves it (where ac_transrate_launches returns 1 and red_bits is at most
 * AC_PACK_ROWS_MAX_BITS), else the launches of the composition's two transrating calls, each 1 or 3 (also everywhere while
 * AC_PROTECT_NOFUSE=1 is set in the environment: read per call).  0 for a NULL plan, C < 1, a plan without a row budget or
 * red_bits below 5 * bark_bands_n.  The bytes do not depend on it. */
AC_API int ac_protect_launches(const ac_psy_plan* psy, int C, int red_bits);
/* The same for one chunk of a stream (AC_EMIT_CARRY): 1 where ac_protect_launches is 1, else its value (the composition's two
 * transrating calls; the copies to and from the carry are the caller's). */
AC_API int ac_protect_chunk_launches(const ac_psy_plan* psy, int C, int red_bits);

/* 16-bit PCM at the boundary (extension; the reference takes float PCM in [-1, 1] only, mdctransformer.py:104):
 * x = pcm / 32768 on the way in; on the way out pcm = 0 if x is NaN else clamp(rint(fp32(32768 x)), -32768, 32767), rint
 * round half to even (+-Inf and products that overflow float32 go to the rail of their sign; a NaN sample is silence).  Both
 * are fused into the kernels' loads / stores, so a frame moves 2 bytes per sample instead of 4.  Served by the wave-level
 * kernels (filters_n 64 ... 2048 in powers of two, 'vorbis' / 'sine' window; below 1024 mono / stereo) and by the LDS-FFT
 * tier at filters_n 120, 240, 480, 960, 1920, 576, 1152 (mono / stereo, any window); AC_EUNSUPPORTED otherwise.  Shapes as
 * the float32 entry points. */
AC_API int ac_mdct_forward_pcm16(const ac_mdct_plan* plan, const int16_t* x, float* X, int B, int K, int C, void* stream);
AC_API int ac_mdct_inverse_pcm16(const ac_mdct_plan* plan, const float* X, int16_t* x, int B, int Kp, int C, void* stream);
AC_API int ac_encode_fused_pcm16(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const int16_t* x, float* X, float* t,
                          float* thr, float drown, int B, int K, int C, void* stream);

/* Perceptual quantiser (extension: the quantisation that add_noise, psychoacoustic.py:150-167, stands in for; float32,
 * even filter_bands_n, any bark_bands_n and channel count).  With scale-factor bands as in ac_psy_scale_bands_host and
 * step(s) = ldexp(fp32(2^((s&3)/4)), s>>2):
 *   sf[b,f,j,c]   = the largest s in [-127, 127] with fp32(step(s) * fp32(sqrt 3)) <= min(thr over band j), else -127;
 *                   0 for an empty band; -128 when an X or thr of the band is NaN / Inf;
 *   codes[b,f,i,c] = clamp(rint(fp32(X * 2^-(s/4))), -32767, 32767) (0 in a band with sf = -128);
 *   dequantised X = fp32(code * step(sf)) (NaN in a band with sf = -128): |error| <= thr / (2 sqrt 3) (1 + 1e-6) + 1e-6 |X|.
 * ac_quantize: X, thr [B,F,N,C] float32 -> codes int16 [B,F,N,C], sf int8 [B,F,M,C].  ac_dequantize: the inverse map.
 * ac_decode_quantized: the synthesis (ac_mdct_inverse, or ac_mdct_inverse_pcm16 when pcm16 is given instead of x) of the
 *   dequantised spectra, codes [B,Kp,N,C] -> x [B,(Kp+1)*N,C]; bit-equal to ac_dequantize followed by the inverse.
 *   scratch [B,Kp,N,C] float32 receives the dequantised spectra where ac_decode_quantized_launches returns 2 and may be
 *   NULL where it returns 1 (filters_n 1024 / 2048 on the wave-level kernels, mono / stereo: one launch that dequantises in
 *   its loads).  mdct and psy must share filters_n and device.
 *   With sf == NULL, codes addresses one ac_packed_rows (a host struct of device pointers, read during the call): the rows of
 *   the packed bitstream (below) at index [B,Kp,C], contiguous, are decoded in ONE launch that reads the bitstream where the
 *   synthesis above reads codes and sf -- bit-equal to ac_unpack followed by ac_decode_quantized, with ac_unpack's reading
 *   of damaged rows and of row starts outside data.  Served where ac_decode_packed_launches returns 1; AC_EUNSUPPORTED
 *   elsewhere (unpack the rows with ac_unpack and pass codes and sf).  codes == NULL stays an error.
 *   Concealment of lost rows: with sf == NULL, a scratch that is not NULL addresses one ac_conceal (a
 *   host struct, read during the call); scratch == NULL is the call above, on the same kernel.  lost uint8 [B,Kp,C] (device),
 *   nonzero = the row did not arrive; lost == NULL: no row is lost.  max_age outside [0, AC_CONCEAL_MAX_AGE] is AC_EINVAL.
 *   Row (b,f,c) is read from the row at index[b,f-age,c], age = the smallest a in [0, min(max_age, f)] with
 *   lost[b,f-a,c] == 0, with ac_unpack's reading of it, and every scale factor s != -128 replaced by
 *   max(s - AC_CONCEAL_FADE * age, -127): the spectrum of the source row times 2^-age, exactly, wherever the clamp is not
 *   met (step(s - 4) = step(s) / 2).  A band with sf = -128 stays one.  Where no such a exists -- a run of lost rows longer
 *   than max_age, or lost rows before the first one of a clip and channel that arrived -- the row reads as a row that
 *   starts at nbytes: silence.  Sources are looked for in this call's index only.  Still one launch; served where
 *   ac_decode_packed_launches returns 1 and AC_EUNSUPPORTED elsewhere.  Streams (ac_stream_inverse_typed) do not conceal.
 *   Recovery: a max_age that is not negative and has AC_CONCEAL_REDUNDANT set marks the struct as the
 *   longer ac_conceal_redundant, whose first two members are ac_conceal's; max_age is the rest of the field.  Ahead of the
 *   rule above, a row with lost[b,f,c] != 0, f + 1 < Kp and lost[b,f+1,c] == 0 is read from index[b,f+1,c] + redundant_at
 *   -- the redundant part of a protected slot where redundant_at is its row_bytes -- with age 0, as ac_unpack reads any
 *   row start; it is no source of concealment itself.  redundant_at outside [1, 2^31), lost == NULL or a max_age outside
 *   [0, AC_CONCEAL_MAX_AGE] is AC_EINVAL.  One launch, served as the form above.  Without the bit the call is the one above.
 * ac_decode_packed_launches: 1 where that form is served (float32 plans on the wave-level kernels, filters_n = 1024,
 *   bark_bands_n = 64, mono / stereo), else 1 + ac_decode_quantized_launches: ac_unpack, then ac_decode_quantized (also
 *   everywhere while AC_DECODE_PACKED_NOFUSE=1 is set in the environment: read per call).  0 for NULL or mismatched plans. */
typedef struct ac_packed_rows {
  const uint8_t* data;  /* [nbytes] the bitstream (device) */
  int64_t nbytes;
  const int64_t* index; /* [B,Kp,C] byte offset of every row in data (device); any int64 */
} ac_packed_rows;
#define AC_CONCEAL_FADE 4     /* scale-factor units a concealed row loses per frame of age: 6.02 dB, an exact halving */
#define AC_CONCEAL_MAX_AGE 31 /* the largest max_age */
typedef struct ac_conceal {
  const uint8_t* lost;  /* [B,Kp,C] nonzero = the row did not arrive (device); NULL: none is lost */
  int32_t max_age;      /* frames a row may be repeated over, 0 .. AC_CONCEAL_MAX_AGE; 0 = zero-filling */
} ac_conceal;
enum { AC_CONCEAL_REDUNDANT = 256 };   /* in ac_conceal's max_age: the struct is an ac_conceal_redundant */
typedef struct ac_conceal_redundant {
  const uint8_t* lost;  /* as ac_conceal's; not NULL */
  int32_t max_age;      /* (0 .. AC_CONCEAL_MAX_AGE) | AC_CONCEAL_REDUNDANT */
  int64_t redundant_at; /* bytes from a row's start to the copy of the frame before it, in [1, 2^31) */
} ac_conceal_redundant;
AC_API int ac_quantize(const ac_psy_plan* psy, const float* X, const float* thr, int16_t* codes, int8_t* sf, int B, int F,
                       int C, void* stream);
AC_API int ac_dequantize(const ac_psy_plan* psy, const int16_t* codes, const int8_t* sf, float* X, int B, int F, int C,
                         void* stream);
AC_API int ac_decode_quantized(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const int16_t* codes, const int8_t* sf,
                               float* x, int16_t* pcm16, float* scratch, int B, int Kp, int C, void* stream);
AC_API int ac_decode_quantized_launches(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C);
AC_API int ac_decode_packed_launches(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C);

/* Packed bitstream of quantised spectra (extension).  A row is one (b, f, c) of codes [B,F,N,C] and
 * sf [B,F,M,C]; bit p of a row is bit p % 32 of its little-endian 32-bit word p / 32; fields are written LSB first:
 *   1. widths: M fields of 5 bits, band j at bits [5j, 5j+5): 31 where sf = -128, else w_j = the bit length of the band's
 *      largest zz(q) = (q << 1) ^ (q >> 15) on the 16 bits of the code (0 for an empty or all-zero band);
 *   2. for every band with 1 <= w_j <= 16, in band order: its sf, 8 bits of two's complement;
 *   3. for every such band, in band order: each bin's zz(q) in w_j bits, in bin order;
 *   4. zero bits up to a multiple of 32.
 * Rows follow one another in (b, f, c) order in data; index[b,f,c] int64 is a row's byte offset (a multiple of 4).
 * ac_pack_index: the row lengths, scanned into index [B,F,C], and their sum into *total (device, one int64); scratch of
 *   ac_pack_scratch_bytes(B, F, C) bytes (NULL where that is 0).  ac_pack: the rows into data [*total] at index.
 * ac_unpack: data [nbytes] and index [B,F,C] (any row starts, e.g. a slice of frames) -> the canonical codes [B,F,N,C] and
 *   sf [B,F,M,C]: codes 0 and sf -128 in a band of width 31, sf 0 in a band of width 0, the stored values elsewhere.  A
 *   width of 17 .. 30 reads as 31; bits at or beyond nbytes (or before 0) read as 0: nothing outside data is loaded.
 * float32 psychoacoustic plans with an even filter_bands_n, as the quantiser; an empty batch launches nothing. */
AC_API size_t ac_pack_scratch_bytes(int B, int F, int C);
AC_API int ac_pack_index(const ac_psy_plan* psy, const int16_t* codes, const int8_t* sf, int64_t* index, int64_t* total,
                         void* scratch, int B, int F, int C, void* stream);
AC_API int ac_pack(const ac_psy_plan* psy, const int16_t* codes, const int8_t* sf, const int64_t* index, uint8_t* data, int B,
                   int F, int C, void* stream);
AC_API int ac_unpack(const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes, const int64_t* index, int16_t* codes,
                     int8_t* sf, int B, int F, int C, void* stream);

/* Rate control (extension): ac_quantize with every scale factor of a row (b, f, c) raised by one offset.
 * With sf0 the scale factors of ac_quantize, a row's scale factors at offset k are 0 in an empty band, -128 where sf0 = -128
 * and clamp(sf0 + k, -127, 127) elsewhere; its codes are ac_quantize's rule with those steps.  bits(k), the row's packed
 * length before padding (5M + sum over bands of width 1..16 of 8 + width * band length), does not grow with k.
 * ac_quantize_budget: X, thr [B,F,N,C] float32 -> codes int16 [B,F,N,C], sf int8 [B,F,M,C], offset int16 [B,F,C] and
 *   row_bits_out int32 [B,F,C] (may be NULL) = bits(offset), where offset is the smallest k in [kmin, 254] with
 *   bits(k) <= the row's budget, else 254 (a budget not met shows as row_bits_out > budget).  The budget is
 *   row_bits_per_row[b,f,c] (int32 [B,F,C], entries not checked) or, where that is NULL, row_bits (>= 5M).  kmin = 0 with a
 *   budget of 16N + 13M gives ac_quantize's output.  kmin in [-254, 254]; plans as ac_quantize.
 *   With thr == NULL, X addresses one ac_quantized_rows (a host struct of device pointers, read during the call) and the call
 *   requantises: the row's stored scale factors stand for sf0 and fp32(code * step(sf)) for X, so the
 *   rules above run on a row that is already quantised -- codes under sf = -128 count as 0 and an all-zero band as sf 0, as
 *   ac_unpack returns them.  At an offset of 0 a row comes back as it was (-32768 as -32767).  kmin in [0, 254] in this form:
 *   an offset below 0 cannot restore what the first quantiser dropped.  The inputs must not overlap the outputs. */
typedef struct ac_quantized_rows {
  const int16_t* codes; /* [B,F,N,C] (device) */
  const int8_t* sf;     /* [B,F,M,C] (device) */
} ac_quantized_rows;
AC_API int ac_quantize_budget(const ac_psy_plan* psy, const float* X, const float* thr, int row_bits,
                              const int32_t* row_bits_per_row, int kmin, int16_t* codes, int8_t* sf, int16_t* offset,
                              int32_t* row_bits_out, int B, int F, int C, void* stream);

/* A plan at a row budget: the budget travels in the plan, so that the entry points that quantise from sf0 serve a codec that
 * IS at a bitrate, the fused encode among them.  ac_psy_plan_with_row_budget: a plan of its own with the N, M, sample rate,
 * alpha, precompute type, spreading form and device of `plan`; it owns its device tables, is destroyed with
 * ac_psy_plan_destroy, and its creation may block the host as the other plan builders may.  row_bits >= 5M and kmin in
 * [-254, 254], AC_EINVAL otherwise; deriving from a derived plan replaces the budget.  Every entry point treats the derived
 * plan exactly as `plan`, except the two that quantise from sf0:
 *   ac_quantize(derived, X, thr, codes, sf, ...) writes the codes and sf ac_quantize_budget(plan, X, thr, row_bits, NULL,
 *     kmin, ...) writes, bit for bit;
 *   ac_encode_fused_ex(..., derived, ..., AC_EMIT_CODES, ...) gives that on the X and thr of ac_encode_fused, under the X / t /
 *     thr rules of AC_EMIT_CODES: ONE launch that meets the budget while the frame is in registers where
 *     ac_encode_quantized_launches returns 1, the encode followed by the budgeted quantiser where it returns 2.
 * ac_quantize_budget and ac_quantize_clip_budget obey their own arguments on any plan.  Dequantise, pack, unpack and decode
 * need nothing: the offset is in the scale factors.
 * ac_psy_plan_row_budget: the budget of a plan into *row_bits and *kmin (either may be NULL); 0, 0 for a plan without one. */
AC_API int ac_psy_plan_with_row_budget(const ac_psy_plan* plan, int row_bits, int kmin, ac_psy_plan** out);
AC_API int ac_psy_plan_row_budget(const ac_psy_plan* plan, int* row_bits, int* kmin);

/* Rate control per clip (extension): one budget for the F*C rows of a clip, r = f*C + c.  With bits_r(k)
 * of ac_quantize_budget, len_r(k) = 32 * ceil(bits_r(k) / 32) is a row's packed length with its padding and total_b(k) the sum
 * over the clip's rows.  k_b = the smallest k in [kmin, 254] with total_b(k) <= T_b, else 254.  Where k_b > kmin and
 * total_b(k_b) <= T_b, the first p_b rows take the offset k_b - 1: with d_r = len_r(k_b - 1) - len_r(k_b), p_b is the number of
 * rows whose inclusive prefix sum of d is at most T_b - total_b(k_b); otherwise p_b = 0.  Every other row takes k_b.
 * ac_quantize_clip_budget: X, thr [B,F,N,C] float32 -> codes int16 [B,F,N,C], sf int8 [B,F,M,C], offset int16 [B,F,C] and,
 *   each NULL or given, row_bits_out int32 [B,F,C] = bits_r(offset_r), clip_offset int16 [B] = k_b and clip_bits_out
 *   int64 [B] = the sum of len_r(offset_r): the clip's bits in ac_pack's data (a budget not met shows as clip_bits_out > T_b).
 *   T_b is clip_bits_per_clip[b] (device int64 [B], entries not checked) or, where that is NULL, clip_bits
 *   (>= F * C * 32 * ceil(5M / 32)).  scratch: ac_clip_budget_scratch_bytes(psy, B, F, C) device bytes, 16-byte aligned; the
 *   call allocates nothing and does not synchronise with the host.  kmin in [-254, 254]; plans as ac_quantize. */
AC_API size_t ac_clip_budget_scratch_bytes(const ac_psy_plan* psy, int B, int F, int C);
AC_API int ac_quantize_clip_budget(const ac_psy_plan* psy, const float* X, const float* thr, int64_t clip_bits,
                                   const int64_t* clip_bits_per_clip, int kmin, int16_t* codes, int8_t* sf, int16_t* offset,
                                   int32_t* row_bits_out, int16_t* clip_offset, int64_t* clip_bits_out, void* scratch, int B,
                                   int F, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Streaming overlap-add (chunked transform with device-resident state).
 * Analysis state: the last input block per (b,c) [B,N,C]; synthesis state: the aliased second half of
 * the last DCT-IV output per (b,c) [B,C,N/2].  A fresh/reset stream starts from zero state, so the
 * concatenation of chunk outputs equals the one-shot transform frame for frame.
 * Streams: ac_stream_create allocates the float32 state, zeroes it and waits for the zeroing (it may block the host, as the
 * plan builders may for their uploads): nothing a creation call enqueued can be overtaken by a later call on any stream.  The float64 state (ac_stream_*_typed with AC_F64) is allocated by the
 * first float64 chunk call -- the one allocation a chunk call makes, of the library's own memory -- and zeroed with
 * hipMemsetAsync on THAT call's stream, ahead of its kernels; nothing goes to the null stream.  ac_stream_reset zeroes the
 * state on its stream.  The state is carried from call to call: the caller orders the calls on one ac_stream (one HIP
 * stream, or events between streams), as it orders the chunks themselves.
 * ---------------------------------------------------------------------------------------- */
AC_API int ac_stream_create(const ac_mdct_plan* plan, int B, int C, ac_stream** out);
AC_API int ac_stream_reset(ac_stream* s, void* stream);
AC_API int ac_stream_destroy(ac_stream* s);
/* x_chunk [B, k*N, C] -> X [B, k, N, C]  (frame i = blocks i-1, i; block -1 = state) */
AC_API int ac_stream_forward(ac_stream* s, const float* x_chunk, float* X, int k, void* stream);
/* the same with the masking model on the chunk's frames: X, t [B, k, 1, C], thr [B, k, N, C] equal, frame for frame and bit
 * for bit, what ac_encode_fused returns for the whole signal (one fused launch where the wave-level kernels serve both
 * plans; psychoacoustic.py:102-148 on mdctransformer.py:62-125) */
AC_API int ac_stream_encode(ac_stream* s, const ac_psy_plan* psy, const float* x_chunk, float* X, float* t, float* thr,
                     float drown, int k, void* stream);
/* X_chunk [B, k, N, C] -> x [B, k*N, C]  (block i = frames i, i-1; frame -1 = state) */
AC_API int ac_stream_inverse(ac_stream* s, const float* X_chunk, float* x, int k, void* stream);
/* The two state buffers of a stream are double-buffered (a kernel reads one while it writes the other), so the current
 * state changes address with every chunk call.  ac_stream_settle moves it back to the stream's home buffers: at most two
 * small device-to-device copies on `stream` (B*N*C and B*C*N/2 floats), nothing when it is already there.  Needed only by
 * callers that replay a captured ac_stream_run (below) after chunk calls: settle before capturing and before each such replay. */
AC_API int ac_stream_settle(ac_stream* s, void* stream);

/* Feeds nchunks consecutive chunks of k blocks through the stream in one call (a long device-resident signal, a ring
 * buffer that has filled up): chunk i is analysed -- with the masking model when psy is not NULL, else t_chunks /
 * thr_chunks are ignored -- from x_chunks[i] [B, k*N, C] into X_chunks[i] (t_chunks[i], thr_chunks[i]) and, when
 * xhat_chunks is not NULL, synthesised from X_chunks[i] into xhat_chunks[i] [B, k*N, C].  Results are those of nchunks
 * calls of ac_stream_encode (ac_stream_forward) and ac_stream_inverse on `stream`, issued from one host call (no per-call
 * binding overhead).  With synthesis, chunks small enough to be latency-bound (one or a few clips) and distinct buffers
 * per chunk, the analysis of chunk i + 1 and the synthesis of chunk i share ONE launch (float32, mono / stereo,
 * filters_n 1024 / 2048): nchunks + 1 launches instead of 2 nchunks, same results bit for bit.  A caller that reuses
 * one buffer for consecutive chunks gets the dependent chain.  The call settles the stream's state at its home buffers on
 * entry and on exit (ac_stream_settle) and nothing synchronises or allocates: a call is capturable into a HIP graph
 * (hipStreamBeginCapture on `stream`; call ac_stream_settle BEFORE the capture so that no state copy is recorded), and
 * replaying the graph repeats it on new contents of the same buffers -- 7.9 us per chunk of one stereo clip against
 * 11.9 us for the plain launches (the gaps between dependent launches go).  A replay addresses the home buffers: if chunk
 * calls (ac_stream_forward / _encode / _inverse) or ac_stream_reset ran since the last ac_stream_run, call
 * ac_stream_settle before replaying.  The pointer lists are host arrays. */
AC_API int ac_stream_run(ac_stream* s, const ac_psy_plan* psy, int nchunks, int k, const float* const* x_chunks,
                  float* const* X_chunks, float* const* t_chunks, float* const* thr_chunks, float* const* xhat_chunks,
                  float drown, void* stream);

/* ------------------------------------------------------------------------------------------
 * Element-wise utilities of PsychoacousticModel (psychoacoustic.py:71-100, 150-167).
 * ---------------------------------------------------------------------------------------- */
/* amplitude_to_dB (norm = 0) / amplitude_to_dB_norm (norm = 1) on n floats. */
AC_API int ac_amplitude_to_db(const float* a, float* out, size_t n, int norm, void* stream);
/* d amplitude_to_dB(_norm) / d a: grad_a = grad_out * (20 / ln 10) / a where a^2 > 1e-14 (0 inside the clamp), / 140 for
 * the normalised form. */
AC_API int ac_amplitude_to_db_backward(const float* a, const float* grad_out, float* grad_a, size_t n, int norm, void* stream);
/* add_noise: out = X + thr * Normal(0, 1/6), counter-based generator keyed by (seed, element-pair index).  X == NULL
 * stands for zeros: ac_add_noise(NULL, g, out, n, seed) is the gradient of add_noise with respect to the threshold
 * (the gradient with respect to X is g itself). */
AC_API int ac_add_noise(const float* X, const float* thr, float* out, size_t n, uint64_t seed, void* stream);

/* ------------------------------------------------------------------------------------------
 * Placed buffers (see the performance note at the top).  ac_workspace_create allocates, straight
 * from the HIP runtime, device buffers for batches of B clips x K blocks x C channels of this (mdct, psy) pair:
 *   region A = [copies x (X [B,K+1,N,C] | t [B,K+1,1,C]) | x [B,K*N,C]],   region B = [copies x (thr like X | xhat [B,(K+2)*N,C])]
 * and places region B for the MI355X's HBM: up to max_tries candidate allocations are timed with the fused encode itself
 * (median of three launches on noise, device warmed first), untouched spacers of 12 GiB (at most span_gib in all) move
 * each next candidate along the VRAM, the search stops at the first candidate that reaches the two-class rate or once two
 * candidates differ by the gap between the classes; the fastest stays, every other allocation and every spacer is back
 * with the driver before the call returns.  The one entry point (with ac_probe_placement) that synchronises.  Memory
 * held afterwards: exactly the two regions (ac_workspace_regions).  copies > 1 gives double-buffered outputs.
 * ac_workspace_buffers returns the tensors of copy `copy` (any pointer argument may be NULL); x is filled with
 * uniform(-1, 1) noise by the probe.  Results of the kernels do not depend on where their buffers live.
 * ---------------------------------------------------------------------------------------- */
typedef struct ac_workspace ac_workspace;
AC_API int ac_workspace_create(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int B, int K, int C, int copies, int max_tries,
                               double span_gib, void* stream, ac_workspace** out);
AC_API int ac_workspace_buffers(const ac_workspace* ws, int copy, float** x, float** X, float** t, float** thr, float** xhat);
AC_API int ac_workspace_regions(const ac_workspace* ws, void** a, size_t* bytes_a, void** b, size_t* bytes_b);
/* tries made, index of the chosen one, encode time of every try in ms (encode_ms: room for 16 floats), spacer memory
 * held for a moment during the search in GiB */
AC_API int ac_workspace_report(const ac_workspace* ws, int* tries, int* chosen, float* encode_ms, double* spacer_gib);
AC_API int ac_workspace_destroy(ac_workspace* ws);
/* The two regions as a pool: a float32 tensor of `shape` (ndim <= 8, compact row-major) carved out of region 0 (A: spectra)
 * or 1 (B: thresholds, PCM), returned as a DLManagedTensor* (dlpack.h) whose deleter gives the memory back -- what
 * torch.from_dlpack / any DLPack consumer turns into a tensor that owns its storage.  A released extent is handed out again
 * only for work on the stream its last tenant was allocated for (same-stream order is execution order).  NULL when the
 * region has no room: the caller then allocates elsewhere.  Once used, the fixed tensors of ac_workspace_buffers overlap
 * the pool's and must not be used; ac_workspace_destroy defers freeing the regions until the last tensor is released.
 * ac_workspace_live: tensors handed out and not yet released.
 * ac_workspace_record_stream: the pool's counterpart of torch's Tensor.record_stream (which a DLPack tensor's storage does not
 * reach): tells the pool that the tensor starting at `data` is also used by work on `stream`.  When the tensor dies, the pool
 * records an event on every such stream and the extent's next tenant -- whatever stream it is allocated for -- waits for them
 * first, so a consumer on a side stream that drops its last reference early cannot have the memory rewritten under it.
 * AC_EINVAL when `data` is not the start of a live tensor of this pool. */
AC_API void* ac_workspace_alloc_dlpack(ac_workspace* ws, int region, int ndim, const int64_t* shape, void* stream);
AC_API long ac_workspace_live(ac_workspace* ws);
AC_API int ac_workspace_record_stream(ac_workspace* ws, const void* data, void* stream);

/* The probe on its own: runs ac_encode_fused with each of the n caller-owned candidate threshold buffers (x, X, t fixed;
 * contents of X, t and the candidates are overwritten), times every candidate with HIP events (median of three launches
 * after one warm-up) and returns the index of the fastest in *best and, when ms is not NULL, the n times in milliseconds. */
AC_API int ac_probe_placement(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const float* x, float* X, float* t,
                       float* const* thr_candidates, int n_candidates, int B, int K, int C, void* stream, int* best,
                       float* ms);

/* ------------------------------------------------------------------------------------------
 * compute_dtype variants (mdctransformer.py:13-14,22-23; psychoacoustic.py:14-15,30,42-43: the reference accepts
 * float64 / float32 / bfloat16 and requires the inputs to be of that type).  Same shapes and layouts as the float32
 * entry points; `dtype` names the element type of every tensor argument:
 *   AC_F32   the float32 entry points above (wave-level / LDS-FFT / generic kernels);
 *   AC_F64   float64 tensors, float64 arithmetic and float64 constants throughout (O(N^2) DCT-IV, any even
 *            filters_n): the on-device oracle the tests hold the float32 kernels against at full size;
 *   AC_BF16  bfloat16 tensors (half the bytes of float32), float32 arithmetic inside: the wave-level kernels for mono
 *            and stereo at filters_n 1024 / 2048 (conversion fused into their loads and stores; the fused encode rounds
 *            X and the tonality to bfloat16 before the masking model uses them, so fused and un-fused calls agree),
 *            else the LDS-FFT kernels for filters_n from 16 to 4096 with a 5-smooth half and the O(N^2) kernels; results carry
 *            bfloat16's output rounding (2^-9 relative) -- more accurate than the reference's all-bfloat16 op sequence.
 *   AC_F16   float16 tensors, float32 arithmetic inside; the filter bank only (ac_mdct_forward_typed / ac_mdct_inverse_typed:
 *            MDCTransformer accepts it and up-casts inside its DCT-IV, mdctransformer.py:327-344; PsychoacousticModel refuses it
 *            by name, psychoacoustic.py:42-43 -- the masking entry points return AC_EINVAL): the 8-byte LDS-FFT kernels for
 *            filters_n from 16 to 4096 with a 5-smooth half, else the O(N^2) kernels; results carry float16's rounding
 *            (2^-11 relative) and range (a coefficient beyond 65504 becomes infinity, as a cast makes it).
 *
 * Non-finite inputs (all dtypes): the filter bank is linear arithmetic -- a NaN or infinite sample makes every coefficient
 * of the two frames that contain it NaN (as the reference's dense products do).  The masking model follows tf.maximum /
 * tf.minimum, which propagate NaN (psychoacoustic.py:113-116, 205-208, 331): a frame and signal with a NaN or infinite
 * intensity has a NaN tonality, and a NaN intensity or a NaN tonality makes the whole threshold row of that frame and signal
 * NaN; every other frame and the other signal are untouched.  One corner differs: intensities that overflow float32
 * (|X| > 1.8e19) with a caller-supplied finite tonality give NaN thresholds where the reference has infinities.  Denormal
 * inputs are ordinary numbers (nothing is flushed on the way in; intensities below 1e-14 meet the model's floor).
 * Streaming (ac_stream_*_typed) serves AC_F32 and AC_F64 at every size (float64: a state of its own in double, the float64
 * kernels) and AC_BF16 where the wave-level kernels do (filters_n 1024 / 2048, mono / stereo; the state stays float32);
 * chunked results equal the one-shot calls bit for bit.  Backward passes: the filter bank through ac_mdct_plan_adjoint and
 * the typed forward entry points in every dtype; the masking model through the *_backward_typed entry points below.
 * ---------------------------------------------------------------------------------------- */
AC_API int ac_mdct_forward_typed(const ac_mdct_plan* plan, const void* x, void* X, int dtype, int B, int K, int C, void* stream);
AC_API int ac_mdct_inverse_typed(const ac_mdct_plan* plan, const void* X, void* x, int dtype, int B, int Kp, int C, void* stream);
AC_API int ac_tonality_typed(const ac_psy_plan* plan, const void* X, void* t, int dtype, int B, int F, int C, void* stream);
AC_API int ac_mask_threshold_typed(const ac_psy_plan* plan, const void* X, const void* t, double drown, void* thr, int dtype,
                            int B, int F, int C, void* stream);
/* the adjoints of the two (ac_tonality_backward / ac_mask_threshold_backward on tensors of `dtype`: the reference's op chain is
 * differentiable in every dtype it accepts, psychoacoustic.py:311): AC_F64 in float64 throughout, AC_BF16 bfloat16 tensors with
 * float32 arithmetic; grad_X is overwritten (no accumulate form) */
AC_API int ac_tonality_backward_typed(const ac_psy_plan* plan, const void* X, const void* grad_t, void* grad_X, int dtype, int B, int F,
                                      int C, void* stream);
AC_API int ac_mask_threshold_backward_typed(const ac_psy_plan* plan, const void* X, const void* t, double drown, const void* grad_thr,
                                            void* grad_X, void* grad_t, int dtype, int B, int F, int C, void* stream);
AC_API int ac_encode_fused_typed(const ac_mdct_plan* mdct, const ac_psy_plan* psy, const void* x, void* X, void* t, void* thr,
                          double drown, int dtype, int B, int K, int C, void* stream);
/* ac_stream_forward / ac_stream_encode (psy may be NULL: then t, thr are ignored) and ac_stream_inverse on tensors of `dtype` */
AC_API int ac_stream_encode_typed(ac_stream* s, const ac_psy_plan* psy, const void* x_chunk, void* X, void* t, void* thr,
                                  double drown, int dtype, int k, void* stream);
AC_API int ac_stream_inverse_typed(ac_stream* s, const void* X_chunk, void* x, int dtype, int k, void* stream);
/* Packed rows in a stream (extension): AC_PACKED is a format of the SPECTRUM side of the two calls above and
 * of nothing else -- every other *_typed entry point rejects it as a dtype.  The PCM side is float32 (or, out of the decoder,
 * 16-bit PCM); the overlap state is the float32 state ac_stream_encode / ac_stream_inverse keep, in the same pair of buffers, so
 * chunk calls of every form may follow each other on one ac_stream and ac_stream_settle / ac_stream_run find the state.
 *   ac_stream_encode_typed(s, psy, x_chunk, X, NULL, NULL, drown, AC_PACKED, k, stream): x_chunk float32 [B,k*N,C]; X addresses
 *     one ac_packed_out (its row_bytes must be the plan's ceil(row_bits / 32) * 4, else AC_EINVAL); psy must carry a row budget
 *     (AC_EINVAL otherwise) and t, thr must be NULL.  Writes data [B k C row_bytes] and fits [B,k,C]: row r = (b k + f) C + c,
 *     frame f of the chunk being frame (blocks so far + f) of the stream, holds the bytes AC_EMIT_PACKED writes for that frame
 *     -- ac_pack's bytes then zeros, or the marked row.  k == 0 is AC_OK.
 *   ac_stream_inverse_typed(s, X_chunk, x, AC_PACKED, k, stream): X_chunk addresses one ac_stream_packed_in; x is float32 or
 *     int16 [B,k*N,C] per pcm16.  Bit-equal to ac_unpack, ac_dequantize, ac_stream_inverse (pcm16: that result through
 *     ac_mdct_inverse_pcm16's store: 0 if NaN else clamp(rint(fp32(32768 x)), -32768, 32767)); damaged rows and row starts outside
 *     data read as ac_unpack reads them.
 * Each is ONE launch where ac_stream_packed_launches returns 1, and AC_EUNSUPPORTED elsewhere, with the state untouched: compose
 * it from ac_stream_encode, ac_quantize_budget (row_bits_out > 8 row_bytes: fill the row's sf with -128) and ac_pack at row
 * starts r row_bytes into zero-filled data; from ac_unpack, ac_dequantize and ac_stream_inverse.
 * ac_stream_packed_launches(s, psy, decode): library launches of a chunk on this stream.  decode = 0: 1 where
 *   ac_encode_packed_launches is 1 for the stream's channels and the kernel instance with streaming state passed its register
 *   gate (stereo with the f32 spreading product did not), else ac_encode_launches + 2.  decode != 0: 1 where
 *   ac_decode_packed_launches is 1, else 3 (decode = 2: of the concealing decode, decode = 3: of the recovering one, below).  AC_ENCODE_PACKED_NOFUSE=1 / AC_DECODE_PACKED_NOFUSE=1 apply as they do one-shot
 *   (read per call).  0 for NULL or mismatched arguments, or (decode = 0) a plan without a row budget.
 * 16-bit PCM into the encoder: ac_stream_encode_typed(..., dtype = AC_PACKED | AC_IN_PCM16 (48), ...) takes x_chunk as int16
 *   [B,k*N,C], x = pcm / 32768: the rows, and the float32 state it leaves, are those of the AC_PACKED call on that float32
 *   chunk.  ONE launch where ac_stream_packed_launches_pcm16(s, psy) returns 1 -- where ac_encode_packed_launches is 1 and the
 *   16-bit instance with streaming state passed its register gate (mono and stereo with the f32 spreading product did not) --
 *   and AC_EUNSUPPORTED elsewhere, with the state untouched; the query then returns ac_encode_launches + 2 (convert the chunk
 *   and compose as above), or 0 as ac_stream_packed_launches does.  No other *_typed entry point takes the value. */
enum { AC_PACKED = 16 };   /* ac_stream_encode_typed / ac_stream_inverse_typed: the spectra are packed rows */
typedef struct ac_stream_packed_in {
  ac_packed_rows rows;      /* data, nbytes, index [B,k,C] */
  const ac_psy_plan* psy;   /* the band layout of the rows */
  int32_t pcm16;            /* 0: x is float32 [B,k*N,C]; 1: int16 */
} ac_stream_packed_in;
/* Lost rows concealed in a stream (extension; DESIGN.md section 8f, "Streams"): AC_CONCEAL is a flag beside AC_PACKED for
 * ac_stream_inverse_typed and nothing else.
 *   ac_stream_inverse_typed(s, X_chunk, x, AC_PACKED | AC_CONCEAL (144), k, stream): X_chunk addresses one
 *     ac_stream_packed_lost_in.  lost uint8 [B,k,C] (nonzero: the row did not arrive), max_age in [0, AC_CONCEAL_MAX_AGE].  The
 *     stream carries, per clip and channel, the last row that arrived (its first 2152 bytes, bytes outside data as 0) and the
 *     gap g in [0, 32]: the frames since it at the end of the previous chunk, 32 = none within reach.  Row (b, f, c) is read
 *     from index[b, f-a, c] for the smallest a in [0, min(max_age, f)] with lost[b, f-a, c] == 0; else from the carried row,
 *     with age g + f + 1, where g <= 31 and that age <= max_age; else it is silence.  Scale factors fade as ac_conceal fades
 *     them.  So the chunk calls of any split give the blocks ac_decode_quantized with an ac_conceal gives for the whole signal,
 *     bit for bit.  Afterwards: the last row of the chunk that arrived is carried with g = min(32, k-1 - its frame); none
 *     arrived: g = min(32, g + k).  AC_EINVAL for max_age outside its range, a NULL lost, an unaligned pointer or pcm16 not 0 /
 *     1.  k == 0 is AC_OK and leaves the state.  The state is allocated by the first such call, zeroed on its stream, and freed
 *     with the stream; ac_stream_reset resets it.  Every other call that advances the synthesis state (ac_stream_inverse,
 *     ac_stream_inverse_typed without AC_CONCEAL, ac_stream_run) leaves no source: the next concealing call reads g = 32.
 *   ONE launch where ac_stream_packed_launches(s, psy, 2) returns 1 (where decode = 1 does); AC_EUNSUPPORTED elsewhere, with all
 *   state untouched, and the query returns 3: ac_unpack, ac_dequantize, ac_stream_inverse, with the fade and the carried row
 *   kept by the caller. */
enum { AC_CONCEAL = 128 };   /* ac_stream_inverse_typed, beside AC_PACKED: rows marked in lost are concealed */
typedef struct ac_stream_packed_lost_in {
  ac_stream_packed_in in;
  const uint8_t* lost;      /* [B,k,C]: nonzero = the row did not arrive */
  int32_t max_age;          /* 0 .. AC_CONCEAL_MAX_AGE */
} ac_stream_packed_lost_in;
/* Lost rows recovered in a stream (extension; DESIGN.md section 8g, "Streams"): in the call above, a max_age that is not negative
 * and has AC_CONCEAL_REDUNDANT set marks X_chunk as the longer ac_stream_packed_recover_in, whose leading members are
 * ac_stream_packed_lost_in's; max_age is the rest of the field.  redundant_at outside [1, 2^31) is AC_EINVAL.
 *   A delayed stream: the k blocks written are the frames of D, row 0, ..., row k-2, where D is the deferred row -- the last row
 *     of the chunk before; on a new or reset stream a row that did not arrive and has no source before it -- and the chunk's last
 *     row becomes the next D.  A frame that is lost (D: g != 0) and whose successor in the chunk arrived (of D: row 0; of row f:
 *     row f+1) is read from index[b, successor, c] + redundant_at as ac_unpack reads any start, with no fade.  Every other frame
 *     as AC_CONCEAL alone reads it, D from the carried row where g == 0.  The state afterwards is the one AC_CONCEAL alone
 *     leaves for rows 0 .. k-1.  So the chunk calls of any split of index [B,K',C] give blocks 0 .. K'-1 of ac_decode_quantized
 *     with an ac_conceal_redundant on that index and lost with one lost frame put in front (index[:, :1], 1), bit for bit;
 *     block K' is a last chunk of one row marked lost (any index, data may be empty), after which ac_stream_reset is due.
 *   Mode: from its first such chunk until ac_stream_reset a stream is delayed, and every other call that advances the synthesis
 *     (ac_stream_inverse, ac_stream_inverse_typed in any other form, ac_stream_run) and ac_stream_settle are AC_EINVAL; so is such a chunk on a stream
 *     whose synthesis one of those calls has advanced since it was created or reset.  A refused call leaves all state untouched.
 *   ONE launch where ac_stream_packed_launches(s, psy, 3) returns 1 (where decode = 1 does); AC_EUNSUPPORTED elsewhere, with all
 *   state untouched, and the query returns 3: ac_unpack, ac_dequantize, ac_stream_inverse, with the plan of sources, the fade, the
 *   carried and the deferred row kept by the caller. */
/*   (A caller's ac_stream_packed_lost_in whose max_age has the bit set, valid or not, is read as the longer struct: 8 bytes
 *   past its end.  Keep the bit out of a max_age that is not meant to carry it.) */
typedef struct ac_stream_packed_recover_in {
  ac_stream_packed_in in;
  const uint8_t* lost;      /* [B,k,C]: nonzero = the row did not arrive */
  int32_t max_age;          /* (0 .. AC_CONCEAL_MAX_AGE) | AC_CONCEAL_REDUNDANT */
  int64_t redundant_at;     /* bytes from a row's start to the copy of the row before it, in [1, 2^31) */
} ac_stream_packed_recover_in;
AC_API int ac_stream_packed_launches(const ac_stream* s, const ac_psy_plan* psy, int decode);
AC_API int ac_stream_packed_launches_pcm16(const ac_stream* s, const ac_psy_plan* psy);
AC_API int ac_amplitude_to_db_typed(const void* a, void* out, size_t n, int norm, int dtype, void* stream);
AC_API int ac_add_noise_typed(const void* X, const void* thr, void* out, size_t n, uint64_t seed, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AUDIOCODEC_AMD_H */
