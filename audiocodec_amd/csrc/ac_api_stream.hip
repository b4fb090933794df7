// C ABI, streaming: everything that takes an ac_stream -- create / reset / destroy, the chunk calls on float32, typed and
// packed tensors, settle and run.
#include "ac_api_internal.h"

using namespace ac;

extern "C" {

// Every chunk call ends in one of these two: the kernels wrote the new state into the second buffer of its pair, so the pair
// swaps roles.  The tail's swap also settles the concealment state, which nothing else may assign per
// chunk: a concealing chunk wrote its other half, now current; any other synthesis left it behind the signal, stale.
// recovering: the chunk was synthesised one frame behind its rows ("Streams"), which sets the stream's mode.
static void advance_prev(ac_stream* s) { std::swap(s->d_prev_block, s->d_prev_tmp); }
static void advance_tail(ac_stream* s, bool concealed, bool recovering = false) {
  std::swap(s->d_tail, s->d_tail_tmp);
  if (concealed) s->conceal_cur ^= 1;
  s->conceal_stale = !concealed;
  (recovering ? s->delayed : s->advanced) = true;
}
// every call that advances the synthesis as it is, on a stream whose recovering chunks run one frame behind
#define AC_REQUIRE_NOT_DELAYED(s, what)                                                                                          \
  AC_REQUIRE(!(s)->delayed, "%s on a stream that decodes recovering chunks, one frame behind its rows (AC_CONCEAL_REDUNDANT): " \
             "flush it and call ac_stream_reset first", what)

int ac_stream_create(const ac_mdct_plan* plan, int B, int C, ac_stream** out) {
  AC_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  AC_REQUIRE(plan != nullptr, "plan is NULL");
  AC_REQUIRE(B >= 1 && C >= 1, "B (%d) and C (%d) must be positive", B, C);
  DeviceGuard guard(plan->device);
  ac_stream* s = new_or_error<ac_stream>();
  if (!s) return AC_ENOMEM;
  s->plan = plan;
  s->B = B;
  s->C = C;
  s->N = plan->N;
  s->device = plan->device;
  const size_t nb = (size_t)B * plan->N * C * sizeof(float);
  const size_t nt = (size_t)B * C * (plan->N / 2) * sizeof(float);
  hipError_t e = hipMalloc((void**)&s->d_prev_block, nb);
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_prev_tmp, nb);
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_tail, nt);
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_tail_tmp, nt);
  if (e == hipSuccess) e = hipMemset(s->d_prev_block, 0, nb);
  if (e == hipSuccess) e = hipMemset(s->d_prev_tmp, 0, nb);
  if (e == hipSuccess) e = hipMemset(s->d_tail, 0, nt);
  if (e == hipSuccess) e = hipMemset(s->d_tail_tmp, 0, nt);
  if (e == hipSuccess) e = creation_sync();   // (the zeroing has run before any chunk call can)
  if (e != hipSuccess) {
    set_error("stream state allocation failed: %s", hipGetErrorString(e));
    ac_stream_destroy(s);
    return e == hipErrorOutOfMemory ? AC_ENOMEM : AC_EHIP;
  }
  s->d_prev_home = s->d_prev_block;
  s->d_tail_home = s->d_tail;
  *out = s;
  return AC_OK;
}

int ac_stream_reset(ac_stream* s, void* stream) {
  AC_REQUIRE(s != nullptr, "stream is NULL");
  DeviceGuard guard(s->device);
  if (s->d_prev_block != s->d_prev_home) std::swap(s->d_prev_block, s->d_prev_tmp);   // the zero state lives at home
  if (s->d_tail != s->d_tail_home) std::swap(s->d_tail, s->d_tail_tmp);
  const size_t nb = (size_t)s->B * s->N * s->C * sizeof(float);
  const size_t nt = (size_t)s->B * s->C * (s->N / 2) * sizeof(float);
  AC_HIP_CHECK(hipMemsetAsync(s->d_prev_block, 0, nb, (hipStream_t)stream));
  AC_HIP_CHECK(hipMemsetAsync(s->d_tail, 0, nt, (hipStream_t)stream));
  if (s->d_prev64) AC_HIP_CHECK(hipMemsetAsync(s->d_prev64, 0, 2 * nb, (hipStream_t)stream));
  if (s->d_tail64) AC_HIP_CHECK(hipMemsetAsync(s->d_tail64, 0, 2 * nt, (hipStream_t)stream));
  s->conceal_stale = true;   // (the concealment state, where there is one: the next concealing chunk reads every gap as 32)
  s->delayed = s->advanced = false;
  return AC_OK;
}

int ac_stream_destroy(ac_stream* s) {
  if (!s) return AC_OK;
  DeviceGuard guard(s->device);   // (not s->plan->device: the plan may already be gone when a process tears down)
  (void)hipFree(s->d_prev_block);
  (void)hipFree(s->d_prev_tmp);
  (void)hipFree(s->d_tail);
  (void)hipFree(s->d_tail_tmp);
  (void)hipFree(s->d_prev64);
  (void)hipFree(s->d_tail64);
  (void)hipFree(s->d_tail64_tmp);
  (void)hipFree(s->d_conceal);
  delete s;
  return AC_OK;
}

// analysis of one chunk, with or without the masking model; the wave-level kernels write the new state (the chunk's last
// block) themselves into the second state buffer, the other tiers take a strided copy
static int stream_analysis(ac_stream* s, const ac_psy_plan* psy, const float* x_chunk, float* X, float* t, float* thr,
                           float drown, int k, void* stream) {
  AC_REQUIRE(s != nullptr, "stream is NULL");
  AC_REQUIRE(k >= 0, "negative chunk length %d", k);
  if (k == 0) return AC_OK;
  AC_REQUIRE(x_chunk != nullptr && X != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(x_chunk, X, thr);
  const ac_mdct_plan* p = s->plan;
  int st = AC_OK;
  if (psy) {
    AC_REQUIRE(t != nullptr && thr != nullptr, "NULL tensor pointer");
    st = check_plan_pair(p, psy);
  }
  if (st) return st;
  DeviceGuard guard(s->device);
  hipStream_t hs = (hipStream_t)stream;
  const bool fast = wave_level(p, s->C, 0, k);
  // (filters_n = 2048 mono: the fused kernel is not instantiated, see encode_fused; filters_n 64 ... 512: the masking model
  // for general band layouts rides in the several-frames-per-wave kernels)
  const bool fused = psy && fast && ((psy_fast_serves(psy, s->C) && fast_mdct_frames_per_wave(p->N) == 1 && !fused_encode_takes_two_launches(p->N, s->C, 0)) ||
                                     fast_multi_fuses(p, psy, s->C, 0, k));
  if (fast) {
    st = launch_fwd_fast(p, fused ? psy : nullptr, x_chunk, false, X, fused ? t : nullptr, fused ? thr : nullptr, drown,
                         s->d_prev_block, s->B, k, k, s->C, hs, s->d_prev_tmp);
    if (st) return st;
    advance_prev(s);
  } else {
    st = launch_fwd_typed(p, x_chunk, X, s->d_prev_block, AC_F32, s->B, k, k, s->C, hs);
    if (st) return st;
    // new state = last block of the chunk, per clip: B rows of N*C floats, source pitch k*N*C floats
    const size_t row = (size_t)p->N * s->C * sizeof(float);
    AC_HIP_CHECK(hipMemcpy2DAsync(s->d_prev_block, row, x_chunk + (size_t)(k - 1) * p->N * s->C, row * k, row,
                                  (size_t)s->B, hipMemcpyDeviceToDevice, hs));
  }
  if (psy && !fused) {
    // the same second step encode_fused takes for these configurations (so that chunked and one-shot results agree bit
    // for bit): tonality + threshold in one wave-level pass over X, or the two generic kernels
    if (psy_fast_serves(psy, s->C)) return launch_psy_fast(psy, X, nullptr, t, thr, drown, s->B, k, s->C, hs);
    if (psy_mid_serves(psy, s->C)) return launch_psy_mid(psy, X, nullptr, t, thr, drown, s->B, k, s->C, hs);
    st = ac_tonality(psy, X, t, s->B, k, s->C, stream);
    if (!st) st = ac_mask_threshold(psy, X, t, drown, thr, s->B, k, s->C, stream);
  }
  return st;
}

int ac_stream_forward(ac_stream* s, const float* x_chunk, float* X, int k, void* stream) {
  return stream_analysis(s, nullptr, x_chunk, X, nullptr, nullptr, 0.f, k, stream);
}

int ac_stream_encode(ac_stream* s, const ac_psy_plan* psy, const float* x_chunk, float* X, float* t, float* thr,
                     float drown, int k, void* stream) {
  AC_REQUIRE(psy != nullptr, "plan is NULL");
  return stream_analysis(s, psy, x_chunk, X, t, thr, drown, k, stream);
}

int ac_stream_inverse(ac_stream* s, const float* X_chunk, float* x, int k, void* stream) {
  AC_REQUIRE(s != nullptr, "stream is NULL");
  AC_REQUIRE(k >= 0, "negative chunk length %d", k);
  if (k == 0) return AC_OK;
  AC_REQUIRE(X_chunk != nullptr && x != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(X_chunk, x);
  AC_REQUIRE_NOT_DELAYED(s, "ac_stream_inverse");
  const ac_mdct_plan* p = s->plan;
  DeviceGuard guard(s->device);
  hipStream_t hs = (hipStream_t)stream;
  int st;
  if (wave_level(p, s->C, 0, k))
    st = launch_inv_fast(p, X_chunk, x, false, s->d_tail, s->d_tail_tmp, s->B, k, k, s->C, hs);
  else
    st = launch_inv_typed(p, X_chunk, x, s->d_tail, s->d_tail_tmp, AC_F32, s->B, k, k, s->C, hs);
  if (!st) advance_tail(s, false);
  return st;
}

// The state buffers swap roles with every chunk; after an odd number of chunks the current state sits in the other
// buffer.  ac_stream_settle moves it back to the stream's home buffers (one small device copy per state, none when it is
// already there).  ac_stream_run settles on entry and on exit, so the launches of a call captured into a HIP graph
// address the home buffers, and a replay reads and writes the same addresses as the captured call -- provided the state is
// at home when the replay starts: after chunk calls (ac_stream_forward / _encode / _inverse), call ac_stream_settle first.
static int settle_state(ac_stream* s, hipStream_t hs) {
  DeviceGuard guard(s->device);
  s->conceal_stale = true;   // (what follows -- ac_stream_run, or a replay the library never sees -- advances d_tail and conceals nothing)
  if (s->d_prev_block != s->d_prev_home) {
    AC_HIP_CHECK(hipMemcpyAsync(s->d_prev_home, s->d_prev_block, (size_t)s->B * s->N * s->C * sizeof(float), hipMemcpyDeviceToDevice, hs));
    std::swap(s->d_prev_block, s->d_prev_tmp);
  }
  if (s->d_tail != s->d_tail_home) {
    AC_HIP_CHECK(hipMemcpyAsync(s->d_tail_home, s->d_tail, (size_t)s->B * s->C * (s->N / 2) * sizeof(float), hipMemcpyDeviceToDevice, hs));
    std::swap(s->d_tail, s->d_tail_tmp);
  }
  return AC_OK;
}

int ac_stream_settle(ac_stream* s, void* stream) {
  AC_REQUIRE(s != nullptr, "stream is NULL");
  AC_REQUIRE_NOT_DELAYED(s, "ac_stream_settle");   // (it would leave no source: the deferred row would be lost unseen)
  return settle_state(s, (hipStream_t)stream);
}

int ac_stream_run(ac_stream* s, const ac_psy_plan* psy, int nchunks, int k, const float* const* x_chunks,
                  float* const* X_chunks, float* const* t_chunks, float* const* thr_chunks, float* const* xhat_chunks,
                  float drown, void* stream) {
  AC_REQUIRE(s != nullptr, "stream is NULL");
  AC_REQUIRE(nchunks >= 0 && k >= 0, "negative chunk count / length (%d, %d)", nchunks, k);
  if (nchunks == 0 || k == 0) return AC_OK;
  AC_REQUIRE_NOT_DELAYED(s, "ac_stream_run");   // (with or without synthesis: it settles the state, which leaves no source)
  AC_REQUIRE(x_chunks != nullptr && X_chunks != nullptr, "NULL chunk list");
  AC_REQUIRE(psy == nullptr || (t_chunks != nullptr && thr_chunks != nullptr), "NULL chunk list");
  for (int i = 0; i < nchunks; ++i) {
    AC_REQUIRE(x_chunks[i] != nullptr && X_chunks[i] != nullptr, "chunk %d: NULL tensor pointer", i);
    AC_REQUIRE(psy == nullptr || (t_chunks[i] != nullptr && thr_chunks[i] != nullptr), "chunk %d: NULL tensor pointer", i);
    AC_REQUIRE(xhat_chunks == nullptr || xhat_chunks[i] != nullptr, "chunk %d: NULL tensor pointer", i);
    AC_REQUIRE_ALIGNED(x_chunks[i], X_chunks[i], psy ? thr_chunks[i] : nullptr, xhat_chunks ? xhat_chunks[i] : nullptr);
  }
  // Small chunks with synthesis (one clip, a few hundred frames per chunk): the analysis of chunk i + 1 rides in the same
  // launch as the synthesis of chunk i (k_duplex_fast) -- the two are independent, and a chunk's two dependent launches
  // of ~8 us each are latency, not bandwidth.  (Synthesis on a second HIP stream beside the analysis was measured slower
  // on MI355X: 25-30 us per chunk of 256 stereo frames against 17-20 us -- a cross-stream event hop costs more than
  // the ~7 us kernel it would hide; DESIGN_LOG.md section 7.)  Same kernel bodies: the results equal the chain's.
  const ac_mdct_plan* p = s->plan;
  hipStream_t hs = (hipStream_t)stream;
  int st = psy ? check_plan_pair(p, psy) : AC_OK;
  if (!st) st = settle_state(s, hs);   // the state at its home buffers on entry and again on exit
  if (st) return st;
  bool duplex = xhat_chunks && nchunks >= 2 && wave_level(p, s->C, 0, k) && fast_duplex_serves(p, psy, s->B, s->C, k, k);
  if (duplex) {
    // the two halves of a launch must not touch each other's tensors: a caller that reuses one X (or PCM) buffer for
    // consecutive chunks gets the dependent chain
    const size_t nX = (size_t)s->B * k * p->N * s->C, nt = (size_t)s->B * k * s->C;
    auto apart = [](const float* a, size_t na, const float* b, size_t nb) { return a + na <= b || b + nb <= a; };
    for (int i = 0; i + 1 < nchunks && duplex; ++i) {
      duplex = apart(X_chunks[i], nX, X_chunks[i + 1], nX) && apart(xhat_chunks[i], nX, x_chunks[i + 1], nX) &&
               apart(xhat_chunks[i], nX, X_chunks[i + 1], nX) && apart(X_chunks[i], nX, x_chunks[i + 1], nX);
      if (duplex && psy)
        duplex = apart(X_chunks[i], nX, thr_chunks[i + 1], nX) && apart(xhat_chunks[i], nX, thr_chunks[i + 1], nX) &&
                 apart(X_chunks[i], nX, t_chunks[i + 1], nt) && apart(xhat_chunks[i], nX, t_chunks[i + 1], nt);
    }
  }
  if (duplex) {
    DeviceGuard guard(s->device);
    st = stream_analysis(s, psy, x_chunks[0], X_chunks[0], psy ? t_chunks[0] : nullptr, psy ? thr_chunks[0] : nullptr, drown,
                         k, stream);
    for (int i = 0; i + 1 < nchunks && !st; ++i) {
      st = launch_duplex_fast(p, psy, x_chunks[i + 1], X_chunks[i + 1], psy ? t_chunks[i + 1] : nullptr,
                              psy ? thr_chunks[i + 1] : nullptr, drown, s->d_prev_block, s->d_prev_tmp, k, X_chunks[i],
                              xhat_chunks[i], s->d_tail, s->d_tail_tmp, k, s->B, s->C, hs);
      if (!st) {
        advance_prev(s);
        advance_tail(s, false);
      }
    }
    if (!st) st = ac_stream_inverse(s, X_chunks[nchunks - 1], xhat_chunks[nchunks - 1], k, stream);
    return st ? st : settle_state(s, hs);
  }
  for (int i = 0; i < nchunks && !st; ++i) {
    st = stream_analysis(s, psy, x_chunks[i], X_chunks[i], psy ? t_chunks[i] : nullptr, psy ? thr_chunks[i] : nullptr,
                         drown, k, stream);
    if (!st && xhat_chunks) st = ac_stream_inverse(s, X_chunks[i], xhat_chunks[i], k, stream);
  }
  return st ? st : settle_state(s, hs);
}

// ---- streaming on bfloat16 tensors: the wave-level kernels (filters_n 1024 / 2048, mono / stereo) with the conversion in
// their loads and stores; the state stays float32 (a bfloat16 block is exact in it, the aliased half is kept unrounded),
// so chunked results equal the one-shot *_typed calls bit for bit
// float64 streams: the state in double (allocated by the first float64 call), the float64 kernels (O(N^2), any even size).
// The state is zeroed on the CALL's stream, ahead of the chunk's kernels in the same queue: a synchronous hipMemset would
// go to the null stream, which nothing orders with a caller's non-blocking stream.
static int stream_state64(ac_stream* s, hipStream_t hs) {
  if (s->d_prev64) return AC_OK;
  const size_t nb = (size_t)s->B * s->N * s->C * sizeof(double), nt = (size_t)s->B * s->C * (s->N / 2) * sizeof(double);
  hipError_t e = hipMalloc((void**)&s->d_prev64, nb);
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_tail64, nt);
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_tail64_tmp, nt);
  if (e == hipSuccess) e = hipMemsetAsync(s->d_prev64, 0, nb, hs);
  if (e == hipSuccess) e = hipMemsetAsync(s->d_tail64, 0, nt, hs);
  if (e == hipSuccess) e = hipMemsetAsync(s->d_tail64_tmp, 0, nt, hs);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("float64 stream state allocation failed: %s", hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? AC_ENOMEM : AC_EHIP;
  }
  return AC_OK;
}
static int stream_typed_check(const ac_stream* s, int dtype, int k) {
  AC_REQUIRE(s != nullptr, "stream is NULL");
  AC_REQUIRE_DTYPE(dtype);
  AC_REQUIRE(k >= 0, "negative chunk length %d", k);
  if (dtype == AC_F64) return AC_OK;
  if (!(s->plan->fast && fast_mdct_frames_per_wave(s->N) == 1 && s->C <= 2 && !g_force_generic)) {
    set_error("streaming on bfloat16 tensors is served by the wave-level kernels only (filters_n 1024 / 2048, mono / stereo); "
              "float32 and float64 streams take every size");
    return AC_EUNSUPPORTED;
  }
  return AC_OK;
}

// ---- packed rows in a stream (AC_PACKED): a chunk of k blocks to k fixed-stride packed rows per signal
// and back, one launch each, on the float32 state of the stream
// (16-bit PCM chunks, AC_PACKED | AC_IN_PCM16: k_fwd_fast_qps16 has a register gate of its own)
static bool stream_encode_packed_fuses(const ac_stream* s, const ac_psy_plan* psy, bool pcm16) {
  return encode_packed_fuses(s->plan, psy, s->C) &&
         (pcm16 ? fast_encode_pack_stream_pcm16_serves : fast_encode_pack_stream_serves)(s->plan, psy, s->C);
}

int ac_stream_packed_launches(const ac_stream* s, const ac_psy_plan* psy, int decode) {
  if (!s || !plans_match(s->plan, psy)) return 0;
  // ac_unpack, ac_dequantize, ac_stream_inverse (decode == 2, concealing: the fade between them is the caller's; decode == 3,
  // recovering first, one frame behind: so are the plan and the deferred row)
  if (decode == 3) return decode_packed_fuses(s->plan, psy, s->C) && fast_inv_packed_recover_stream_serves(s->plan, psy, s->C) ? 1 : 3;
  if (decode == 2) return decode_packed_fuses(s->plan, psy, s->C) && fast_inv_packed_conceal_stream_serves(s->plan, psy, s->C) ? 1 : 3;
  if (decode) return decode_packed_fuses(s->plan, psy, s->C) ? 1 : 3;
  if (!psy->row_bits) return 0;
  // ac_stream_encode, ac_quantize_budget, ac_pack
  return stream_encode_packed_fuses(s, psy, false) ? 1 : ac_encode_launches(s->plan, psy, s->C) + 2;
}

int ac_stream_packed_launches_pcm16(const ac_stream* s, const ac_psy_plan* psy) {
  if (!s || !plans_match(s->plan, psy) || !psy->row_bits) return 0;
  return stream_encode_packed_fuses(s, psy, true) ? 1 : ac_encode_launches(s->plan, psy, s->C) + 2;
}

static int stream_encode_packed(ac_stream* s, const ac_psy_plan* psy, const void* x_chunk, bool pcm16, const ac_packed_out* out,
                                const void* t, const void* thr, double drown, int k, void* stream) {
  AC_REQUIRE(s != nullptr, "stream is NULL");
  AC_REQUIRE(psy != nullptr, "AC_PACKED needs the masking model's plan");
  AC_REQUIRE(k >= 0, "negative chunk length %d", k);
  const ac_mdct_plan* p = s->plan;
  int st = check_plan_pair(p, psy);
  if (st) return st;
  AC_REQUIRE(psy->row_bits != 0, "AC_PACKED needs a plan with a row budget (ac_psy_plan_with_row_budget)");
  AC_REQUIRE(t == nullptr && thr == nullptr, "AC_PACKED writes no t or thr: they must be NULL");
  AC_REQUIRE(out != nullptr, "AC_PACKED without its ac_packed_out (X)");
  const ac_packed_out po = *out;
  st = check_row_bytes(po, psy);
  if (st) return st;
  if (k == 0) return AC_OK;
  if (!stream_encode_packed_fuses(s, psy, pcm16)) {
    set_error("AC_PACKED: no kernel encodes a chunk%s to packed rows in one launch for filters_n = %d, bark_bands_n = %d, %d "
              "channels, row budget %d here (ac_stream_packed_launches%s() != 1): use the composition -- ac_stream_encode%s, "
              "ac_quantize_budget, then ac_pack at row starts r * row_bytes into zero-filled data",
              pcm16 ? " of 16-bit PCM" : "", p->N, psy->M, s->C, psy->row_bits, pcm16 ? "_pcm16" : "",
              pcm16 ? " on pcm / 32768 as float32" : "");
    return AC_EUNSUPPORTED;
  }
  st = check_quant(psy, s->B, k, s->C);
  if (st) return st;
  AC_REQUIRE(po.data != nullptr && po.fits != nullptr && x_chunk != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(x_chunk, po.data);
  DeviceGuard guard(s->device);
  st = (pcm16 ? launch_fwd_fast_pack_rows_stream_pcm16 : launch_fwd_fast_pack_rows_stream)(
      p, psy, x_chunk, (float)drown, po.data, po.row_bytes, po.fits, s->d_prev_block, s->d_prev_tmp, s->B, k, s->C, (hipStream_t)stream);
  if (!st) advance_prev(s);
  return st;
}

// the concealment state of a stream (AC_PACKED | AC_CONCEAL): allocated and zeroed -- the padding behind every carried row stays
// zero from here on -- by the first concealing call, on that call's stream
static size_t conceal_gap_bytes(const ac_stream* s) { return ((size_t)s->B * (size_t)s->C + 15) / 16 * 16; }
static int stream_conceal_state(ac_stream* s, hipStream_t hs) {
  if (s->d_conceal) return AC_OK;
  const size_t n = 2 * (conceal_state_row_bytes(s->B, s->C) + conceal_gap_bytes(s));
  hipError_t e = hipMalloc((void**)&s->d_conceal, n);
  if (e == hipSuccess) e = hipMemsetAsync(s->d_conceal, 0, n, hs);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(s->d_conceal);
    s->d_conceal = nullptr;
    set_error("concealment state allocation failed: %s", hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? AC_ENOMEM : AC_EHIP;
  }
  return AC_OK;   // (conceal_cur is 0 and conceal_stale true: only a concealing chunk, which needs this buffer, changes that)
}

// A chunk of packed rows through the synthesis (AC_PACKED), with the rows marked lost concealed (AC_PACKED | AC_CONCEAL): there
// X_chunk addresses an ac_stream_packed_lost_in, which begins with the ac_stream_packed_in of the plain form.  A max_age there
// that is not negative and has AC_CONCEAL_REDUNDANT set marks the longer ac_stream_packed_recover_in: the chunk recovers before it
// conceals and is synthesised one frame behind its rows ("Streams").
static int stream_inverse_packed(ac_stream* s, const void* X_chunk, bool conceal, void* x, int k, void* stream) {
  AC_REQUIRE(s != nullptr, "stream is NULL");
  AC_REQUIRE(k >= 0, "negative chunk length %d", k);
  AC_REQUIRE(X_chunk != nullptr || !conceal, "AC_PACKED | AC_CONCEAL without its ac_stream_packed_lost_in (X_chunk)");
  AC_REQUIRE(X_chunk != nullptr, "AC_PACKED without its ac_stream_packed_in (X_chunk)");
  ac_stream_packed_lost_in li = {};
  if (conceal) li = *static_cast<const ac_stream_packed_lost_in*>(X_chunk);
  else li.in = *static_cast<const ac_stream_packed_in*>(X_chunk);
  const ac_stream_packed_in& pin = li.in;
  const ac_psy_plan* psy = pin.psy;
  const ac_mdct_plan* p = s->plan;
  AC_REQUIRE(psy != nullptr, "ac_stream_packed_in: psy is NULL");
  int st = check_plan_pair(p, psy);
  if (st) return st;
  AC_REQUIRE(pin.pcm16 == 0 || pin.pcm16 == 1, "ac_stream_packed_in: pcm16 must be 0 or 1 (got %d)", (int)pin.pcm16);
  int64_t redundant_at = 0;   // nonzero: a recovering chunk
  if (conceal) {
    if (li.max_age >= 0 && (li.max_age & AC_CONCEAL_REDUNDANT)) {
      redundant_at = static_cast<const ac_stream_packed_recover_in*>(X_chunk)->redundant_at;
      li.max_age &= ~AC_CONCEAL_REDUNDANT;
      AC_REQUIRE(redundant_at >= 1 && redundant_at <= 2147483647ll, "ac_stream_packed_recover_in: redundant_at (%lld) outside "
                 "[1, 2^31)", (long long)redundant_at);
    }
    AC_REQUIRE(li.max_age >= 0 && li.max_age <= AC_CONCEAL_MAX_AGE, "ac_stream_packed_lost_in: max_age (%d) outside [0, %d]",
               (int)li.max_age, AC_CONCEAL_MAX_AGE);
    AC_REQUIRE(li.lost != nullptr, "ac_stream_packed_lost_in: lost is NULL");
  }
  if (k == 0) return AC_OK;
  if (redundant_at) {
    AC_REQUIRE(!s->advanced, "AC_CONCEAL_REDUNDANT on a stream whose synthesis has advanced without it since it was created or "
               "reset: a recovering chunk is one frame behind its rows -- call ac_stream_reset first");
    if (ac_stream_packed_launches(s, psy, 3) != 1) {
      set_error("AC_PACKED | AC_CONCEAL with AC_CONCEAL_REDUNDANT: no kernel decodes a chunk of packed rows with lost rows recovered "
                "in one launch for filters_n = %d, bark_bands_n = %d, %d channels here (ac_stream_packed_launches(s, psy, 3) != 1): "
                "compose it from ac_unpack, the fade, ac_dequantize and ac_stream_inverse, and keep the deferred row yourself",
                p->N, psy->M, s->C);
      return AC_EUNSUPPORTED;
    }
  } else {
    AC_REQUIRE_NOT_DELAYED(s, "ac_stream_inverse_typed without AC_CONCEAL_REDUNDANT");
  }
  if (conceal && !redundant_at && ac_stream_packed_launches(s, psy, 2) != 1) {
    set_error("AC_PACKED | AC_CONCEAL: no kernel decodes a chunk of packed rows with lost rows concealed in one launch for "
              "filters_n = %d, bark_bands_n = %d, %d channels here (ac_stream_packed_launches(s, psy, 2) != 1): compose it from "
              "ac_unpack, the fade, ac_dequantize and ac_stream_inverse, and carry the last row that arrived yourself",
              p->N, psy->M, s->C);
    return AC_EUNSUPPORTED;
  }
  if (!conceal && !decode_packed_fuses(p, psy, s->C)) {
    set_error("AC_PACKED: no kernel decodes a chunk of packed rows in one launch for filters_n = %d, bark_bands_n = %d, %d "
              "channels here (ac_stream_packed_launches() != 1): use the composition -- ac_unpack, ac_dequantize, then "
              "ac_stream_inverse",
              p->N, psy->M, s->C);
    return AC_EUNSUPPORTED;
  }
  st = check_quant(psy, s->B, k, s->C);
  if (!st) st = check_packed_rows(pin.rows, true, x != nullptr);
  if (st) return st;
  AC_REQUIRE_ALIGNED(x);
  DeviceGuard guard(s->device);
  hipStream_t hs = (hipStream_t)stream;
  if (conceal) {
    st = stream_conceal_state(s, hs);
    if (st) return st;
    const size_t nr = conceal_state_row_bytes(s->B, s->C), ng = conceal_gap_bytes(s);
    uint8_t* rows[2] = {s->d_conceal, s->d_conceal + nr};
    uint8_t* gaps[2] = {s->d_conceal + 2 * nr, s->d_conceal + 2 * nr + ng};
    const int cur = s->conceal_cur;
    if (redundant_at)
      st = launch_inv_fast_packed_recover_stream(p, psy, pin.rows.data, pin.rows.nbytes, pin.rows.index, li.lost, li.max_age,
                                                 redundant_at, x, pin.pcm16 != 0, s->d_tail, s->d_tail_tmp, gaps[cur], rows[cur],
                                                 gaps[cur ^ 1], rows[cur ^ 1], s->conceal_stale, s->B, k, s->C, hs);
    else
      st = launch_inv_fast_packed_conceal_stream(p, psy, pin.rows.data, pin.rows.nbytes, pin.rows.index, li.lost, li.max_age, x,
                                                 pin.pcm16 != 0, s->d_tail, s->d_tail_tmp, gaps[cur], rows[cur], gaps[cur ^ 1],
                                                 rows[cur ^ 1], s->conceal_stale, s->B, k, s->C, hs);
  } else {
    st = launch_inv_fast_packed(p, psy, pin.rows.data, pin.rows.nbytes, pin.rows.index, x, pin.pcm16 != 0, s->d_tail, s->d_tail_tmp,
                                s->B, k, k, s->C, hs);
  }
  if (!st) advance_tail(s, conceal, redundant_at != 0);
  return st;
}

int ac_stream_encode_typed(ac_stream* s, const ac_psy_plan* psy, const void* x_chunk, void* X, void* t, void* thr, double drown,
                           int dtype, int k, void* stream) {
  if (dtype == AC_PACKED || dtype == (AC_PACKED | AC_IN_PCM16))
    return stream_encode_packed(s, psy, x_chunk, dtype != AC_PACKED, static_cast<const ac_packed_out*>(X), t, thr, drown, k, stream);
  AC_REQUIRE_DTYPE(dtype);
  if (dtype == AC_F32) {
    if (psy) return ac_stream_encode(s, psy, static_cast<const float*>(x_chunk), static_cast<float*>(X), static_cast<float*>(t),
                                     static_cast<float*>(thr), (float)drown, k, stream);
    return ac_stream_forward(s, static_cast<const float*>(x_chunk), static_cast<float*>(X), k, stream);
  }
  int st = stream_typed_check(s, dtype, k);
  if (st) return st;
  if (k == 0) return AC_OK;
  AC_REQUIRE(x_chunk != nullptr && X != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(x_chunk, X, thr);
  const ac_mdct_plan* p = s->plan;
  if (psy) {
    AC_REQUIRE(t != nullptr && thr != nullptr, "NULL tensor pointer");
    AC_REQUIRE(p->N == psy->N && p->device == psy->device, "plans do not belong together");
    AC_REQUIRE(dtype == AC_F64 || psy->fast, "internal: the masking model of this size has no bfloat16 wave-level kernels");
  }
  DeviceGuard guard(s->device);
  hipStream_t hs = (hipStream_t)stream;
  if (dtype == AC_F64) {   // analysis with the stored block -1, the new state = the chunk's last block, the model on the chunk
    st = stream_state64(s, hs);
    if (st) return st;
    const double* xd = static_cast<const double*>(x_chunk);
    st = launch_fwd_typed(p, x_chunk, X, s->d_prev64, AC_F64, s->B, k, k, s->C, hs);
    if (st) return st;
    const size_t row = (size_t)p->N * s->C * sizeof(double);
    AC_HIP_CHECK(hipMemcpy2DAsync(s->d_prev64, row, xd + (size_t)(k - 1) * p->N * s->C, row * k, row, (size_t)s->B, hipMemcpyDeviceToDevice, hs));
    if (psy) {
      st = launch_tonality_typed(psy, X, t, AC_F64, s->B, k, s->C, hs);
      if (!st) st = launch_threshold_typed(psy, X, t, drown, thr, AC_F64, s->B, k, s->C, hs);
    }
    return st;
  }
  const bool fused = psy && !fused_encode_takes_two_launches(p->N, s->C, 2);   // (as ac_encode_fused_typed)
  st = launch_fwd_fast(p, fused ? psy : nullptr, x_chunk, 2, static_cast<float*>(X), fused ? static_cast<float*>(t) : nullptr,
                       fused ? static_cast<float*>(thr) : nullptr, (float)drown, s->d_prev_block, s->B, k, k, s->C, hs, s->d_prev_tmp);
  if (st) return st;
  advance_prev(s);
  if (psy && !fused)
    st = launch_psy_fast(psy, static_cast<const float*>(X), nullptr, static_cast<float*>(t), static_cast<float*>(thr), (float)drown,
                         s->B, k, s->C, hs, 2);
  return st;
}

int ac_stream_inverse_typed(ac_stream* s, const void* X_chunk, void* x, int dtype, int k, void* stream) {
  if (dtype == AC_PACKED || dtype == (AC_PACKED | AC_CONCEAL))
    return stream_inverse_packed(s, X_chunk, dtype != AC_PACKED, x, k, stream);
  AC_REQUIRE_DTYPE(dtype);
  if (dtype == AC_F32) return ac_stream_inverse(s, static_cast<const float*>(X_chunk), static_cast<float*>(x), k, stream);
  int st = stream_typed_check(s, dtype, k);
  if (st) return st;
  if (k == 0) return AC_OK;
  AC_REQUIRE(X_chunk != nullptr && x != nullptr, "NULL tensor pointer");
  AC_REQUIRE_ALIGNED(X_chunk, x);
  AC_REQUIRE_NOT_DELAYED(s, "ac_stream_inverse_typed");
  DeviceGuard guard(s->device);
  if (dtype == AC_F64) {
    st = stream_state64(s, (hipStream_t)stream);
    if (!st) st = launch_inv_typed(s->plan, X_chunk, x, s->d_tail64, s->d_tail64_tmp, AC_F64, s->B, k, k, s->C, (hipStream_t)stream);
    if (st) return st;
    std::swap(s->d_tail64, s->d_tail64_tmp);
    s->advanced = true;
    return AC_OK;
  }
  st = launch_inv_fast(s->plan, static_cast<const float*>(X_chunk), x, 2, s->d_tail, s->d_tail_tmp, s->B, k, k, s->C, (hipStream_t)stream);
  if (!st) advance_tail(s, false);
  return st;
}

}  // extern "C"
