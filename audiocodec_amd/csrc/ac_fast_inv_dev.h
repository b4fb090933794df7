// Synthesis of the wave-level kernels for filters_n = 1024 / 2048 (ac_fast_dev.h): the body shared by k_inv_fast,
// k_inv_fast_q (instantiated in ac_fast_inv.hip), k_inv_fast_p (ac_fast_inv_p.hip), its concealing forms k_inv_fast_pl
// (ac_fast_inv_pl.hip), k_inv_fast_pls (ac_fast_inv_pls.hip), k_inv_fast_plr (ac_fast_inv_plr.hip) and k_inv_fast_plsr
// (ac_fast_inv_plsr.hip) and k_duplex_fast (ac_fast_fwd.hip), and
// prep_inv_fast(), the host code that fills its arguments for these objects (InvArgs has internal linkage, so no function
// can pass it between them).
#pragma once
#include <cstdlib>

#include "ac_fast.h"
#include "ac_fast_dev.h"
#include "ac_fast_inv_p_dev.h"

namespace ac {
namespace {

// ------------------------------------------------------------------------------------------------------
// synthesis
// ------------------------------------------------------------------------------------------------------
struct InvArgs {
  const float* X;          // [B, Kp, N, C]
  void* x;                 // [B, nblk*N, C] float32, or int16 PCM for the PCM16 kernels
  const float* tail_in;    // [B, C, N/2] or null
  float* tail_out;         // [B, C, N/2] or null
  const float* tab;
  int B, Kp, nblk, C, seglen, nseg;
  int rev;                 // 1: workgroups walk the spectrum from its end (AC_INV_REV tuning hook)
  long long npairs, nsig;  // see Pair
  long long ntasks;        // npairs * nseg
};

// DCT-IV of one frame held in natural order: returns (now, nxt) per output element k = lane + 64 j.
// Element e = lane + 64 r is X[2e] (granule e, this lane) + i X[N-1-2e] (granule N/2-1-e, lane 63 - lane).
template <int R>
__device__ __forceinline__ void idct_frame(const v4f (&frm)[R], char* buf, gtab_t tab, const v2f (&p1)[R], int lane,
                                           v2f (&now)[R], v2f (&nxt)[R]) {
  using G = Geo<R>;
  C2 z[R];
  {
    v2f xo_in[R], xo[R];
#pragma unroll
    for (int c = 0; c < R; ++c) xo_in[c] = v2f{frm[c].z, frm[c].w};
    rev_exchange<R - 1, R>(buf, lane, xo_in, xo);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const C2 v = {v2f{frm[r].x, frm[r].y}, xo[r]};
      z[r] = cmul(v, reinterpret_cast<const v2f*>(tab + G::I_PRE)[r * 64 + lane]);
    }
  }
  fft_wave<R>(z, buf, tab, p1, lane);
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const C2 r = cmul_negim(z[j], reinterpret_cast<const v2f*>(tab + G::I_POST)[j * 64 + lane]);
    // u[2k] = Re, u[N-1-2k] = -Im; k < N/4 (j < R/2): u[2k] belongs to this block, u[N-1-2k] to the next
    if (j < R / 2) {
      now[j] = r.re;
      nxt[j] = r.im;
    } else {
      now[j] = r.im;
      nxt[j] = r.re;
    }
  }
}

// synthesis from quantised spectra (IOF 3: float32 PCM out, 4: 16-bit PCM out): InvArgs::X addresses the int16 codes
struct QuantRows {
  const int8_t* sf;        // [B, Kp, M, C]
  const uint32_t* band32;  // [N/2]: bands of bins 2q | 2q+1 << 16
  int M;
};

template <int R, int CMODE, int NW, int IOF = 0>
__device__ __forceinline__ void inv_fast_body(const InvArgs& a, char* lds, const int bid, const int nblocks,
                                              const QuantRows* qr = nullptr, const PackedRows* pr = nullptr,
                                              const ConcealRows* cl = nullptr, const ConcealState* cs = nullptr,
                                              const RedundRows* rd = nullptr) {
  using G = Geo<R>;
  constexpr bool QUANT = IOF >= 3;
  constexpr bool PACKED = IOF >= 5;   // (IOF 5 / 6) the quantised spectra come as rows of the packed bitstream
  constexpr bool CONCEAL = IOF >= 7;  // (IOF 7 / 8) ... and a row that did not arrive is concealed (ConcealRows)
  constexpr bool DELAYED = IOF == 13 || IOF == 14;  // (IOF 13 / 14) a chunk of a stream that recovers: synthesis frame n is row n - 1
  constexpr bool CSTREAM = IOF == 9 || IOF == 10 || DELAYED;   // (IOF 9 / 10) ... with the last row of the chunks before as a source (ConcealState)
  constexpr bool REDUND = IOF >= 11;  // (IOF 11 / 12) one-shot, a lost row recovered from its successor's copy (RedundRows)
  static_assert(!PACKED || R == 8, "packed rows: filters_n = 1024");
  constexpr int OIOF = PACKED ? (IOF - 5) % 2 : QUANT ? IOF - 3 : IOF;   // format of the PCM side
  constexpr int FH = G::FH;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  load_tables<NW, WAVE_LDS, G::I_LDS, 0>(lds, a.tab + G::I_TOTAL, nullptr);
  char* buf = lds + wave * WAVE_LDS;
  gtab_t tab = reinterpret_cast<const float*>(lds + NW * WAVE_LDS);
  v2f p1[R];
  load_p1<R>(a.tab + G::I_TOTAL, lane, p1);
  const int C = a.C;
  const size_t blk = (size_t)G::FN * C;
  // Synthesis block n overlap-adds the DCT-IV of frames n and n-1, so a wave walks a short strip of consecutive output
  // blocks with the aliased half of the last frame carried in registers.  The waves of a workgroup own consecutive
  // strips: the first block of a strip is finished last, when the neighbouring wave hands over the aliased half of
  // its last frame through LDS -- only the first wave of a workgroup pays an extra DCT-IV (of the frame before its
  // strip).  Workgroups are dispatched in order, which keeps the window of memory in flight contiguous.
  constexpr bool COOP = (R == 8);   // hand-over between waves (the 2048-filter kernel has no registers to spare)
  const long long task_raw = (long long)(a.rev ? nblocks - 1 - bid : bid) * NW + wave;
  const bool valid = task_raw < a.ntasks;
  const long long task = valid ? task_raw : a.ntasks - 1;   // idle waves of the last workgroup only join the barriers
  const int sgm = (int)(task % a.nseg);
  const Pair pq = make_pair<CMODE>(task / a.nseg, C, a.nsig);
  const bool has1 = pq.has1;
  const int n0 = sgm * a.seglen;
  const int n1 = min(a.nblk, n0 + a.seglen);
  using spec_t = typename std::conditional<IOF == 2 || QUANT, int16_t, float>::type;   // storage of the spectrum
  const spec_t* X0 = reinterpret_cast<const spec_t*>(a.X) + row_off(pq.b0, a.Kp, 0, blk, pq.c0);   // frame 0 of the two signals
  const spec_t* X1 = reinterpret_cast<const spec_t*>(a.X) + row_off(pq.b1, a.Kp, 0, blk, pq.c1);
  // what a loaded frame is held as until it is transformed: float32 rows, or the raw codes and scale factors (QUANT)
  using hold_t = typename std::conditional<PACKED, PGran, typename std::conditional<QUANT, QGran, v4f>::type>::type;
  // (QUANT) the bands of the lane's bin pairs, the same in every frame: held in registers by the 1024-filter kernel; the
  // 2048-filter one (no registers to spare, and no frame in flight ahead) reads them with the frame
  constexpr bool BW_REGS = QUANT && R == 8;
  uint32_t bw[BW_REGS ? R : 1];
  if constexpr (PACKED) {
    load_bw_p<R>(*pr, lane, bw);
  } else if constexpr (BW_REGS) {
#pragma unroll
    for (int i = 0; i < R; ++i) bw[i] = qr->band32[64 * i + lane];
  }
  // (PACKED) the wave's band records of the rows of frames n0-1 .. n1-1, filled by parse_strip_p below
  uint32_t* rec = reinterpret_cast<uint32_t*>(lds + NW * WAVE_LDS + G::TAB_LDS + (PACKED ? wave * P_REC_BYTES : 0));
  auto load_frame = [&](int n, const spec_t* r0, const spec_t* r1, hold_t (&dst)[R]) {
    if constexpr (PACKED) {
      load_row_p<R, CSTREAM>(*pr, rec, n - (n0 - 1), bw, has1, dst, cs);
    } else if constexpr (QUANT) {
      const size_t mc = (size_t)qr->M * C;
      const int8_t* sf0 = qr->sf + row_off(pq.b0, a.Kp, n, mc, pq.c0);
      const int8_t* sf1 = qr->sf + row_off(pq.b1, a.Kp, n, mc, pq.c1);
      if constexpr (BW_REGS) {
        load_row_q<CMODE, R>(r0, r1, sf0, sf1, bw, has1, lane, dst);
      } else {
        uint32_t bl[R];
#pragma unroll
        for (int i = 0; i < R; ++i) bl[i] = qr->band32[64 * i + lane];
        load_row_q<CMODE, R>(r0, r1, sf0, sf1, bl, has1, lane, dst);
      }
    } else if constexpr (IOF == 2) load_row_h<Bf16Fmt, CMODE, R>(r0, r1, C, has1, lane, dst);
    else load_row<CMODE, R>(r0, r1, C, has1, lane, dst);
  };
  const size_t ts0 = ((size_t)pq.b0 * C + pq.c0) * FH, ts1 = ((size_t)pq.b1 * C + pq.c1) * FH;   // stream state rows
  constexpr bool AHEAD = (R == 8);   // the next frame in flight while the current one is transformed
  const bool left = valid && n0 >= 1;              // block n0 needs the aliased half of frame n0-1 ...
  const bool deferred = COOP && left && wave > 0;  // ... which the previous wave (strip sgm-1 of the same signals) hands over

  // block n from the current frame's half (now) and the previous frame's aliased half (cin):
  // with (a, b) = COEF[k]: o1 = a now + b cin -> out[j], o2 = b now - a cin -> out[N-1-j]  
  // k < N/4: j = N/2-1 - 2k (odd: granule N/4-1-k, lane 63 - lane), N-1-j = N/2 + 2k (even: granule N/4+k, this lane)
  // else     j = 2k - N/2 (even: granule k - N/4, this lane),       N-1-j = 3N/2-1 - 2k (odd: granule 3N/4-1-k)
  auto emit = [&](int n, const v2f (&now)[R], const v2f (&cin)[R]) {
    v4f row[R];
    v2f xe[R], xo_in[R], xo[R];
#pragma unroll
    for (int j2 = 0; j2 < R; ++j2) {
      const v2f ab = reinterpret_cast<const v2f*>(tab + G::I_COEF)[j2 * 64 + lane];
      const v2f o1 = ab.x * now[j2] + ab.y * cin[j2];
      const v2f o2 = ab.y * now[j2] - ab.x * cin[j2];
      xe[(j2 + R / 2) & (R - 1)] = (j2 < R / 2) ? o2 : o1;
      xo_in[j2] = (j2 < R / 2) ? o1 : o2;
    }
    rev_exchange<R / 2 - 1, R>(buf, lane, xo_in, xo);
#pragma unroll
    for (int i = 0; i < R; ++i) row[i] = v4f{xe[i].x, xe[i].y, xo[i].x, xo[i].y};
    const size_t o0 = row_off(pq.b0, a.nblk, n, blk, pq.c0), o1 = row_off(pq.b1, a.nblk, n, blk, pq.c1);
    if constexpr (OIOF != 0)
      store_row_h<typename RowFmt<OIOF>::type, CMODE, R>(static_cast<int16_t*>(a.x) + o0, static_cast<int16_t*>(a.x) + o1, C, has1, lane, row);
    else store_row<CMODE, R>(static_cast<float*>(a.x) + o0, static_cast<float*>(a.x) + o1, C, has1, lane, row);
  };

  v2f carry[R], now0[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    carry[r] = v2f{0.f, 0.f};
    now0[r] = v2f{0.f, 0.f};
  }
  if constexpr (PACKED) {
    // slot 0 is frame n0-1, read only by a wave that transforms it itself
    if (valid)
      parse_strip_p<CONCEAL, CSTREAM, REDUND>(*pr, pq.b0, pq.b1, pq.c0, pq.c1, a.Kp, C, n0 - 1 - (DELAYED ? 1 : 0), (left && !deferred) ? 0 : 1,
                                              min(n1, a.Kp) - (n0 - 1), has1, lane, buf, rec, cl, cs, rd);
  }
  if (valid) {
    hold_t ahead[R];
    if (left && !deferred) {
      // aliased half of frame n0-1 (always an existing frame: n0-1 < Kp)
      hold_t row[R];
      load_frame(n0 - 1, X0 + (size_t)(n0 - 1) * blk, X1 + (size_t)(n0 - 1) * blk, row);
      if (AHEAD && n0 < a.Kp) load_frame(n0, X0 + (size_t)n0 * blk, X1 + (size_t)n0 * blk, ahead);
      v2f dummy[R];
      if constexpr (PACKED) {
        QGran g[R];
        v4f frm[R];
        extract_row_p<R>(rec, 0, bw, has1, row, g);
        dequant_frame<R>(g, frm);
        idct_frame<R>(frm, buf, tab, p1, lane, dummy, carry);
      } else if constexpr (QUANT) {
        v4f frm[R];
        dequant_frame<R>(row, frm);
        idct_frame<R>(frm, buf, tab, p1, lane, dummy, carry);
      } else {
        idct_frame<R>(row, buf, tab, p1, lane, dummy, carry);
      }
    } else {
      if (AHEAD && n0 < a.Kp) load_frame(n0, X0 + (size_t)n0 * blk, X1 + (size_t)n0 * blk, ahead);
      if (!left && a.tail_in) {
#pragma unroll
        for (int j2 = 0; j2 < R; ++j2) {
          const int k = lane + 64 * j2;
          const int j = (j2 < R / 2) ? (FH - 1 - 2 * k) : (2 * k - FH);
          carry[j2].x = a.tail_in[ts0 + j];
          carry[j2].y = has1 ? a.tail_in[ts1 + j] : 0.f;
        }
      }
    }

    for (int n = n0; n < n1; ++n) {
      v2f now[R], nxt[R];
      if (n < a.Kp) {
        if (!AHEAD) load_frame(n, X0 + (size_t)n * blk, X1 + (size_t)n * blk, ahead);
        if constexpr (PACKED) {
          QGran g[R];
          v4f frm[R];
          extract_row_p<R>(rec, n - (n0 - 1), bw, has1, ahead, g);
          dequant_frame<R>(g, frm);
          idct_frame<R>(frm, buf, tab, p1, lane, now, nxt);
        } else if constexpr (QUANT) {   // (the frame's loads were issued one frame earlier: the waits land here)
          v4f frm[R];
          dequant_frame<R>(ahead, frm);
          idct_frame<R>(frm, buf, tab, p1, lane, now, nxt);
        } else {
          idct_frame<R>(ahead, buf, tab, p1, lane, now, nxt);
        }
        if (AHEAD && n + 1 < n1 && n + 1 < a.Kp)
          load_frame(n + 1, X0 + (size_t)(n + 1) * blk, X1 + (size_t)(n + 1) * blk, ahead);
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          now[r] = v2f{0.f, 0.f};
          nxt[r] = v2f{0.f, 0.f};
        }
      }
      if (deferred && n == n0) {
#pragma unroll
        for (int r = 0; r < R; ++r) now0[r] = now[r];   // finished after the hand-over
      } else {
        emit(n, now, carry);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) carry[r] = nxt[r];
    }

    if (a.tail_out && n1 == a.nblk) {
#pragma unroll
      for (int j2 = 0; j2 < R; ++j2) {
        const int k = lane + 64 * j2;
        const int j = (j2 < R / 2) ? (FH - 1 - 2 * k) : (2 * k - FH);
        a.tail_out[ts0 + j] = carry[j2].x;
        if (has1) a.tail_out[ts1 + j] = carry[j2].y;
      }
    }
    if constexpr (CSTREAM) {   // ... and the concealment state with it
      if (n1 == a.nblk) carry_state_p(*pr, *cl, *cs, pq.b0, pq.b1, pq.c0, pq.c1, a.Kp, C, has1, lane);
    }
  }

  if (COOP) {
    // hand the aliased half of the strip's last frame to the wave that owns the next strip
    wave_sync();
    if (valid) {
#pragma unroll
      for (int r = 0; r < R; ++r) *reinterpret_cast<v2f*>(buf + 8 * lane + 512 * r) = carry[r];
    }
    __syncthreads();
    v2f cin[R];
    if (deferred) {
#pragma unroll
      for (int r = 0; r < R; ++r) cin[r] = *reinterpret_cast<const v2f*>(buf - WAVE_LDS + 8 * lane + 512 * r);
    }
    __syncthreads();   // every hand-over has been read: the buffers may be reused for the last exchange
    if (deferred) emit(n0, now0, cin);
  }
}

template <int R, int CMODE, int NW, int IOF = 0>
__global__ __launch_bounds__(NW * 64, ((IOF == 2 || (IOF == 1 && !(R == 8 && CMODE != 1))) ? 2 : wpe<R, CMODE>())) void k_inv_fast(InvArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[NW * WAVE_LDS + Geo<R>::TAB_LDS];
  inv_fast_body<R, CMODE, NW, IOF>(a, lds, (int)blockIdx.x, (int)gridDim.x);
}

// the same synthesis reading quantised spectra (IOF 3 / 4, mono / stereo); its own kernel, so the instances above keep their
// launch bounds and arguments
template <int R, int CMODE, int NW, int IOF>
__global__ __launch_bounds__(NW * 64, 2) void k_inv_fast_q(InvArgs a, QuantRows qr) {
  static_assert(IOF == 3 || IOF == 4, "quantised spectra");
  __shared__ __attribute__((aligned(16))) char lds[NW * WAVE_LDS + Geo<R>::TAB_LDS];
  inv_fast_body<R, CMODE, NW, IOF>(a, lds, (int)blockIdx.x, (int)gridDim.x, &qr);
}

// the same synthesis reading rows of the packed bitstream (IOF 5 / 6, filters_n = 1024 with 64 bands, mono / stereo): the band
// records of a wave's strip live behind the tables.  Strips of at most P_SLOTS - 1 blocks (launch_inv_fast_packed sees to it)
template <int R, int CMODE, int NW, int IOF>
__global__ __launch_bounds__(NW * 64, 2) void k_inv_fast_p(InvArgs a, PackedRows pr) {
  static_assert(R == 8 && (IOF == 5 || IOF == 6), "packed rows");
  __shared__ __attribute__((aligned(16))) char lds[NW * WAVE_LDS + Geo<R>::TAB_LDS + NW * P_REC_BYTES];
  inv_fast_body<R, CMODE, NW, IOF>(a, lds, (int)blockIdx.x, (int)gridDim.x, nullptr, &pr);
}

// arguments and grid of the one-frame-per-wave synthesis kernels (filters_n 1024 / 2048)
static int prep_inv_fast(const ac_mdct_plan* p, const float* X, void* x, int iof, const float* tail_in, float* tail_out,
                         int B, int Kp, int nblk, int C, InvArgs& a, unsigned& grid) {
  if (iof == 2 && C > 2) {
    set_error("internal: no wave-level synthesis kernel for bfloat16 tensors with %d channels", C);
    return AC_EUNSUPPORTED;
  }
  a.X = X;
  a.x = x;
  a.tail_in = tail_in;
  a.tail_out = tail_out;
  a.tab = p->d_fast;
  a.B = B;
  a.Kp = Kp;
  a.nblk = nblk;
  a.C = C;
  a.nsig = (long long)B * C;
  a.npairs = (C == 2) ? (long long)B : (a.nsig + 1) / 2;
  a.seglen = pick_seglen(a.npairs, nblk, (p->N == Geo<8>::FN && C == 2) ? 2 : 3);
  // small launches (a streaming chunk of one clip): one block per strip, so that the blocks spread over the chip
  if (a.npairs * ((nblk + a.seglen - 1) / a.seglen) < (long long)AC_WAVES * p->cus * 2) a.seglen = pick_seglen(a.npairs, nblk, 1);
  a.nseg = (nblk + a.seglen - 1) / a.seglen;
  a.ntasks = a.npairs * a.nseg;
  static const int inv_rev = [] { const char* e = getenv("AC_INV_REV"); return e ? atoi(e) : 0; }();
  a.rev = inv_rev;
  // one strip per wave, workgroups dispatched in order (persistent waves drift apart and measured slower here)
  return grid_for(a.ntasks, AC_WAVES, &grid);
}

// ... and of the kernels that read packed rows (k_inv_fast_p, k_inv_fast_pl): strips of at most P_SLOTS - 1 blocks
static int prep_inv_fast_packed(const ac_mdct_plan* p, const ac_psy_plan* psy, const uint8_t* data, int64_t nbytes,
                                const int64_t* index, void* x, bool pcm16, const float* tail_in, float* tail_out, int B, int Kp,
                                int nblk, int C, InvArgs& a, PackedRows& pr, unsigned& grid) {
  int st = prep_inv_fast(p, nullptr, x, pcm16 ? 1 : 0, tail_in, tail_out, B, Kp, nblk, C, a, grid);
  if (st) return st;
  if (a.seglen > P_SLOTS - 1) {   // (AC_SEGLEN asked for longer strips than a wave holds band records for)
    a.seglen = P_SLOTS - 1;
    a.nseg = (a.nblk + a.seglen - 1) / a.seglen;
    a.ntasks = a.npairs * a.nseg;
    st = grid_for(a.ntasks, AC_WAVES, &grid);
    if (st) return st;
  }
  pr.data = data;
  pr.nbytes = nbytes;
  pr.index = index;
  pr.band32 = reinterpret_cast<const uint32_t*>(psy->d_qband);
  pr.off = psy->d_qoff;
  return AC_OK;
}

}  // namespace
}  // namespace ac
