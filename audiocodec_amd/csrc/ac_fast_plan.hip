// Host side of the wave-level kernels (ac_fast_dev.h): the table images of the transforms and of the masking model, what
// the tier serves, and the grid helpers of its launchers.  No kernels; a .hip file so that the table builders keep the
// floating-point contraction they were always compiled with.
#include <cmath>
#include <cstring>
#include <vector>

#include "ac_fast.h"
#include "ac_fast_psy_dev.h"

namespace ac {

template <int R>
static bool build_mdct_fast_R(int N, const FoldCoef& c, std::vector<float>* out) {
  using G = Geo<R>;
  if (N != G::FN) return false;
  const int h = N / 2;
  std::vector<float> t(2 * G::I_TOTAL, 0.f);
  float* tf = t.data();                 // analysis image
  float* ti = t.data() + G::I_TOTAL;    // synthesis image
  const double pi = 3.14159265358979323846;
  auto put2 = [](float* base, int i, double re, double im) {
    base[2 * i] = (float)re;
    base[2 * i + 1] = (float)im;
  };
  // the reference's lower-right quadrant (1 - w[N+j] w[N-1-j]) / w[j] carries ~1e-10 of fp64 cancellation noise
  auto same = [](double x, double y) { return std::fabs(x - y) <= 1e-8; };
  for (int r = 0; r < R; ++r) {
    for (int l = 0; l < 64; ++l) {
      const int i = r * 64 + l;
      const int e = l + 64 * r;                                   // input element of (lane, register)
      const int k = l + 64 * r;                                   // output bin of (lane, register)
      double ang = -pi * (e + 0.25) / N;
      put2(tf + G::I_PRE, i, std::cos(ang), std::sin(ang));
      put2(ti + G::I_PRE, i, std::cos(ang), std::sin(ang));
      ang = -2.0 * pi * (double)(l * r) / (double)G::FH;          // W_{64R}^(lane k0), k0 = r
      put2(tf + G::I_P1, i, std::cos(ang), std::sin(ang));
      put2(ti + G::I_P1, i, std::cos(ang), std::sin(ang));
      if (l < 8 && r < 8) {
        ang = -2.0 * pi * (double)(l * r) / 64.0;                 // [k1 = r][e0 = l]
        put2(tf + G::I_P2, r * 8 + l, std::cos(ang), std::sin(ang));
        put2(ti + G::I_P2, r * 8 + l, std::cos(ang), std::sin(ang));
      }
      ang = -pi * (double)k / N;
      const double sf = 1.0 / (N * std::sqrt(2.0)), si = 2.0 * std::sqrt(2.0);
      put2(tf + G::I_POST, i, std::cos(ang) * sf, std::sin(ang) * sf);
      put2(ti + G::I_POST, i, std::cos(ang) * si, std::sin(ang) * si);
      // analysis fold of element e (see k_fwd_fast): current-frame part cE xe + cO xo, carried part kE xe + kO xo
      double cE, cO, kE, kO;
      if (e < h / 2) {   // samples N/2+2e (even) / N/2-1-2e (odd); current part = v[N-1-2e], carry = v'[2e]
        const int jc = h - 1 - 2 * e, jk = 2 * e;
        cE = c.a2[jc]; cO = c.a1[jc]; kE = c.a4[jk]; kO = c.a3[jk];
        if (!same(cE, -kO) || !same(cO, kE)) return false;        // (-A, B, B, A)
      } else {           // samples 2p (even) / N-1-2p (odd), p = e-N/4: current part = v[2e], carry = v'[N-1-2e]
        const int pidx = e - h / 2;
        const int jc = 2 * pidx, jk = h - 1 - 2 * pidx;
        cE = c.a1[jc]; cO = c.a2[jc]; kE = c.a3[jk]; kO = c.a4[jk];
        if (!same(cE, kO) || !same(cO, -kE)) return false;        // (A, -B, B, A)
      }
      put2(tf + G::I_COEF, i, kO, kE);                             // (A, B)
      // synthesis unfold of output element k (see k_inv_fast): o1 = s1 now + s2 carry, o2 = s3 now + s4 carry
      const int j = (k < h / 2) ? (h - 1 - 2 * k) : (2 * k - h);
      if (!same(c.s3[j], c.s2[j]) || !same(c.s4[j], -c.s1[j])) return false;   // (a, b, b, -a)
      put2(ti + G::I_COEF, i, c.s1[j], c.s2[j]);
    }
  }
  if (out) *out = t;
  return true;
}

// Table images of the several-frames-per-wave kernels (filters_n = 16 LB, LB = 32 or 16 lanes per frame): the Geo<8>
// layout with every entry replicated to the 64 lanes, l = lane mod LB taking the place of the lane.
// *fold4 (may be null): set when some fold block is not a rotation (float32-precomputed constants, mdctransformer.py:218-221
// in float32; the rectangular window, :209-211): the kernels then take the FOLD4 form, which reads the block's other two
// coefficients from I_COEF2.  A caller that passes no fold4 gets false for such tables.
static bool build_mdct_multi(int N, const FoldCoef& c, std::vector<float>* out, bool* fold4) {
  using G = Geo<8>;
  if (N != 512 && N != 256 && N != 128 && N != 64) return false;
  const int LB = N / 16, Q2 = LB >= 8 ? LB / 8 : 1, h = N / 2, FH = 8 * LB;
  const bool two_halves = N == 64;   // input side on 8 lanes x 4 registers (see load_half), output side on LB = 4 lanes
  bool general = false;
  std::vector<float> t(2 * G::I_TOTAL, 0.f);
  float* tf = t.data();
  float* ti = t.data() + G::I_TOTAL;
  const double pi = 3.14159265358979323846;
  auto put2 = [](float* base, int i, double re, double im) {
    base[2 * i] = (float)re;
    base[2 * i + 1] = (float)im;
  };
  auto same = [](double x, double y) { return std::fabs(x - y) <= 1e-8; };
  for (int r = 0; r < 8; ++r) {
    for (int lane = 0; lane < 64; ++lane) {
      const int l = lane % LB, i = r * 64 + lane;
      const int le = two_halves ? lane % 8 : l, k0 = two_halves ? r % 4 : r;   // input side: lane of the group, pass-1 index
      const int e = two_halves ? le + 8 * (r % 4) : l + LB * r, k = l + LB * r;
      double ang = -pi * (e + 0.25) / N;
      put2(tf + G::I_PRE, i, std::cos(ang), std::sin(ang));
      put2(ti + G::I_PRE, i, std::cos(ang), std::sin(ang));
      ang = -2.0 * pi * (double)(le * k0) / (double)FH;             // pass 1: W_{8 LB}^(l k0)
      put2(tf + G::I_P1, i, std::cos(ang), std::sin(ang));
      put2(ti + G::I_P1, i, std::cos(ang), std::sin(ang));
      if (lane < 8) {
        ang = -2.0 * pi * (double)(lane * (r % Q2)) / (double)LB;   // pass 2: [k = r][m0 = lane]  W_LB^(m0 k1'), k1' = k mod Q2
        put2(tf + G::I_P2, r * 8 + lane, std::cos(ang), std::sin(ang));
        put2(ti + G::I_P2, r * 8 + lane, std::cos(ang), std::sin(ang));
      }
      ang = -pi * (double)k / N;
      const double sf = 1.0 / (N * std::sqrt(2.0)), si = 2.0 * std::sqrt(2.0);
      put2(tf + G::I_POST, i, std::cos(ang) * sf, std::sin(ang) * sf);
      put2(ti + G::I_POST, i, std::cos(ang) * si, std::sin(ang) * si);
      double cE, cO, kE, kO;
      if (e < h / 2) {
        const int jc = h - 1 - 2 * e, jk = 2 * e;
        cE = c.a2[jc]; cO = c.a1[jc]; kE = c.a4[jk]; kO = c.a3[jk];
        if (!same(cE, -kO) || !same(cO, kE)) general = true;
      } else {
        const int pidx = e - h / 2;
        const int jc = 2 * pidx, jk = h - 1 - 2 * pidx;
        cE = c.a1[jc]; cO = c.a2[jc]; kE = c.a3[jk]; kO = c.a4[jk];
        if (!same(cE, kO) || !same(cO, -kE)) general = true;
      }
      put2(tf + G::I_COEF, i, kO, kE);
      put2(tf + G::I_COEF2, i, cE, cO);
      const int j = (k < h / 2) ? (h - 1 - 2 * k) : (2 * k - h);
      if (!same(c.s3[j], c.s2[j]) || !same(c.s4[j], -c.s1[j])) general = true;
      put2(ti + G::I_COEF, i, c.s1[j], c.s2[j]);
      put2(ti + G::I_COEF2, i, c.s3[j], c.s4[j]);
    }
  }
  if (general && !fold4) return false;
  if (fold4) *fold4 = general;
  if (out) *out = t;
  return true;
}

// Builds the two table images; false when the size is not served (filters_n 1024 and 2048 are) or the window's fold
// blocks are not rotations (the rectangular "window", mdctransformer.py:209-211), which the two-coefficient fold
// cannot express.
static bool build_mdct_fast(int N, const FoldCoef& c, std::vector<float>* out, bool* fold4) {
  if (fold4) *fold4 = false;
  if (N == Geo<8>::FN) return build_mdct_fast_R<8>(N, c, out);
  if (N == Geo<16>::FN) return build_mdct_fast_R<16>(N, c, out);
  if (N == 512 || N == 256 || N == 128 || N == 64) return build_mdct_multi(N, c, out, fold4);
  return false;
}

// frames per wave of the plan's kernels: 1 (filters_n 1024 / 2048), 2 (512), 4 (256), 8 (128) or 16 (64)
int fast_mdct_frames_per_wave(int N) { return N == 512 ? 2 : N == 256 ? 4 : N == 128 ? 8 : N == 64 ? 16 : 1; }
// what the several-frames-per-wave kernels serve: float32 tensors or 16-bit PCM on the PCM side, mono or stereo, at
// least one block
bool fast_multi_serves(const ac_mdct_plan* p, int C, int iof, int blocks) {
  // (the FOLD4 kernels -- fold blocks that are not rotations -- are instantiated for float32 tensors only)
  return fast_mdct_frames_per_wave(p->N) > 1 && (C == 1 || C == 2) && (iof == 0 || (iof == 1 && !p->fold4)) && blocks >= 1;
}

// the fused encode of the several-frames-per-wave kernels: float32 mono / stereo tensors, rotation fold blocks, and a
// masking model the general-layout wave-level code serves at this size
bool fast_multi_fuses(const ac_mdct_plan* p, const ac_psy_plan* psy, int C, int iof, int blocks) {
  return psy != nullptr && psy->runs && !p->fold4 && iof == 0 && psy->N == p->N && fast_multi_serves(p, C, iof, blocks) &&
         (size_t)AC_WAVES * 16384 + 12800 + (size_t)psy->runs_lay.off_idx * 4 <= 160 * 1024;
}

bool fast_mdct_supported(int N, const FoldCoef& c) {
  bool fold4;
  return build_mdct_fast(N, c, nullptr, &fold4);
}

int fast_mdct_plan_init(ac_mdct_plan* p) {
  std::vector<float> t;
  bool fold4 = false;
  if (!build_mdct_fast(p->N, p->coef, &t, &fold4)) {
    set_error("internal: wave-level kernels not supported for this configuration");
    return AC_EUNSUPPORTED;
  }
  p->fold4 = fold4 ? 1 : 0;
  p->fast_bytes = t.size() * sizeof(float);
  return p->tables.upload(t, &p->d_fast);
}

// The wave-level epilogue needs: N = 128 R (1024 or 2048), 64 Bark bands (lane = band), every band a contiguous bin
// range whose interior weights are exactly 1, every bin overlapping at most two (adjacent) bands, a per-band constant
// W_inv on the bins that belong to one band only, and per-half gather lists of at most 24 entries.
template <int R>
static bool build_psy_fast_R(const ac_psy_plan* p, std::vector<uint32_t>* out) {
  using P = PsyGeo<R>;
  const PsyTables& t = p->host;
  const int N = t.N, M = t.M;
  if (N != P::FN || M != 64) return false;
  auto Wf = [&](int f, int j) { return (float)t.W[(size_t)f * M + j]; };
  auto Vf = [&](int j, int f) { return (float)t.W_inv[(size_t)j * N + f]; };
  std::vector<uint32_t> w(P::P_TOTAL_MF, 0u);
  auto putf = [&](int idx, float v) { uint32_t u; memcpy(&u, &v, 4); w[idx] = u; };
  auto band = [](int group, int j, int word) { return P::PL_BAND + 4 * (group * 64 + j) + word; };
  // LDS byte offset of I[f] in the wave buffer while half f / 1024 is staged (granule swizzle of psy_stage)
  auto addrI = [](int f) { const int q = (f & 1023) >> 1; return (uint32_t)(16 * (q ^ ((q >> 4) & 3)) + 8 * (f & 1)); };
  for (int j = 0; j < M; ++j) {
    int f0 = -1, f1 = -1;
    for (int f = 0; f < N; ++f)
      if (Wf(f, j) != 0.f) {
        if (f0 < 0) f0 = f;
        f1 = f;
      }
    if (f0 < 0) return false;
    for (int f = f0; f <= f1; ++f) {
      if (Wf(f, j) == 0.f) return false;
      if (f > f0 && f < f1 && Wf(f, j) != 1.0f) return false;
    }
    for (int h = 0; h < P::NH; ++h) {
      const int lo = 1024 * h, hi = lo + 1023;   // bins of this half
      const bool has0 = f0 >= lo && f0 <= hi, has1 = f1 > f0 && f1 >= lo && f1 <= hi;
      w[band(h, j, 0)] = (has0 ? addrI(f0) : (uint32_t)ZERO_OFF) | ((has1 ? addrI(f1) : (uint32_t)ZERO_OFF) << 16);
      putf(band(h, j, 1), has0 ? Wf(f0, j) : 0.f);
      putf(band(h, j, 2), has1 ? Wf(f1, j) : 0.f);
      putf(band(h, j, 3), (float)t.quiet[j]);
      // interior bins f0+1 .. f1-1 (weight 1) inside this half: single bins up to an 8-aligned boundary, whole
      // chunks, single bins
      std::vector<uint32_t> lst;
      const int a = std::max(f0 + 1, lo), b = std::min(f1 - 1, hi);
      for (int f = a; f <= b;) {
        if ((f & 7) == 0 && f + 7 <= b) {
          lst.push_back((uint32_t)(S8_OFF + 8 * ((f & 1023) >> 3)));
          f += 8;
        } else {
          lst.push_back(addrI(f));
          f += 1;
        }
      }
      if ((int)lst.size() > 2 * P::PL_HALF) return false;
      lst.resize(2 * P::PL_HALF, (uint32_t)ZERO_OFF);
      for (int hlf = 0; hlf < P::PL_HALF; ++hlf)
        w[P::PL_LST + (h * P::PL_HALF + hlf) * 64 + j] = lst[2 * hlf] | (lst[2 * hlf + 1] << 16);
    }
    putf(band(P::NH, j, 0), t.beta[j]);
  }
  // bins -> entries; nnz pattern of W and W_inv is identical (same overlap)
  std::vector<int> entry(N, -1);
  std::vector<float> rho(M, 0.f), u0(M, 0.f), u1(M, 0.f);
  std::vector<bool> have_rho(M, false);
  for (int f = 0; f < N; ++f) {
    int cnt = 0, jf = -1;
    for (int j = 0; j < M; ++j)
      if (Vf(j, f) != 0.f) {
        if (cnt == 0) jf = j;
        ++cnt;
      }
    if (cnt == 1) {
      const float v = Vf(jf, f);
      if (!have_rho[jf]) {
        rho[jf] = v;
        have_rho[jf] = true;
      } else if (std::fabs(v - rho[jf]) > 1e-6f * rho[jf]) {
        return false;
      }
      entry[f] = 2 * jf;
    } else if (cnt == 2 && jf + 1 < M && Vf(jf + 1, f) != 0.f) {
      if (u0[jf] != 0.f || u1[jf] != 0.f) return false;   // one shared bin per band boundary
      u0[jf] = Vf(jf, f);
      u1[jf] = Vf(jf + 1, f);
      entry[f] = 2 * jf + 1;
    } else {
      return false;
    }
  }
  for (int j = 0; j < M; ++j) {
    putf(band(P::NH, j, 1), rho[j]);
    putf(band(P::NH, j, 2), u0[j]);
    putf(band(P::NH, j, 3), u1[j]);
  }
  // threshold entry e lives at byte 8 e of the wave buffer; word i of lane l = offsets of bins 2q, 2q+1, q = 64 i + l
  for (int l = 0; l < 64; ++l)
    for (int i = 0; i < R; ++i) {
      const int q = 64 * i + l;
      const uint32_t e0 = 8u * (uint32_t)entry[2 * q], e1 = 8u * (uint32_t)entry[2 * q + 1];
      w[P::PL_IDX + 4 * ((i >> 2) * 64 + l) + (i & 3)] = e0 | (e1 << 16);
    }
  for (int i = 0; i < 128; ++i) putf(P::PL_G + i, (float)t.g[i]);
  // bf16 tiles for spread_mfma: copy c, entry y = rev[y - c], rev[m] = g[128 - m] (m = 1 .. 127); hi parts, then lo parts
  {
    auto bf16_rne = [](float f) { uint32_t u; memcpy(&u, &f, 4); u += 0x7fffu + ((u >> 16) & 1u); return (uint16_t)(u >> 16); };
    auto bf16_val = [](uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; };
    uint16_t* tb = reinterpret_cast<uint16_t*>(w.data() + P::PL_MF);
    for (int c = 0; c < 4; ++c)
      for (int y = 0; y < 132; ++y) {
        const int m = y - c;
        if (m < 1 || m > 127) continue;
        const float v = (float)t.g[128 - m];
        const uint16_t hi = bf16_rne(v);
        tb[(c * MF_COPY_STRIDE) / 2 + y] = hi;
        tb[(MF_TAB_BYTES + c * MF_COPY_STRIDE) / 2 + y] = bf16_rne(v - bf16_val(hi));
      }
  }
  if (out) *out = w;
  return true;
}

static bool build_psy_fast(const ac_psy_plan* p, std::vector<uint32_t>* out) {
  if (p->host.N == PsyGeo<8>::FN) return build_psy_fast_R<8>(p, out);
  if (p->host.N == PsyGeo<16>::FN) return build_psy_fast_R<16>(p, out);
  return false;
}

bool fast_psy_supported(const ac_psy_plan* p) { return build_psy_fast(p, nullptr); }

int fast_psy_plan_init(ac_psy_plan* p) {
  std::vector<uint32_t> w;
  if (!build_psy_fast(p, &w)) {
    set_error("internal: fused epilogue not supported for this configuration");
    return AC_EUNSUPPORTED;
  }
  p->fast_bytes = w.size() * sizeof(uint32_t);
  return p->tables.upload(w, reinterpret_cast<uint32_t**>(&p->d_fast));   // (words of mixed type behind a float pointer)
}

int grid_for(long long ntasks, int nw, unsigned* grid) {
  const long long g = (ntasks + nw - 1) / nw;
  if (g > 2147483647ll) {
    set_error("problem too large for one launch (%lld workgroups)", g);
    return AC_EINVAL;
  }
  *grid = (unsigned)g;
  return AC_OK;
}

// workgroups of a persistent launch: enough to fill every CU at the kernel's occupancy, a multiple of 8 (XCDs)
unsigned persistent_grid(int cus, int wg_per_cu, long long ntasks, int nw) {
  long long g = (long long)cus * wg_per_cu;
  const long long need = (ntasks + nw - 1) / nw;
  if (g > need) g = need;
  g = (g + 7) / 8 * 8;
  return (unsigned)g;
}

}  // namespace ac
