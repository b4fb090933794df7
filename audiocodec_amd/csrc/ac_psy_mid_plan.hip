// Host side of the wave-level masking model for general band layouts: the table images of the band walk (build_mid; read by
// k_psy_mid, ac_psy_mid.hip) and of the run-structured form (build_runs; ac_psy_runs_dev.h), what the tier serves and the
// launch-time parameters of a plan's images.  No kernels; a .hip file so that the table builders keep the floating-point
// contraction they were always compiled with.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ac_psy_mid_launch.h"

namespace ac {

using namespace mid;

namespace {

struct MidLayout {
  int wi_w = 0, off_S = 0, off_band = 0, off_wbe = 0, off_wi = 0, words = 0;
};

bool build_mid(const ac_psy_plan* p, std::vector<uint32_t>* out, MidLayout* lay) {
  const PsyTables& t = p->host;
  const int N = t.N, M = t.M;
  if (N < 2 || N > 4096 || (N & 1) || M < 1 || M > 64) return false;
  SparseRows wb, wi;
  w_by_band(t, wb);
  winv_by_bin(t, wi);
  if (wi.max_row < 1 || wi.max_row > 16) return false;   // (filters_n = 64 at 48 kHz: a 375 Hz bin spans nine Bark bands)
  MidLayout L;
  L.wi_w = wi.max_row;
  L.off_S = 0;
  L.off_band = L.off_S + 2 * (MF_TAB_BYTES / 4);
  L.off_band = (L.off_band + 3) / 4 * 4;                  // 16-byte aligned rows of four words
  L.off_wbe = L.off_band + 4 * 64;                        // (16-byte aligned: off_band is, and so is every band's start)
  // a band's weights cover the run of bins from its first to its last non-zero (zeros in between, if any, stay zeros)
  std::vector<int> first(M, 0), count(M, 0), start(M, 0);
  int total = 0;
  for (int j = 0; j < M; ++j) {
    if (wb.ptr[j + 1] > wb.ptr[j]) {
      int lo = N, hi = -1;
      for (int e = wb.ptr[j]; e < wb.ptr[j + 1]; ++e) {
        lo = std::min(lo, (int)wb.idx[e]);
        hi = std::max(hi, (int)wb.idx[e]);
      }
      first[j] = lo;
      count[j] = hi - lo + 1;
    }
    start[j] = total;
    total += (count[j] + 3) / 4 * 4;   // (a band's weights: a multiple of four, zero-padded)
  }
  if (total > 4 * N + 4 * M) return false;   // (bands that each span most of the spectrum: not a Bark mapping; other tiers)
  L.off_wi = L.off_wbe + total;
  L.off_wi = (L.off_wi + 3) / 4 * 4;                      // 16-byte reads: the entries of two adjacent bins
  L.words = L.off_wi + 2 * N * L.wi_w;
  L.words = (L.words + 3) / 4 * 4;
  std::vector<uint32_t> w((size_t)L.words, 0u);
  auto putf = [&](int i, float v) { uint32_t u; memcpy(&u, &v, 4); w[(size_t)i] = u; };
  // S is Toeplitz by construction; the kernel reads it through the prototype.  Refuse anything else.
  if ((int)t.g.size() != 2 * M) return false;
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < M; ++j)
      if ((float)t.S[(size_t)i * M + j] != (float)t.g[(size_t)(M - i + j)]) return false;
  {
    // bf16 tiles for spread_tiles: copy c, entry y = rev[y - c], rev[m] = gp[128 - m] (m = 1 .. 127), with
    // gp[64 + d] = g[M + d] where |d| < M, else 0; hi parts, then lo parts (the layout of spread_mfma in ac_fast_psy_dev.h)
    auto gp = [&](int k) { const int d = k - 64; return (d > -M && d < M) ? (float)t.g[(size_t)(M + d)] : 0.f; };
    auto bf16_rne = [](float f) { uint32_t u; memcpy(&u, &f, 4); u += 0x7fffu + ((u >> 16) & 1u); return (uint16_t)(u >> 16); };
    auto bf16_val = [](uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; };
    uint16_t* tb = reinterpret_cast<uint16_t*>(w.data() + L.off_S);
    for (int c = 0; c < 4; ++c)
      for (int y = 0; y < 132; ++y) {
        const int m = y - c;
        if (m < 1 || m > 127) continue;
        const float v = gp(128 - m);
        const uint16_t hi = bf16_rne(v);
        tb[(c * MF_COPY_STRIDE) / 2 + y] = hi;
        tb[(MF_TAB_BYTES + c * MF_COPY_STRIDE) / 2 + y] = bf16_rne(v - bf16_val(hi));
      }
  }
  for (int j = 0; j < M; ++j) {
    w[(size_t)L.off_band + 4 * j + 0] = (uint32_t)start[j];
    w[(size_t)L.off_band + 4 * j + 1] = (uint32_t)count[j] | ((uint32_t)first[j] << 16);
    putf(L.off_band + 4 * j + 2, (float)t.quiet[j]);
    putf(L.off_band + 4 * j + 3, t.beta[j]);
    for (int e = wb.ptr[j]; e < wb.ptr[j + 1]; ++e) putf(L.off_wbe + start[j] + (wb.idx[e] - first[j]), wb.val[e]);
  }
  for (int f = 0; f < N; ++f) {
    int k = 0;
    for (int e = wi.ptr[f]; e < wi.ptr[f + 1]; ++e, ++k) {
      w[(size_t)L.off_wi + 2 * ((size_t)k * N + f)] = (uint32_t)(8 * wi.idx[e]);   // byte offset of G[band]
      putf(L.off_wi + 2 * (k * N + f) + 1, wi.val[e]);
    }
  }
  if (out) *out = w;
  if (lay) *lay = L;
  return true;
}

}  // namespace

size_t mid_lds_bytes(int N, int lds_words, int nw, int fb) { return (size_t)lds_words * 4 + (size_t)nw * fb * (N >= 64 ? 8 * (size_t)N : 512); }

bool mid_psy_supported(const ac_psy_plan* p) { return build_mid(p, nullptr, nullptr); }

mid::MidParams mid_params(const ac_psy_plan* p, float drown) {
  mid::MidParams m;
  m.img_words = p->mid_words;
  m.lds_words = mid_r(p->N) >= AC_MID_WI_GLOBAL_R ? p->mid_off_wi : p->mid_words;   // (off_wi is 16-byte aligned)
  m.N = p->N;
  m.M = p->M;
  m.wi_w = p->mid_wi_w;
  m.off_S = p->mid_off_S;
  m.off_band = p->mid_off_band;
  m.off_wbe = p->mid_off_wbe;
  m.off_wi = p->mid_off_wi;
  m.alpha = (float)p->alpha;
  m.inv_alpha = (float)(1.0 / p->alpha);
  m.drown = drown;
  m.inv_n = 1.0f / (float)p->N;
  return m;
}

int mid_psy_plan_init(ac_psy_plan* p) {
  std::vector<uint32_t> w;
  MidLayout L;
  if (!build_mid(p, &w, &L)) {
    set_error("internal: wave-level masking model (general band layout) not supported for this configuration");
    return AC_EUNSUPPORTED;
  }
  p->mid_words = L.words;
  p->mid_wi_w = L.wi_w;
  p->mid_off_S = L.off_S;
  p->mid_off_band = L.off_band;
  p->mid_off_wbe = L.off_wbe;
  p->mid_off_wi = L.off_wi;
  return p->tables.upload(w, &p->d_mid);
}


// The run-structured image (ac_psy_runs_dev.h).  Host only: nothing here touches the device.
bool build_runs(const PsyTables& t, std::vector<uint32_t>* out, RunsLayout* lay) {
  const int N = t.N, M = t.M;
  if (N < 2 || N > 4096 || (N & 1) || M < 1 || M > 64) return false;
  if ((int)t.g.size() != 2 * M) return false;
  for (int i = 0; i < M; ++i)   // S is Toeplitz by construction; the kernel reads it through the prototype
    for (int j = 0; j < M; ++j)
      if ((float)t.S[(size_t)i * M + j] != (float)t.g[(size_t)(M - i + j)]) return false;
  auto Wf = [&](int f, int j) { return (float)t.W[(size_t)f * M + j]; };
  auto Vf = [&](int j, int f) { return (float)t.W_inv[(size_t)j * N + f]; };
  // bands: one contiguous run of bins, interior weights exactly 1
  std::vector<int> f0(M, -1), f1(M, -1);
  for (int j = 0; j < M; ++j) {
    for (int f = 0; f < N; ++f)
      if (Wf(f, j) != 0.f) {
        if (f0[j] < 0) f0[j] = f;
        f1[j] = f;
      }
    if (f0[j] < 0) return false;
    for (int f = f0[j]; f <= f1[j]; ++f) {
      if (Wf(f, j) == 0.f) return false;
      if (f > f0[j] && f < f1[j] && Wf(f, j) != 1.0f) return false;
    }
  }
  RunsLayout L;
  const runs::RunsGeo geo = runs::runs_geo(N);   // (the kernels derive the same numbers from filter_bands_n)
  auto a16 = [](int v) { return runs::a16(v); };
  L.n4 = geo.n4;
  L.n16 = geo.n16;
  L.o4 = geo.o4;
  L.o16 = geo.o16;
  // interior of band j as aligned runs of 64 (when use64) / 16 / 4 bins and single bins, greedily from the left
  auto list_of = [&](int j, bool use64, int o64, int oz, std::vector<uint32_t>& lst) {
    lst.clear();
    (void)oz;
    for (int f = f0[j] + 1; f <= f1[j] - 1;) {
      if (use64 && (f & 63) == 0 && f + 63 <= f1[j] - 1) {
        lst.push_back((uint32_t)(o64 + 8 * (f >> 6)));
        f += 64;
      } else if ((f & 15) == 0 && f + 15 <= f1[j] - 1) {
        lst.push_back((uint32_t)(L.o16 + 8 * (f >> 4)));
        f += 16;
      } else if ((f & 3) == 0 && f + 3 <= f1[j] - 1) {
        lst.push_back((uint32_t)(L.o4 + 8 * (f >> 2)));
        f += 4;
      } else {
        lst.push_back((uint32_t)(8 * f));
        f += 1;
      }
    }
  };
  const int o64c = geo.o64;
  int lmax[2] = {0, 0};
  std::vector<uint32_t> lst;
  for (int u = 0; u < 2; ++u)
    for (int j = 0; j < M; ++j) {
      list_of(j, u == 1, o64c, 0, lst);
      lmax[u] = std::max(lmax[u], (int)lst.size());
    }
  const bool use64 = lmax[1] + 2 <= lmax[0];   // a fourth level only where it shortens the longest list by a word
  L.n64 = use64 ? N / 64 : 0;
  L.o64 = o64c;
  L.oz = use64 ? a16(L.o64 + 8 * L.n64) : o64c;
  L.slot = a16(L.oz + 8);
  if (L.slot > 65535) return false;
  L.lw = (lmax[use64 ? 1 : 0] + 1) / 2;
  // bins -> entries
  std::vector<int> entry(N, -1), ej0(64, 0), ecnt(64, 0), ebin(64, -1);
  std::vector<float> rho(M, 0.f);
  std::vector<bool> have_rho(M, false);
  int nb = 0, kb = 1;
  for (int f = 0; f < N; ++f) {
    int cnt = 0, jf = -1, jl = -1;
    for (int j = 0; j < M; ++j)
      if (Vf(j, f) != 0.f) {
        if (cnt == 0) jf = j;
        jl = j;
        ++cnt;
      }
    if (cnt == 0 || jl - jf + 1 != cnt) return false;   // (a bin meets a run of consecutive bands)
    if (cnt == 1) {
      const float v = Vf(jf, f);
      if (!have_rho[jf]) {
        rho[jf] = v;
        have_rho[jf] = true;
      } else if (std::fabs(v - rho[jf]) > 1e-6f * rho[jf]) {
        return false;
      }
      entry[f] = 512 + 16 * jf;
    } else {
      if (nb >= 64) return false;
      ej0[nb] = jf;
      ecnt[nb] = cnt;
      ebin[nb] = f;
      kb = std::max(kb, cnt);
      entry[f] = 512 + 16 * nb + 8;
      ++nb;
    }
  }
  if (kb > 64) return false;
  L.kb = kb;
  const int R = mid_r(N);
  L.off_S = runs::OFF_S;
  L.off_bc = runs::OFF_BC;
  L.off_bd = runs::OFF_BD;
  L.off_lst = runs::OFF_LST;
  L.off_bw = runs::off_bw(L.lw);
  L.off_idx = runs::off_idx(L.lw, L.kb);   // (every part a multiple of 64 words: 16-byte aligned)
  static_assert(runs::OFF_BC % 4 == 0, "16-byte rows");
  if (L.slot > runs::runs_slot_max(N)) return false;   // (cannot happen: the compile-time strides of the fused kernels rely on it)
  L.words = (L.off_idx + 64 * R + 3) / 4 * 4;
  std::vector<uint32_t> w((size_t)L.words, 0u);
  auto putf = [&](int i, float v) { uint32_t u; memcpy(&u, &v, 4); w[(size_t)i] = u; };
  {
    auto gp = [&](int k) { const int d = k - 64; return (d > -M && d < M) ? (float)t.g[(size_t)(M + d)] : 0.f; };
    auto bf16_rne = [](float f) { uint32_t u; memcpy(&u, &f, 4); u += 0x7fffu + ((u >> 16) & 1u); return (uint16_t)(u >> 16); };
    auto bf16_val = [](uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; };
    uint16_t* tb = reinterpret_cast<uint16_t*>(w.data() + L.off_S);
    for (int c = 0; c < 4; ++c)
      for (int y = 0; y < 132; ++y) {
        const int m = y - c;
        if (m < 1 || m > 127) continue;
        const float v = gp(128 - m);
        const uint16_t hi = bf16_rne(v);
        tb[(c * MF_COPY_STRIDE) / 2 + y] = hi;
        tb[(MF_TAB_BYTES + c * MF_COPY_STRIDE) / 2 + y] = bf16_rne(v - bf16_val(hi));
      }
  }
  for (int l = 0; l < 64; ++l) {
    const int bc = L.off_bc + 4 * l, bd = L.off_bd + 4 * l;
    if (l < M) {
      const bool two = f1[l] > f0[l];
      w[(size_t)bc] = (uint32_t)(8 * f0[l]) | ((uint32_t)(two ? 8 * f1[l] : L.oz) << 16);
      putf(bc + 1, Wf(f0[l], l));
      putf(bc + 2, two ? Wf(f1[l], l) : 0.f);
      putf(bd + 0, t.beta[l] + 9.0f);
      putf(bd + 1, (float)t.quiet[l]);
      putf(bd + 2, rho[l]);
      list_of(l, use64, L.o64, L.oz, lst);
    } else {
      w[(size_t)bc] = (uint32_t)L.oz | ((uint32_t)L.oz << 16);
      lst.clear();
    }
    lst.resize((size_t)2 * L.lw, (uint32_t)L.oz);
    for (int k = 0; k < L.lw; ++k) w[(size_t)L.off_lst + 64 * k + l] = lst[2 * k] | (lst[2 * k + 1] << 16);
    // edge bin l: its bands' G are read from a window of kb that stays inside the 64 G of the slot
    if (l < nb) {
      const int js = std::min(ej0[l], 64 - L.kb);
      w[(size_t)bc + 3] = (uint32_t)(8 * js);
      for (int k = 0; k < ecnt[l]; ++k) putf(L.off_bw + 64 * (ej0[l] - js + k) + l, Vf(ej0[l] + k, ebin[l]));
    }
  }
  for (int l = 0; l < 64; ++l)
    for (int i = 0; i < R; ++i) {
      const int q = 64 * i + l;
      if (2 * q + 1 < N) w[(size_t)L.off_idx + 64 * i + l] = (uint32_t)entry[2 * q] | ((uint32_t)entry[2 * q + 1] << 16);
    }
  if (out) *out = w;
  if (lay) *lay = L;
  return true;
}

bool runs_supported(const ac_psy_plan* p) { return p->runs != 0; }

runs::RunsParams runs_params(const ac_psy_plan* p, float drown, bool idx_in_lds) {
  const RunsLayout& L = p->runs_lay;
  runs::RunsParams m;
  m.N = p->N;
  m.M = p->M;
  m.lds_words = idx_in_lds ? L.words : L.off_idx;   // (off_idx is a multiple of four words: build_runs)
  m.lw = L.lw;
  m.kb = L.kb;
  m.n64 = L.n64;
  m.oz = L.oz;
  m.slot = L.slot;
  m.alpha = (float)p->alpha;
  m.inv_alpha = (float)(1.0 / p->alpha);
  m.omd = 1.0f - drown;
  m.inv_n = 1.0f / (float)p->N;
  return m;
}

int runs_psy_plan_init(ac_psy_plan* p) {
  std::vector<uint32_t> w;
  if (!build_runs(p->host, &w, &p->runs_lay)) return AC_EUNSUPPORTED;   // (not an error: the plan keeps the band walk)
  const int st = p->tables.upload(w, &p->d_runs);
  if (!st) p->runs = 1;
  return st;
}

}  // namespace ac
