"""GPU (MI355X): every path of the masking model that reads alpha -- the compression exponent of the spreading sum
(psychoacoustic.py:14, 205-208, 223), a constructor keyword the plan carries into the kernels as a run-time value -- at
alpha 0.3 (the largest amplification, 1 / alpha = 3.33), 0.8 and 1.0 (both powers are the identity: alpha and 1 / alpha
swapped shows nowhere else), against the float64 oracle at that alpha on the kernel's own inputs.  The rest of the suite runs
the default 0.6 only; the oracle itself is pinned to the reference's own code at these alphas by
tests/golden/psy_alpha_cases.npz (test_oracle_golden.py, and test_host.py for the library's host spreading matrix).

Forward bars on the thresholds (element-wise relative): every float32 path and the split-bfloat16 spreading product
1e-4; the plain-bfloat16 product 5e-3 max(1, 0.6 / alpha) -- a relative error d of the spreading sum A becomes d / alpha in
T = A^(1/alpha) and d / (2 alpha) in the threshold, so the bar at 0.6 grows by that factor below 0.6; float64 1e-10;
bfloat16 tensors 6e-3 (the chain is of degree one in X: rounding of the tensors is not amplified by alpha).  Tonality does
not depend on alpha: conftest.tonality_err <= 1 on the float32 paths.  Every comparison also shows its bar is not vacuous:
the same kernel output against the oracle at alpha * 1.02 falls outside it.

Backward bars: those of test_psy_backward.py (psy_backward_checks.BARS) times max(1, 0.6 / alpha) -- the gradient carries
the same T / (alpha Y) factor -- with both of that module's sensitivity guards and a third: the reference gradient of a
model at alpha * 1.02 falls outside the bar as well.

Worst values measured on the MI355X over this module, at alpha 0.3 / 0.8 / 1.0 (no path was found wrong):
  * float32 forward: wave-level f32 3.5e-6 / 2.6e-6 / 2.4e-6; split bfloat16 1.5e-5 / 4.9e-6 / 4.1e-6; the run-structured
    model (mono / stereo, strided pairs, team, fused encodes) 1.5e-5 / 5.3e-6 / 4.5e-6; the band walk 1.5e-5 / 4.0e-6 /
    3.3e-6; the generic kernels 2.4e-6 / 1.8e-6 / 1.3e-6
  * plain bfloat16 product: 6.5e-3 / 2.8e-3 / 1.9e-3 (bars 1e-2 / 5e-3 / 5e-3); float64 2.0e-13; bfloat16 tensors 3.9e-3
  * gradients (peak, rel-L2): fast 9.6e-7, 5.1e-7 / 1.4e-6, 5.4e-7 / 1.2e-6, 4.9e-7; generic 7.5e-7, 2.9e-7 at worst;
    float64 1.4e-15, 4.9e-16; bfloat16 2.9e-3, 1.9e-3 / 3.6e-3, 2.4e-3 / 3.3e-3, 2.3e-3 -- all inside the bars of alpha
    0.6 even before the 1 / alpha factor.  The float32 torch restatement against itself in float64 (CPU, the shapes of
    the backward cases) is within 6.0e-7, 2.7e-7 at every alpha: the reference alone leaves the bars room.

That the module bites (scratch builds of the library, this module run against each): with 1 / alpha of the wave-level
filler (ac_fast_psy_dev.h:317) fixed at 1 / 0.6 -- bit for bit the product at alpha 0.6, so no older test can tell -- 43 of
the 109 cases fail: all of test_wave_level_model, test_wave_level_encode_stream_and_duplex and test_fast_backward, and the
1024 cases of test_two_models; with alpha and 1 / alpha swapped in runs_params (ac_psy_mid_plan.hip) 28 fail, every case
at alpha 0.3 and 0.8 of test_run_structured_model and test_fused_encode_beside_1024, the 960 cases of test_two_models and
the three-channel cases at 1024 / 2048, and none at 1.0, where the swap is the identity; with the same swap in mid_params
(same file) test_band_walk fails and nothing else.
"""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_elem, tonality_err
import psy_backward_checks as checks
from psy_backward_checks import forced_generic as _forced_generic
from wave_sizes import ENC_SIZES

import audiocodec_amd
from audiocodec_amd import _lib
from oracle.audiocodec_oracle import PsychoOracle

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the forward parity bar of test_gpu_parity.py
ALPHAS = (0.3, 0.8, 1.0)
FORMS = ("f32", "bf16x2_mfma", "bf16_mfma")
WORST = {}          # forward: path -> worst relative threshold error; backward: (path, alpha) -> (peak, rel-L2)
WORST_BWD = {}


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X (run with -m gpu on the GPU box)"
    assert _lib.load().ac_set_force_generic(0) == 0, "AC_TESTING=1 not in effect"
    yield
    _lib.load().ac_set_force_generic(0)
    if WORST:
        print("\nworst relative threshold error per path and alpha:")
        for k in sorted(WORST):
            print("  %-34s %.2e" % ("%s a=%.1f" % k, WORST[k]))
    for a in sorted(WORST_BWD):
        print("worst gradient errors (peak, rel-L2) at alpha %.1f:" % a)
        for k in sorted(WORST_BWD[a]):
            print("  %-9s %.2e  %.2e" % (k, *WORST_BWD[a][k]))


def _amp(alpha):
    """The growth of a bar below alpha 0.6: the 1 / alpha amplification relative to the default model's."""
    return max(1.0, 0.6 / alpha)


def _form_bar(spreading, alpha, C=2):
    """The bar of a spreading product (the matrix-core forms serve mono and stereo; more channels run float32)."""
    return 5e-3 * _amp(alpha) if spreading == "bf16_mfma" and C <= 2 else TOL


@functools.lru_cache(maxsize=None)
def _oracle(sr, N, M, alpha):
    return PsychoOracle(sr, N, M, alpha=alpha, compute_dtype=np.float64)


def _spectrum(seed, B, F, N, C):
    """The input of test_psy_random_vs_oracle -- a 1e-5 ... 1 envelope, per-row gains, one all-zero channel -- and one frame
    that holds a single non-zero bin (F >= 2: the two are different frames, and ordinary frames remain)."""
    assert F >= 2 and B * F * C >= 3
    rng = np.random.default_rng(seed)
    env = np.logspace(-5, 0, N).reshape(1, 1, N, 1)
    X = (rng.uniform(-1, 1, (B, F, N, C)) * env * rng.uniform(1e-3, 1, (B, F, 1, C))).astype(np.float32)
    X[0, 0, :, 0] = 0.0
    X[-1, -1, :, -1] = 0.0
    X[-1, -1, N // 3, -1] = 0.5
    return X


def _pcm(seed, B, K, N, C):
    """PCM with per-row gains and one silent channel."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty(B, K * N, C, device="cuda").uniform_(-1, 1, generator=g)
    x *= torch.empty(B, 1, C, device="cuda").uniform_(1e-3, 1, generator=g)
    x[0, :, 0] = 0.0
    return x


def _np64(t):
    return t.detach().double().cpu().numpy()


def _hold(thr, X64, t64, drown, model, alpha, bar, path):
    """thr (the kernel's) within `bar` of the oracle of `model` = (sr, N, M) at alpha on X64 / t64 -- and outside it of
    the oracle at alpha * 1.02: the bar would notice a wrong exponent."""
    thr = _np64(thr) if isinstance(thr, torch.Tensor) else np.asarray(thr, dtype=np.float64)
    assert np.isfinite(thr).all()
    err = rel_elem(thr, _oracle(*model, alpha).global_masking_threshold(X64, t64, drown))
    WORST[(path, alpha)] = max(WORST.get((path, alpha), 0.0), err)
    print("%s N=%d alpha=%.1f drown=%.1f: thr rel %.2e (bar %.1e)" % (path, model[1], alpha, drown, err, bar))
    assert err <= bar, (path, model, alpha, drown, err, bar)
    # (rel_elem is a maximum over the tensor: the guard shows that the call as a whole notices a wrong exponent, through
    # its ordinary frames.  A silent row sits on the quiet threshold and a single-bin row has one term in its spreading
    # sum, so neither depends on alpha: those rows are held by the `<= bar` side alone)
    wrong = rel_elem(thr, _oracle(*model, alpha * 1.02).global_masking_threshold(X64, t64, drown))
    assert wrong > bar, "the bar of %s does not reject the oracle at alpha * 1.02 (%.2e)" % (path, wrong)


def _hold_model(p, X, model, alpha, bar, path, drowns=(0.4,)):
    """The stand-alone calls of a float32 model -- tonality, then the threshold from it -- against the oracle."""
    t = p.tonality(X)
    X64 = _np64(X)
    assert tonality_err(t, _oracle(*model, alpha).tonality(X64)) <= 1.0, (path, model, alpha)
    for drown in drowns:
        _hold(p.global_masking_threshold(X, t, drown), X64, _np64(t), drown, model, alpha, bar, path)


def _hold_encode(X, t, thr, drown, model, alpha, bar, path):
    """The results of an encode (one launch or several) against the oracle on the kernel's own spectrum."""
    X64 = _np64(X)
    t64 = _oracle(*model, alpha).tonality(X64)
    assert tonality_err(t, t64) <= 1.0, (path, model, alpha)
    _hold(thr, X64, t64, drown, model, alpha, bar, path)


# ---- the wave-level model (ac_fast_psy_dev.h:231-256, parameters filled at :316) ------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("N,C", [(1024, 1), (1024, 2), (1024, 3), (2048, 1), (2048, 2), (2048, 3)])
def test_wave_level_model_at_other_alpha(N, C, alpha):
    """k_psy_fast (ac_fast_psy_dev.h:231-256: Q = max(eps, P)^alpha, fac = 10^(-alpha O / 10), T = (fac A)^(1/alpha), with
    alpha and 1 / alpha filled in at :316) through the stand-alone calls at filter_bands_n 1024 / 2048: mono (an odd
    number of signals), stereo and three channels, each of the three spreading products ("f32", "bf16x2_mfma",
    "bf16_mfma"), drown 0 / 0.4 / 1.  (Three channels reach both this code and, for some of the forms, the run-structured
    model of these sizes: a wrong filler of either fails the three-channel cases.)"""
    B, F = (3 if C == 1 else 2), 3
    X = torch.from_numpy(_spectrum(N + 10 * C, B, F, N, C)).cuda()
    for spreading in FORMS:
        p = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=N, alpha=alpha, spreading=spreading)
        assert p.is_fast() and p.plan_spreading() == spreading
        _hold_model(p, X, (48000, N, 64), alpha, _form_bar(spreading, alpha, C), "wave-level " + spreading, (0.0, 0.4, 1.0))


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("N,C", [(1024, 2), (1024, 1), (2048, 2), (2048, 3)])
def test_wave_level_encode_stream_and_duplex_at_other_alpha(N, C, alpha):
    """The same device code (ac_fast_psy_dev.h:231-256) inside the fused encode (AudioCodec(alpha=...).encode(): one launch
    with the filter bank), the streaming form (stream().encode_chunk, chunk by chunk) and the duplex form (stream().run with
    masking and synthesis: k_duplex_fast, stereo at 1024 with the float32 and split-bfloat16 products), each with every
    spreading product it serves: against the un-fused calls on the same spectrum and against the oracle."""
    B, K, drown, model = (3 if C == 1 else 2), 4, 0.4, (48000, N, 64)
    x = _pcm(N + C, B, K, N, C)
    for spreading in FORMS:
        bar = _form_bar(spreading, alpha, C)
        codec = audiocodec_amd.AudioCodec(48000, N, alpha=alpha, spreading=spreading)
        assert codec.psy.alpha == alpha and codec.psy.is_fast() and codec.psy.plan_spreading() == spreading
        X, t, thr = codec.encode(x, drown)
        _hold_encode(X, t, thr, drown, model, alpha, bar, "fused encode " + spreading)
        tu = codec.psy.tonality(X)
        thru = codec.psy.global_masking_threshold(X, tu, drown)
        assert tonality_err(t, tu) <= 1.0 and float(((thr - thru).abs() / thru).max()) <= bar
        _hold(thru, _np64(X), _np64(tu), drown, model, alpha, bar, "wave-level " + spreading)
        st = codec.stream(B, C)
        parts = [st.encode_chunk(x[:, a * N:b * N].contiguous(), drown=drown) for a, b in ((0, 1), (1, 4))]
        st.close()
        Xs, ts, thrs = (torch.cat([q[i] for q in parts], dim=1) for i in range(3))
        assert float((Xs - X[:, :K]).abs().max()) <= 1e-6
        _hold_encode(Xs, ts, thrs, drown, model, alpha, bar, "streaming encode " + spreading)
        if N == 1024 and C == 2 and spreading != "bf16_mfma":
            x1 = _pcm(7, 1, 12, N, C)
            x1[0, :, 0] = x1[0, :, 1].flip(0) * 0.25         # (one clip: no silent channel, the frames stay ordinary)
            st = codec.stream(1, C)
            Xd, td, thrd, xh = st.run(x1, 4, masking=True, drown=drown)
            st.close()
            Xe, te, thre = codec.encode(x1, drown)
            assert float((Xd - Xe[:, :12]).abs().max()) <= 1e-6 and tonality_err(td, te[:, :12]) <= 1.0
            assert float(((thrd - thre[:, :12]).abs() / thre[:, :12]).max()) <= bar
            assert float((xh[:, N:] - x1[:, :-N]).abs().max()) <= 1.0 / 32768.0
            _hold_encode(Xd, td, thrd, drown, model, alpha, bar, "duplex " + spreading)


# ---- the run-structured model (ac_psy_runs_dev.h, parameters: runs_params, ac_psy_mid_plan.hip) ---------------------------
RUNS = [(48000, 120, 64), (44100, 256, 48), (48000, 512, 64), (48000, 960, 64), (48000, 1920, 64), (48000, 4096, 64)]


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("sr,N,M", RUNS, ids=["%d-%d-%d" % c for c in RUNS])
def test_run_structured_model_at_other_alpha(sr, N, M, alpha, monkeypatch):
    """k_psy_runs / k_psy_runs_c: the run-structured model, which evaluates T in the log domain,
    exp2(inv_alpha max(log2 acc - alpha O log2(10) / 10, log2 eps)) -- other arithmetic than every other path, with the
    parameters of runs_params (ac_psy_mid_plan.hip).  The form the build compiles is band_tail16 (ac_psy_runs_dev.h:422-453);
    band_tail4 (:320-338) is compiled only under -DAC_SPREAD_4X4X4, which no build of the library sets, so no test reaches
    it.  One size per granule-register class (1 / 2 / 4 / 8 / 16 / 32 registers per lane: 120, 256 at 44.1 kHz with 48
    bands, 512, 960, 1920, 4096): mono and stereo, and three and six channels once as strided pairs (AC_PSY_NOTEAM=1) and,
    where a team instance exists (4 / 8 / 16 registers), in the team form (AC_PSY_TEAM_ALWAYS=1); both switches are read
    per call."""
    p = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M, alpha=alpha)
    assert p.tier() == 1 and not p.is_fast()
    team = N in (512, 960, 1920)
    cases = [(1, None), (2, None), (3, "AC_PSY_NOTEAM"), (6, "AC_PSY_NOTEAM")]
    cases += [(3, "AC_PSY_TEAM_ALWAYS"), (6, "AC_PSY_TEAM_ALWAYS")] if team else []
    for C, switch in cases:
        monkeypatch.delenv("AC_PSY_NOTEAM", raising=False)
        monkeypatch.delenv("AC_PSY_TEAM_ALWAYS", raising=False)
        if switch:
            monkeypatch.setenv(switch, "1")
        X = torch.from_numpy(_spectrum(N + C, 3 if C == 1 else 2, 3, N, C)).cuda()
        path = "runs " + {None: "mono/stereo", "AC_PSY_NOTEAM": "strided pairs", "AC_PSY_TEAM_ALWAYS": "team"}[switch]
        _hold_model(p, X, (sr, N, M), alpha, TOL, path, (0.0, 0.4, 1.0) if C == 2 else (0.4,))
    monkeypatch.delenv("AC_PSY_NOTEAM", raising=False)
    monkeypatch.delenv("AC_PSY_TEAM_ALWAYS", raising=False)


# ---- the band walk (ac_psy_mid_dev.h:237-248, parameters: mid_params, ac_psy_mid_plan.hip) -------------------------------
def test_band_walk_at_other_alpha(tmp_path):
    """k_psy_mid (ac_psy_mid_dev.h:237-248 with the parameters of mid_params, ac_psy_mid_plan.hip), reached only with
    AC_NO_RUNS=1 (read once per process): one fresh child with AC_NO_RUNS=1 and AC_LDS_WAVE_NOFUSE=1 runs filter_bands_n 120 /
    480 / 1920 in stereo, three channels and mono (an odd batch) at the three alphas -- the un-fused encode() (tonality and
    threshold in one pass) and the stand-alone calls; what it computed comes back in an .npz file and is held to the
    oracle here."""
    sizes, chans = (120, 480, 1920), (2, 3, 1)
    code = ("import sys, numpy as np, torch, audiocodec_amd\n"
            "out = {}\n"
            "for alpha in %r:\n"
            "    for N in %r:\n"
            "        for C in %r:\n"
            "            g = torch.Generator(device='cuda').manual_seed(N + C)\n"
            "            x = torch.empty(3, 3 * N, C, device='cuda').uniform_(-1, 1, generator=g)\n"
            "            x *= torch.empty(3, 1, C, device='cuda').uniform_(1e-3, 1, generator=g)\n"
            "            x[0, :, 0] = 0.0\n"
            "            codec = audiocodec_amd.AudioCodec(48000, N, alpha=alpha)\n"
            "            assert codec.psy.tier() == 1 and codec.encode_launches(C) >= 2\n"
            "            X, t, thr = codec.encode(x, 0.4)\n"
            "            ts = codec.psy.tonality(X)\n"
            "            thrs = codec.psy.global_masking_threshold(X, ts, 0.4)\n"
            "            for k, v in (('X', X), ('t', t), ('thr', thr), ('ts', ts), ('thrs', thrs)):\n"
            "                out['%%s_%%d_%%d_%%d' %% (k, round(alpha * 10), N, C)] = v.cpu().numpy()\n"
            "np.savez(sys.argv[1], **out)\n" % (ALPHAS, sizes, chans))
    f = str(tmp_path / "walk_alpha.npz")
    r = subprocess.run([sys.executable, "-c", code, f], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, AC_NO_RUNS="1", AC_LDS_WAVE_NOFUSE="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(f)
    for alpha in ALPHAS:
        for N in sizes:
            for C in chans:
                X, t, thr, ts, thrs = (got["%s_%d_%d_%d" % (k, round(alpha * 10), N, C)]
                                       for k in ("X", "t", "thr", "ts", "thrs"))
                model = (48000, N, 64)
                X64 = X.astype(np.float64)
                t64 = _oracle(*model, alpha).tonality(X64)
                assert tonality_err(t, t64) <= 1.0 and tonality_err(ts, t64) <= 1.0, (alpha, N, C)
                _hold(thr, X64, t64, 0.4, model, alpha, TOL, "band walk")
                _hold(thrs, X64, ts.astype(np.float64), 0.4, model, alpha, TOL, "band walk")


# ---- the fused encode of the LDS-FFT tier and below 1024 ---------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("N", [960, 2160, 512, 128])
def test_fused_encode_beside_1024_at_other_alpha(N, alpha, monkeypatch):
    """The run-structured model (ac_psy_runs_dev.h:422-453, runs_params) inside the one-launch encodes: k_enc_wave_v of the
    LDS-FFT tier at filters_n 960 and 2160 (forced on with AC_LDS_WAVE_NOFUSE=2, read per call) and k_fwd_multi at 512 and
    128, mono and stereo: bit for bit the un-fused calls (one definition of the arithmetic), and the oracle at the bar."""
    assert (N in ENC_SIZES) == (N in (960, 2160))
    for C in (1, 2):
        codec = audiocodec_amd.AudioCodec(48000, N, alpha=alpha)
        assert codec.psy.tier() == 1
        x = _pcm(N + C, 3 if C == 1 else 2, 4, N, C)
        if N in ENC_SIZES:
            monkeypatch.setenv("AC_LDS_WAVE_NOFUSE", "2")
        assert codec.encode_launches(C) == 1
        X, t, thr = codec.encode(x, 0.4)
        if N in ENC_SIZES:
            monkeypatch.setenv("AC_LDS_WAVE_NOFUSE", "1")
            assert codec.encode_launches(C) == 2
        Xu = codec.mdct.transform(x)
        tu = codec.psy.tonality(Xu)
        thru = codec.psy.global_masking_threshold(Xu, tu, 0.4)
        monkeypatch.delenv("AC_LDS_WAVE_NOFUSE", raising=False)
        assert torch.equal(X, Xu) and torch.equal(t, tu) and torch.equal(thr, thru)
        _hold_encode(X, t, thr, 0.4, (48000, N, 64), alpha, TOL, "fused encode beside 1024")


# ---- the generic kernels (ac_psy_generic.hip) ---------------------------------------------------------------------------------
GENERIC = [(48000, 1024, 64, torch.float32), (48000, 30, 8, torch.float32), (48000, 1024, 128, torch.float32),
           (48000, 2048, 64, torch.float64), (48000, 960, 64, torch.bfloat16), (48000, 1024, 64, torch.bfloat16)]


def _generic_id(sr, N, M, dt, *rest):
    return "-".join([str(dt).split(".")[-1], "N%d" % N, "M%d" % M] + ["%s" % (r,) for r in rest])


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("case", range(len(GENERIC)), ids=[_generic_id(*c) for c in GENERIC])
def test_generic_forward_at_other_alpha(case, alpha):
    """k_threshold_generic (ac_psy_generic.hip: m_pow(max(eps, P), alpha), 10^(-alpha O / 10), (fac A)^(1/alpha)) with
    ac_set_force_generic(1), in each instance of its one launcher (launch_threshold_T): float32 at 64 bands, at a small layout
    (30 filters, 8 bands) and at 128 bands; float64; bfloat16 tensors with float32 arithmetic.  (The backward has a launcher
    of its own, launch_threshold_bwd_T: below.)"""
    sr, N, M, dt = GENERIC[case]
    p = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M, alpha=alpha, compute_dtype=dt)
    X = torch.from_numpy(_spectrum(N + M, 2, 3, N, 3)).cuda().to(dt)
    X64 = _np64(X)
    to = _oracle(sr, N, M, alpha).tonality(X64)
    path = "generic " + str(dt).split(".")[-1]
    with _forced_generic():
        t = p.tonality(X)
        thrs = [(drown, p.global_masking_threshold(X, t, drown)) for drown in (0.0, 0.4, 1.0)]
    if dt == torch.float32:
        assert tonality_err(t, to) <= 1.0
        bar = TOL
    elif dt == torch.float64:
        assert float(np.abs(_np64(t) - to).max()) <= 1e-12
        bar = 1e-10
    else:
        assert float(np.abs(_np64(t) - to).max()) <= 4e-3
        bar = 6e-3
    for drown, thr in thrs:
        assert thr.dtype == dt
        _hold(thr, X64, _np64(t), drown, (sr, N, M), alpha, bar, path)


# ---- two models alive at once ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [(0.3, 0.8), (0.8, 0.3)], ids=["0.3-then-0.8", "0.8-then-0.3"])
@pytest.mark.parametrize("N,spreading", [(1024, "bf16x2_mfma"), (1024, "bf16_mfma"), (960, None)])
def test_two_models_of_different_alpha_alive_at_once(N, spreading, order):
    """Two plans of the same (sample rate, filter_bands_n, bands) and different alpha, built one after the other and called
    interleaved, each twice, each held to its own oracle: a device table cached without alpha in its key -- the bfloat16 /
    split-bfloat16 image of the spreading matrix at 1024, the run image at 960 -- would serve one of them the other's."""
    dev = torch.device("cuda", torch.cuda.current_device())
    models = []
    for a in order:
        p = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=N, alpha=a, spreading=spreading)
        p._plan(dev)                                          # (plans are built on first use: build them in this order)
        assert spreading is None or p.plan_spreading() == spreading
        models.append((p, a))
    X = torch.from_numpy(_spectrum(N, 2, 3, N, 2)).cuda()
    for rep in range(2):
        for p, a in models:
            _hold_model(p, X, (48000, N, 64), a, _form_bar(spreading, a), "two models " + str(spreading), (0.4,))
        models.reverse()


# ---- backward -----------------------------------------------------------------------------------------------------------------
def _bars(alpha):
    return {k: (v[0] * _amp(alpha), v[1] * _amp(alpha)) for k, v in checks.BARS.items()}


FAST_BWD = [(1024, (3, 3, 3)), (2048, (2, 3, 2)), (2048, (1, 3, 1))]


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("case", range(len(FAST_BWD)), ids=["N%d-B%dF%dC%d" % (n, *s) for n, s in FAST_BWD])
def test_fast_backward_at_other_alpha(case, alpha):
    """k_psy_bwd_fast (ac_fast_psy_bwd.hip:182-232: Q, fac and T recomputed with alpha and 1 / alpha, then gY = gT T /
    (alpha Y), the -alpha ln(10) / 10 of d fac / d t, gP = gQ alpha Q / P) in its three channel modes and both row widths,
    against torch.autograd on the float64 restatement, which reads the model's alpha: the composed chain, the threshold
    alone (grad_X, grad_t) and the tonality alone at drown 0.4 -- and once, at alpha 0.8, at drown 1 where grad_t is exactly
    0 -- with the guards of test_psy_backward.py (drown + 0.05, one column of S zeroed)."""
    N, (B, F, C) = FAST_BWD[case]
    p = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=N, bark_bands_n=64, alpha=alpha)
    assert p.is_fast() and p.alpha == alpha
    g = torch.Generator(device="cuda").manual_seed(300 + case)
    X = checks.draw(B, F, N, C, g, torch.float32)
    worst = WORST_BWD.setdefault(alpha, {})
    wrong = (audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=N, bark_bands_n=64, alpha=alpha * 1.02),)
    checks.check_backward(p, X, 0.4, "fast", g, _bars(alpha), worst, wrong_models=wrong)
    if case == 0 and alpha == 0.8:
        checks.check_backward(p, X, 1.0, "fast", g, _bars(alpha), worst, wrong_models=wrong)


GENERIC_BWD = [(48000, 960, 64, 2, 3, 3, torch.float32), (48000, 120, 20, 2, 3, 7, torch.float32),
               (48000, 1024, 128, 1, 3, 1, torch.float32), (48000, 2048, 64, 2, 3, 1, torch.float64),
               (48000, 960, 64, 2, 3, 3, torch.bfloat16)]


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("case", range(len(GENERIC_BWD)),
                         ids=[_generic_id(c[0], c[1], c[2], c[6], "B%dF%dC%d" % c[3:6]) for c in GENERIC_BWD])
def test_generic_backward_at_other_alpha(case, alpha):
    """k_threshold_bwd_generic (ac_psy_generic.hip, launched by launch_threshold_bwd_T with (TC) alpha) in float32 -- at 960 filters, at
    a small layout of 20 bands with seven channels, and at 128 bands -- in float64 and on bfloat16 tensors: the scheme of
    test_fast_backward_at_other_alpha, drown 1 once per dtype at alpha 0.8."""
    sr, N, M, B, F, C, dt = GENERIC_BWD[case]
    p = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M, alpha=alpha, compute_dtype=dt)
    assert not p.is_fast() or dt != torch.float32
    g = torch.Generator(device="cuda").manual_seed(400 + case)
    X = checks.draw(B, F, N, C, g, dt)
    if dt == torch.bfloat16:
        # the bfloat16 bar (1.2e-2, 6.7e-3) is as wide as what one of 64 columns of S moves in the gradient of a broadband
        # frame (measured on the reference alone: 4e-3 ... 1.1e-2), so the column guard needs a frame whose energy sits in a
        # few bands -- and the alpha guard one whose energy sits in more than one.  An eighth of the bins raised by 100:
        # on the reference alone the drown, column and alpha * 1.02 guards then move the gradient by at least 3.9, 3.1 and
        # 2.6 times the bar (a sixteenth leaves the alpha guard 1.2 times, the broadband frame fails the column guard)
        X = X.double()
        X[:, :, N // 2: N // 2 + N // 8] *= 100.0
        X = X.to(dt)
    path = {torch.float32: "generic", torch.float64: "float64", torch.bfloat16: "bfloat16"}[dt]
    worst = WORST_BWD.setdefault(alpha, {})
    rounded = dt == torch.bfloat16
    wrong = (audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M, alpha=alpha * 1.02, compute_dtype=dt),)
    checks.check_backward(p, X, 0.4, path, g, _bars(alpha), worst, rounded_t=rounded, wrong_models=wrong)
    if case in (0, 3, 4) and alpha == 0.8:
        checks.check_backward(p, X, 1.0, path, g, _bars(alpha), worst, rounded_t=rounded, wrong_models=wrong)
