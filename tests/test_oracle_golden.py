"""CPU: pin the oracle (oracle/audiocodec_oracle.py) against the golden vectors generated from the
reference's own source (oracle/gen_golden.py) and against every assertion of the reference's 7 tests."""

import numpy as np
import pytest

from conftest import rel_elem, rel_l2, rel_peak
from oracle.audiocodec_oracle import MDCTOracle, PsychoOracle, fold_coefficients, sine_wav

# the reference multiplies the DCT by a float32-rounded sqrt(2) (mdctransformer.py:347): a 1.7e-8
# relative scale offset between its fp64 evaluation and exact arithmetic
REF_SQRT2_REL = 2e-8

MDCT_CASES = [("mdct_n64_sine", 64, "vorbis"), ("mdct_n256_roundtrip", 256, "vorbis"),
              ("mdct_n1024_rand_vorbis", 1024, "vorbis"), ("mdct_n1024_rand_sine", 1024, "sine"),
              ("mdct_n2048_rand_vorbis", 2048, "vorbis"), ("mdct_n16_rand_vorbis", 16, "vorbis"),
              ("mdct_n16_rand_sine", 16, "sine"), ("mdct_n16_rand_rect", 16, "rect"),
              ("mdct_n12_rand_vorbis", 12, "vorbis"),
              ("mdct_n1024_mono_1s", 1024, "vorbis")]      # BASELINE configs[0]: one 1-s mono 48 kHz clip


@pytest.mark.parametrize("name,N,wt", MDCT_CASES)
@pytest.mark.parametrize("dense", [False, True])
def test_mdct_oracle_fp64_matches_reference(golden, name, N, wt, dense):
    g = golden(name)
    o = MDCTOracle(N, wt, np.float64)
    X = o.transform(g["x"].astype(np.float64), dense=dense)
    assert X.shape == g["X_ref64"].shape
    assert rel_peak(X, g["X_ref64"]) < REF_SQRT2_REL
    if "xhat_ref64" in g:
        xh = o.inverse_transform(g["X_ref64"], dense=dense)
        assert np.max(np.abs(xh - g["xhat_ref64"])) < REF_SQRT2_REL * max(1.0, np.max(np.abs(g["xhat_ref64"])))


@pytest.mark.parametrize("name,N,wt", MDCT_CASES)
def test_mdct_oracle_fp32_within_reference_envelope(golden, name, N, wt):
    g = golden(name)
    o = MDCTOracle(N, wt, np.float32)
    X = o.transform(g["x"])
    assert X.dtype == np.float32
    assert rel_peak(X, g["X_ref64"]) < 2e-6
    assert rel_peak(X, g["X_ref32"]) < 2e-6
    if "xhat_ref64" in g:
        xh = o.inverse_transform(X)
        assert np.max(np.abs(xh - g["xhat_ref64"])) < 3e-6


def test_config0_single_mono_clip_round_trip(golden):
    """BASELINE configs[0] (plumbing, no GPU): x[1, 47104, 1] -> X[1, 47, 1024, 1] -> x^[1, 49152, 1] on the CPU
    restatement; x^[:, 1024:-1024] == x within 1 LSB of int16"""
    g = golden("mdct_n1024_mono_1s")
    x = g["x"]
    assert x.shape == (1, 47104, 1)
    o = MDCTOracle(1024, "vorbis", np.float32)
    X = o.transform(x)
    assert X.shape == (1, 47, 1024, 1)
    xh = o.inverse_transform(X)
    assert xh.shape == (1, 49152, 1)
    assert np.max(np.abs(xh[:, 1024:-1024] - x)) <= 1.0 / 32768.0


def test_known_answer_vector(golden):
    """tests/test_mdctransformer.py:39-54 -- the only real-TensorFlow numbers in the reference."""
    g = golden("mdct_n64_sine")
    x = sine_wav(0.8, 4, sample_rate=64, duration_sec=4.0)
    x = x[:, : 64 * (x.shape[1] // 64)]
    np.testing.assert_array_equal(x, g["x"])
    for dt in (np.float32, np.float64):
        X = MDCTOracle(64, "vorbis", dt).transform(x.astype(dt))
        a = g["known_answer_frame1_first10"]
        assert np.all(X[0, 1, :10, 0] - a < 1e-6)            # the reference's one-sided assertion (:54)
        assert np.max(np.abs(X[0, 1, :10, 0] - a)) < 1e-6    # and two-sided


def test_inverse_identity_like_reference():
    """tests/test_mdctransformer.py:19-37"""
    N = 256
    x = sine_wav(0.8, 880, sample_rate=16000, duration_sec=1.0)
    x = x[:, : N * (x.shape[1] // N)]
    o = MDCTOracle(N)
    xh = o.inverse_transform(o.transform(x))
    assert np.max(np.abs(x - xh[:, N:-N])) < 1e-5


def test_shape_like_reference():
    """tests/test_mdctransformer.py:56-75"""
    x = np.random.default_rng(0).standard_normal((128, 10 * 64, 2)).astype(np.float32)
    assert MDCTOracle(64).transform(x).shape == (128, 11, 64, 2)


def test_ragged_input_raises():
    with pytest.raises(ValueError):
        MDCTOracle(64).transform(np.zeros((1, 100, 1), np.float32))


def test_dense_matrices(golden):
    g = golden("mdct_n8_H")
    o = MDCTOracle(8, "vorbis", np.float64)
    np.testing.assert_allclose(o.dense_H(), g["H"], atol=1e-15)
    np.testing.assert_allclose(o.dense_H_inv(), g["H_inv"], atol=1e-14)


def _dense(idx, val, shape):
    m = np.zeros(shape)
    m[idx[:, 0], idx[:, 1]] = val
    return m


@pytest.mark.parametrize("sr,N,M", [(48000, 1024, 64), (48000, 2048, 64), (32768, 64, 64), (44100, 256, 48)])
def test_psy_tables(golden, sr, N, M):
    g = golden("psy_%d_%d_%d_tables" % (sr, N, M))
    p = PsychoOracle(sr, N, M, compute_dtype=np.float64)
    np.testing.assert_allclose(p.W64, _dense(g["W_idx"], g["W_val"], (N, M)), atol=1e-15)
    np.testing.assert_allclose(p.W_inv64, _dense(g["W_inv_idx"], g["W_inv_val"], (M, N)), atol=1e-15)
    np.testing.assert_allclose(p.spreading64, g["S"], rtol=1e-13)
    np.testing.assert_allclose(p.quiet64.reshape(-1), g["quiet"], rtol=1e-13)
    assert abs(p.max_bark - g["max_bark"]) < 1e-14
    assert float(p._dB_MIN) == float(g["dB_MIN"]) == -20.0


def test_energy_conservation_like_reference():
    """tests/test_psychoacoustic.py:14-30"""
    p = PsychoOracle(32768, 64)
    assert np.sum(np.abs(np.sum(p.W, axis=1) - 1.0)) < 1e-6
    assert np.sum(np.abs(np.sum(p.W_inv, axis=1) - 1.0)) < 1e-6


def test_tonality_like_reference():
    """tests/test_psychoacoustic.py:32-65"""
    N = 64
    m = MDCTOracle(N)
    p = PsychoOracle(N, N)
    X = m.transform(sine_wav(0.8, 4, sample_rate=64, duration_sec=5.0))
    assert p.tonality(X)[0, 1] == 1.0
    x = np.random.default_rng(3).uniform(-1, 1, (10, 10 * N, 2)).astype(np.float32)
    t = p.tonality(m.transform(x))
    assert t.shape == (10, 11, 1, 2)
    assert np.mean(t[0, 1:-1]) < 0.1


@pytest.mark.parametrize("cfg,sr,N,M", [("psy_48000_1024_64_cases", 48000, 1024, 64), ("psy_64_64_64_cases", 64, 64, 64),
                                        ("psy_48000_2048_64_cases", 48000, 2048, 64),
                                        ("psy_44100_1024_64_cases", 44100, 1024, 64),
                                        ("psy_96000_2048_64_cases", 96000, 2048, 64)])
@pytest.mark.parametrize("dt,tag,tol", [(np.float64, "ref64", 1e-13), (np.float32, "ref32", 3e-6)])
def test_psy_cases(golden, cfg, sr, N, M, dt, tag, tol):
    g = golden(cfg)
    p = PsychoOracle(sr, N, M, compute_dtype=dt)
    for key in [k for k in g if k.startswith("X_")]:
        name = key[2:]
        X = g[key].astype(dt)
        t_ref = g["t_%s_%s" % (name, tag)]
        t = p.tonality(X)
        assert np.max(np.abs(t - t_ref)) < max(tol, 1e-6 if dt == np.float32 else 0)
        for k2 in [k for k in g if k.startswith("thr_" + name) and k.endswith(tag)]:
            mid = k2[len("thr_" + name):-len(tag)].strip("_")
            drown = int(mid[1:]) / 10.0 if mid else 0.0
            for dense in (False, True):
                thr = p.global_masking_threshold(X, t_ref.astype(dt), drown, dense=dense)
                assert rel_elem(thr, g[k2]) < tol


@pytest.mark.parametrize("alpha", [0.3, 0.8, 1.0])
@pytest.mark.parametrize("sr,N,M", [(48000, 1024, 64), (44100, 256, 48)])
def test_psy_cases_at_other_alpha(golden, sr, N, M, alpha):
    """The compression exponent of the spreading sum away from its default 0.6 (oracle/gen_golden.py 8: the reference's own
    code at alpha 0.3 / 0.8 / 1.0): the oracle's spreading matrix at the tolerance of test_psy_tables, its tonality and
    thresholds (drown 0 / 0.5, float64 and float32) at the tolerances of test_psy_cases.  Every GPU test of the masking
    model at another alpha (test_psy_alpha.py) compares with this oracle."""
    g = golden("psy_alpha_cases")
    assert list(g["alphas"]) == [0.3, 0.8, 1.0]
    tag0 = "%d_%d_%d_a%02d_" % (sr, N, M, round(alpha * 10))
    p64 = PsychoOracle(sr, N, M, alpha=alpha, compute_dtype=np.float64)
    np.testing.assert_allclose(p64.spreading64, g[tag0 + "S"], rtol=1e-13)
    # (the matrix does depend on alpha: the default model's is elsewhere by far more than the tolerance)
    assert rel_elem(PsychoOracle(sr, N, M, compute_dtype=np.float64).spreading64, g[tag0 + "S"]) > 0.1
    X = g[tag0 + "X"]
    assert X.shape == (1, 2, N, 2) and not X[0, 1, :, 1].any() and np.count_nonzero(X[0, 0, :, 1]) == 1
    for dt, tag, tol in ((np.float64, "ref64", 1e-13), (np.float32, "ref32", 3e-6)):
        p = PsychoOracle(sr, N, M, alpha=alpha, compute_dtype=dt)
        t_ref = g[tag0 + "t_" + tag]
        assert np.max(np.abs(p.tonality(X.astype(dt)) - t_ref)) < max(tol, 1e-6 if dt == np.float32 else 0)
        t = t_ref.astype(dt)
        for drown in (0.0, 0.5):
            ref = g[tag0 + "thr_d%02d_%s" % (int(drown * 10), tag)]
            for dense in (False, True):
                assert rel_elem(p.global_masking_threshold(X.astype(dt), t, drown, dense=dense), ref) < tol
    # a threshold of the default alpha is no neighbour of these
    thr06 = PsychoOracle(sr, N, M, compute_dtype=np.float64).global_masking_threshold(X.astype(np.float64), g[tag0 + "t_ref64"], 0.0)
    assert rel_elem(thr06, g[tag0 + "thr_d00_ref64"]) > 0.05


@pytest.mark.parametrize("N", [960, 512, 128])
def test_codec_cases_beside_the_powers_of_two(golden, N):
    """filters_n = 960 (no power of two) and 512 (bins overlap several Bark bands): transform, round trip, tonality and
    thresholds of the reference's own code (oracle/gen_golden.py 5d) against the oracle"""
    g = golden("codec_48000_%d_64_cases" % N)
    o = MDCTOracle(N, "vorbis", np.float64)
    for dense in (False, True):
        X = o.transform(g["x"].astype(np.float64), dense=dense)
        assert rel_peak(X, g["X_ref64"]) < REF_SQRT2_REL
        xh = o.inverse_transform(g["X_ref64"], dense=dense)
        assert np.max(np.abs(xh - g["xhat_ref64"])) < REF_SQRT2_REL * max(1.0, np.max(np.abs(g["xhat_ref64"])))
    assert rel_peak(MDCTOracle(N, "vorbis", np.float32).transform(g["x"]), g["X_ref64"]) < 1e-5
    for dt, tag, tol in ((np.float64, "ref64", 1e-13), (np.float32, "ref32", 3e-6)):
        p = PsychoOracle(48000, N, 64, compute_dtype=dt)
        for name in ("rand", "envelope"):
            X = g["Xp_" + name].astype(dt)
            t_ref = g["t_%s_%s" % (name, tag)]
            assert np.max(np.abs(p.tonality(X) - t_ref)) < max(tol, 1e-6 if dt == np.float32 else 0)
            for drown in (0.0, 0.5):
                ref = g["thr_%s_d%02d_%s" % (name, int(drown * 10), tag)]
                for dense in (False, True):
                    assert rel_elem(p.global_masking_threshold(X, t_ref.astype(dt), drown, dense=dense), ref) < tol


def test_probe_values_from_survey(golden):
    """SURVEY.md 8(c) fixture 5: all-zero and single-bin-delta spectra at 48 kHz / 1024 / 64."""
    p = PsychoOracle(48000, 1024, 64)
    Xz = np.zeros((1, 1, 1024, 1), np.float32)
    t = p.tonality(Xz)
    thr = p.global_masking_threshold(Xz, t)
    assert abs(float(t.reshape(-1)[0])) < 2e-6
    assert abs(thr.min() - 1.78e-7) < 1e-9 and abs(thr.max() - 0.134587) < 1e-6
    Xd = np.zeros((1, 1, 1024, 1), np.float32)
    Xd[0, 0, 100, 0] = 0.5
    t = p.tonality(Xd)
    assert float(t.reshape(-1)[0]) == 1.0
    assert abs(p.global_masking_threshold(Xd, t)[0, 0, 100, 0] - 0.00807218) < 1e-7
    assert abs(p.global_masking_threshold(Xd, t, drown=1.0)[0, 0, 100, 0] - 0.181141) < 1e-5


def test_db_utils(golden):
    g = golden("db_utils")
    p = PsychoOracle(48000)
    np.testing.assert_allclose(p.amplitude_to_dB(g["a"]), g["dB_ref32"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(p.amplitude_to_dB_norm(g["a"]), g["dBn_ref32"], rtol=0, atol=1e-6)
    assert p.amplitude_to_dB(np.float32(0.0)) == -20.0 and p.amplitude_to_dB(np.float32(1.0)) == 120.0


# ---- precompute_dtype = float32 (mdctransformer.py:13-14,31-35,58-59; psychoacoustic.py:14-15,61-69) -------------------
def _dense_from_triplets(idx, val, shape):
    m = np.zeros(shape, dtype=val.dtype)
    m[idx[:, 0], idx[:, 1]] = val
    return m


def test_known_answer_vector_with_float32_precompute(golden):
    """The reference's one TensorFlow-generated vector (tests/test_mdctransformer.py:51-52) stems from a revision that
    pre-computed the window in float32: evaluated that way -- the reference's own source with precompute_dtype=tf.float32
    (fixture X_ref32pre) and the oracle's restatement of it -- it is met to 1e-7 TWO-SIDED (measured 1.1e-8 / 4.5e-8),
    where the float64-precompute default only reaches 6e-7.  This is the tightest statement the reference's tests allow
    about real-TensorFlow numbers."""
    g, g1 = golden("precompute_float32_cases"), golden("mdct_n64_sine")
    a = g1["known_answer_frame1_first10"]
    np.testing.assert_array_equal(g["n64_x"], g1["x"])
    assert np.max(np.abs(g["n64_X_ref32pre"][0, 1, :10, 0] - a)) <= 1e-7          # reference source, float32 precompute
    assert np.max(np.abs(g1["X_ref32"][0, 1, :10, 0] - a)) > 3e-7                  # (the float64-precompute default is not that close)
    for dt in (np.float32, np.float64):
        o = MDCTOracle(64, "vorbis", dt, precompute_dtype=np.float32)
        for dense in (False, True):
            X = o.transform(g["n64_x"].astype(dt), dense=dense)
            assert np.max(np.abs(X[0, 1, :10, 0] - a)) <= 1e-7, (dt, dense)
            assert np.max(np.abs(X - g["n64_X_ref32pre"])) <= 1e-7


def test_float32_precompute_reproduces_the_cancellation(golden):
    """(1 - w[N+j] w[N-1-j]) / w[j] (mdctransformer.py:218-221) in float32 is exactly 0 for j = 0 at N = 64;
    the oracle's float32 tables equal the reference's dense H / H_inv bit for bit (same numpy arithmetic)."""
    g = golden("precompute_float32_cases")
    c = fold_coefficients(64, "vorbis", np.float32)
    assert c["a2"].dtype == np.float32 and c["a2"][0] == 0.0 and c["w"][0] > 2e-4
    assert abs(fold_coefficients(64, "vorbis")["a2"][0] + c["w"][0]) < 1e-7          # float64: -w[0], as the identity says
    o = MDCTOracle(64, "vorbis", np.float32, precompute_dtype=np.float32)
    np.testing.assert_array_equal(o.dense_H().astype(np.float32), g["n64_H"])
    np.testing.assert_allclose(o.dense_H_inv().astype(np.float32), g["n64_H_inv"], rtol=0, atol=2e-7)
    for wt in ("sine", "rect"):
        o = MDCTOracle(16, wt, np.float32, precompute_dtype=np.float32)
        np.testing.assert_array_equal(o.dense_H().astype(np.float32), g["n16_%s_H" % wt])
        np.testing.assert_allclose(o.dense_H_inv().astype(np.float32), g["n16_%s_H_inv" % wt], rtol=0, atol=2e-7)
    o = MDCTOracle(256, "vorbis", np.float32, precompute_dtype=np.float32)
    X = o.transform(g["n256_x"])
    assert np.max(np.abs(X - g["n256_X_ref32pre"])) <= 2e-7
    assert np.max(np.abs(o.inverse_transform(X) - g["n256_xhat_ref32pre"])) <= 2e-6


@pytest.mark.parametrize("sr,N,M", [(48000, 1024, 64), (32768, 64, 64)])
def test_psy_tables_with_float32_precompute(golden, sr, N, M):
    """The masking model's constants in float32 arithmetic: the oracle (numpy, the reference's op order) equals the
    reference's own float32-precompute tables; they sit up to 4e-4 (W) away from the float64-precompute ones -- the
    float32 Bark mapping is that coarse (band edges near 24 kHz carry 2e-3 Hz of rounding against 23 Hz bins)."""
    g = golden("precompute_float32_cases")
    tag = "psy_%d_%d_%d_" % (sr, N, M)
    p = PsychoOracle(sr, N, M, compute_dtype=np.float32, precompute_dtype=np.float32)
    np.testing.assert_array_equal(p.W, _dense_from_triplets(g[tag + "W_idx"], g[tag + "W_val"], (N, M)))
    np.testing.assert_array_equal(p.W_inv, _dense_from_triplets(g[tag + "W_inv_idx"], g[tag + "W_inv_val"], (M, N)))
    np.testing.assert_allclose(p.spreading_matrix, g[tag + "S"], rtol=1e-6)
    np.testing.assert_allclose(p.quiet_threshold_intensity.reshape(-1), g[tag + "quiet"], rtol=1e-6)
    assert p.max_bark.dtype == np.float32 and float(p.max_bark) == float(g[tag + "max_bark"])
    p64 = PsychoOracle(sr, N, M, compute_dtype=np.float32)
    assert 0 < np.max(np.abs(p64.W - p.W)) < 1e-3
    if N == 1024:
        t = p.tonality(g["psy_X_rand"])
        np.testing.assert_allclose(t, g["psy_t_rand"], rtol=1e-5, atol=1e-7)
        for key, drown in (("psy_thr_rand_d00", 0.0), ("psy_thr_rand_d05", 0.5)):
            thr = p.global_masking_threshold(g["psy_X_rand"], t, drown)
            assert rel_elem(thr, g[key]) <= 1e-5
