"""GPU (MI355X): three kinds of output held to exact definitions, element by element.

A. The int16 PCM stores (to_pcm16, ac_internal.h):
   pcm = 0 if x is NaN else clamp(rint(fp32(32768 x)), -32768, 32767), rint = round half to even; +-Inf and products that
   overflow float32 go to the rail of their sign.  Every store family decodes spectra that overshoot full scale (per-clip
   gains 1, 1.5 and 1e36 / 32768, one frame with a NaN coefficient): the expectation is that formula, in numpy, on the
   library's own float32 decode of the same spectra -- exact equality, since the float32 and the 16-bit instances of a
   kernel compute the same float32 sample -- and that float32 decode is held to the float64 oracle (rel_peak <= 1e-4) on
   its finite frames.  Exact .5 ties of 32768 x cannot be produced through a transform: they are not tested here.
   The shares of samples on the rails are counted over a clip's interior [N, -N): the first and the last block of a decode
   are the filter bank's fade-in and fade-out, N samples each whatever the clip's length.

B. The bfloat16 and float16 stores round to nearest even.  Every 2-byte result y against the float64 oracle value t on the
   very 2-byte inputs the kernel read:   |y - t| <= 0.5 ulp2(t) + s scale,
   ulp2(t) = 2^(max(floor(log2 |t|), emin) - p)  (bfloat16 p = 7, emin = -126; float16 p = 10, emin = -14), scale the
   frame's peak |t| for the analysis, |t| itself for tonality, thresholds and dB, and for the synthesis the largest peak
   |t| of the block and the two blocks beside it (_block_scale: a block is the overlap-add of two frames that reach over
   those three blocks, and may itself cancel to nothing -- the first block of a round trip peaks at 1e-14 -- while the
   float32 error of the two frames does not).  The slack s is 4 times the worst error of the float32 kernels in the same
   call, at the same shape, on the same inputs (4: instantiations contract multiply-adds differently); it must stay
   <= 2^-13 for the bar to tell rounding from truncation.
   Over the n distinct values above an eighth of that peak the mean of sign(t) (y - t) / ulp2(t) lies within
   +-max(0.05, 5.5 / sqrt(12 n)), in every case (truncation gives -0.5).  Distinct: a threshold repeats over the bins of
   its band, one rounding error however many bins.  The mean of n rounding errors has deviation 1 / sqrt(12 n), so 0.05 is
   5.5 deviations from n = 1008 on and would fail a correct store below that; at fewer values the bar is those 5.5
   deviations, which still excludes -0.5 down to n = 30 (0.29), the least a case may have.  Every comparison also shows
   that its bar bites: the oracle values truncated toward zero to the 2-byte type fall outside it.

C. The noise generator against tests/noise_reference.py (float64; test_noise_reference.py holds that restatement to a
   standard normal): 6 add_noise(0, 1, seed) equals it within NOISE_BAR, the error of v_log_f32 / v_sqrt_f32 / v_cos_f32 /
   v_sin_f32, through the 16-byte body and the scalar tail of k_add_noise, the fused epilogue of encode_ex, and the float64
   and bfloat16 streams; a negative seed and its 64-bit image give one stream.

Measured on the MI355X (the worst float32-kernel-to-oracle error over the calls of this module; the constant is 4 times it):
  * filter bank: analysis 2.68e-7 of the frame's peak, synthesis 3.43e-7 of the block scale -> S_FB 1.4e-6; tonality,
    rel_elem 1.062e-6 -> S_TON 4.3e-6; thresholds, rel_elem 5.50e-6 -> S_THR 2.2e-5; amplitude_to_dB, rel_elem 3.82e-7 ->
    S_DB 1.6e-6: each below 2^-13 = 1.22e-4.  With them the 2-byte results use at most 1.8e-7 of their scale beyond half
    an ulp.
  * mean signed errors, in ulp, by the number n of distinct values: the filter bank at 1024 / 2048 / 960 and the fused X
    (n = 23 000 ... 28 500) within 0.0035, at 256 / 250 (3 100 ... 3 400) within 0.0082, at 12 (470 ... 530, bar 0.069
    ... 0.073) within 0.024; amplitude_to_dB (1 643) 0.0056; thresholds -0.004 (814, bar 0.056), -0.018 (370, bar 0.083), +0.023
    (74, bar 0.18), -0.148 (67, bar 0.19: the largest share of a bar, 0.77); tonality (36 ... 54 values, bars 0.22 ... 0.26) within 0.07.
  * generator: 7.52e-7 over the four seeds, body and tail -> NOISE_BAR 3.1e-6 (condition: <= 1e-4); the fused epilogue
    uses 0.16 of its bar.
  * 16-bit stores: the float32 decode the expectation is computed from is within 3.7e-7 of the oracle; in the synthesis
    from codes 11.6 % of the loud clip's interior sits on each rail (8.3 % of the whole decode); elsewhere it is the sixth
    that uniform PCM times 1.5 gives.
No store was found wrong; NaN -> 0 is the one change of behaviour (it stored -32768).

That the module bites (scratch builds of the library, this module run once against each, 39 cases):
  * Bf16Fmt::enc2 and both pk_bf16 truncating: 5 fail -- the bfloat16 filter bank at 1024 and 2048 (18 168 of 36 864
    elements outside the bar), the wave-level and the run-structured masking model (tonality: 21 of 36 outside), the fused
    encode; the LDS-FFT, generic and float16 cases pass, as they should: their stores are other sites.
  * to_pcm16 without its upper clamp: the 9 cases of part A fail, nothing else.
  * g0 and g1 swapped in normal_pair: the 7 cases of part C fail (worst difference 7.5), nothing else.
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_elem, rel_peak
import noise_reference as nr

import audiocodec_amd
from audiocodec_amd import _lib
from oracle.audiocodec_oracle import MDCTOracle, PsychoOracle

pytestmark = pytest.mark.gpu

TOL = 1e-4               # the forward parity bar of test_gpu_parity.py
S_MAX = 2.0 ** -13       # the most slack that still tells rounding from truncation
S_FB = 1.4e-6            # filter bank, of the frame's peak / the block scale (4 x 3.43e-7)
S_TON = 4.3e-6           # tonality, of |t| (4 x 1.062e-6)
S_THR = 2.2e-5           # thresholds, of |t| (4 x 5.50e-6)
S_DB = 1.6e-6            # amplitude_to_dB, of |t| (4 x 3.82e-7)
NOISE_BAR = 3.1e-6       # |6 add_noise(0, 1) - restatement| (4 x 7.52e-7); must stay <= 1e-4
WORST = {}               # quantity -> worst figure seen in this run (printed at the end)
BIAS = {}                # quantity -> [(distinct values, mean signed error in ulp)] of its cases

FORMATS = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X (run with -m gpu on the GPU box)"
    assert _lib.load().ac_set_force_generic(0) == 0, "AC_TESTING=1 not in effect"
    yield
    _lib.load().ac_set_force_generic(0)
    if WORST:
        print("\nworst figures of test_value_contracts.py:")
        for k in sorted(WORST):
            print("  %-46s %.3e" % (k, WORST[k]))
        for k in sorted(BIAS):
            print("  bias of %-38s %s" % (k, "  ".join("%d: %+.4f" % nm for nm in BIAS[k])))


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def np64(t):
    return t.detach().double().cpu().numpy()


# ---- A. int16 PCM stores ------------------------------------------------------------------------------------------
GAINS = (1.0, 1.5, 1e36 / 32768.0)
NAN_FRAME = 2


def _pcm(N, C, K):
    """Uniform full-scale int16 PCM of three clips (an odd signal count for the mono kernels)."""
    g = torch.Generator(device="cuda").manual_seed(7 * N + C)
    return torch.randint(-32768, 32768, (3, K * N, C), device="cuda", dtype=torch.int16, generator=g)


def _loud_spectra(codec, pcm):
    """X0 = transform(pcm / 32768) and X = gain[b] X0 with one NaN coefficient in channel 0 of frame NAN_FRAME of clip 0."""
    X0 = codec.mdct.transform(pcm.float() / 32768.0)
    X = X0 * torch.tensor(GAINS, dtype=torch.float32, device="cuda").view(3, 1, 1, 1)
    X[0, NAN_FRAME, X.shape[2] // 3, 0] = float("nan")
    return X0, X.contiguous()


def pcm16_of(y):
    """The contract, in numpy, on float32 samples."""
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        p = (y * np.float32(32768.0)).astype(np.float32)
        r = np.clip(np.rint(p), -32768.0, 32767.0)
    return np.where(np.isnan(p), 0.0, r).astype(np.int16)


def _check_pcm16(N, y, out, X_oracle, loud_clip, huge_clip):
    """y: the library's float32 decode [3, S, C]; out: its 16-bit decode; X_oracle: float64 spectra for the oracle -- the
    spectra decoded, except that the huge clip is there without its gain and the poisoned values are finite."""
    y, out = np.asarray(y), np.asarray(out)
    B, S, C = y.shape
    exp = pcm16_of(y)
    yo = MDCTOracle(N, "vorbis", np.float64).inverse_transform(X_oracle)
    # the expectation's float32 samples against the oracle: finite frames, clips with gain <= 1.5
    bad = ~np.isfinite(y)
    where_bad = np.zeros_like(bad)
    where_bad[0, NAN_FRAME * N:(NAN_FRAME + 2) * N, 0] = True      # (the other channel is finite and held to the oracle)
    assert not np.any(bad & ~where_bad) and np.all(bad[0, NAN_FRAME * N:(NAN_FRAME + 2) * N, 0])
    small = [b for b in range(B) if b != huge_clip]
    e = rel_peak(np.where(bad, 0.0, y)[small, None], np.where(bad, 0.0, yo)[small, None])   # (a signal = one "frame")
    _note("pcm16: float32 decode vs oracle (rel_peak)", e)
    assert e <= TOL
    # the conditions that keep the comparison from being vacuous
    loud = exp[loud_clip, N:-N]      # (the clip itself: the first and the last block are the bank's fade-in and fade-out)
    hi, lo = float(np.mean(loud == 32767)), float(np.mean(loud == -32768))
    assert hi >= 0.10 and lo >= 0.10 and 1.0 - hi - lo >= 0.30, (hi, lo)
    inner, ref = exp[huge_clip, N:-N], yo[huge_clip, N:-N]          # (the oracle of the clip before its gain)
    sel = np.abs(ref) > 2.0 / 32768.0
    assert sel.mean() >= 0.9
    assert np.array_equal(inner[sel], np.where(ref[sel] > 0, 32767, -32768))
    assert np.all(exp[0, NAN_FRAME * N:(NAN_FRAME + 2) * N, 0] == 0)
    # the stores
    assert out.dtype == np.int16 and np.array_equal(out, exp), "%d samples differ" % int(np.sum(out != exp))


def _oracle_spectra(X0, X):
    Xo = np64(X)
    X0 = np64(X0)
    Xo[2] = X0[2]
    nan = np.isnan(Xo)
    Xo[nan] = X0[nan]
    return Xo


@pytest.mark.parametrize("N,C,K", [(1024, 2, 5), (2048, 1, 5), (512, 2, 21), (64, 1, 21), (960, 2, 37), (120, 1, 37)])
def test_pcm16_stores_clamp_and_silence_nan(N, C, K):
    """The wave-level synthesis (stereo, mono), the several-frames-per-wave kernels with idle lane groups (K = 21) and the
    LDS-FFT tier (K = 37), each on spectra that overshoot both rails, overflow, and hold a NaN frame."""
    codec = audiocodec_amd.AudioCodec(48000, N)
    X0, X = _loud_spectra(codec, _pcm(N, C, K))
    y = codec.decode(X)
    out = codec.decode(X, pcm16=True)
    assert out.dtype == torch.int16 and tuple(out.shape) == (3, (K + 2) * N, C)
    _check_pcm16(N, y.cpu().numpy(), out.cpu().numpy(), _oracle_spectra(X0, X), loud_clip=1, huge_clip=2)


def test_pcm16_stores_of_the_strided_form(tmp_path):
    """Three channels at 1024: 16-bit PCM runs the wave-level kernels' strided form, float32 runs it only with the channel-pair
    instances of the LDS-FFT tier off (AC_LDS_WAVE_NOVEC=1, read once per process), so both decodes come from a child."""
    N, C, K = 1024, 3, 5
    codec = audiocodec_amd.AudioCodec(48000, N)
    X0, X = _loud_spectra(codec, _pcm(N, C, K))
    np.save(str(tmp_path / "X.npy"), X.cpu().numpy())
    code = ("import sys, numpy as np, torch, audiocodec_amd\n"
            "X = torch.from_numpy(np.load(sys.argv[1])).cuda()\n"
            "codec = audiocodec_amd.AudioCodec(48000, %d)\n"
            "assert codec.mdct.tier(%d) == 3\n"
            "np.savez(sys.argv[2], y=codec.decode(X).cpu().numpy(), out=codec.decode(X, pcm16=True).cpu().numpy())\n" % (N, C))
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "X.npy"), str(tmp_path / "out.npz")], cwd=ROOT,
                       env=dict(os.environ, AC_LDS_WAVE_NOVEC="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(str(tmp_path / "out.npz"))
    _check_pcm16(N, got["y"], got["out"], _oracle_spectra(X0, X), loud_clip=1, huge_clip=2)
    assert np.array_equal(codec.decode(X, pcm16=True).cpu().numpy(), got["out"])   # (this process: the same 16-bit kernel)


@pytest.mark.parametrize("N,C", [(1024, 2), (2048, 1)])
def test_pcm16_stores_of_the_synthesis_from_codes(N, C):
    """decode_quantized(..., pcm16=True), the product's output: lossy codes of PCM 1.5 times full scale overshoot as a
    matter of course; clip 2 has its scale factors raised by 80 (a gain of 2^20), and one band of clip 0 is marked
    non-representable (sf = -128: NaN by DESIGN.md section 8a rule 5), which must decode to silence."""
    K = 5
    codec = audiocodec_amd.AudioCodec(48000, N)
    assert codec.decode_quantized_launches(C) == 1
    x = 1.5 * (_pcm(N, C, K).float() / 32768.0)
    codes, sf0 = codec.encode_quantized(x)
    off = codec.psy.scale_band_offsets
    band = int(np.argmax(np.diff(off)))
    sf = sf0.clone()
    assert not bool((sf0 == -128).any())
    sf[2] = torch.clamp(sf0[2].int() + 80, -127, 127).to(torch.int8)
    sf[0, NAN_FRAME, band, 0] = -128
    Xh = codec.psy.dequantize(codes, sf)
    assert int(torch.isnan(Xh).sum()) == int(off[band + 1] - off[band])
    y = codec.decode(Xh)
    out = codec.decode_quantized(codes, sf, pcm16=True)
    assert out.dtype == torch.int16
    _check_pcm16(N, y.cpu().numpy(), out.cpu().numpy(), _oracle_spectra(codec.psy.dequantize(codes, sf0), Xh),
                 loud_clip=1, huge_clip=2)
    assert torch.equal(codec.decode(Xh, pcm16=True), out)


# ---- B. bfloat16 / float16 stores -----------------------------------------------------------------------------------
def ulp2(t, dtype):
    p, emin = FORMATS[dtype]
    _, e = np.frexp(np.abs(t))                      # |t| = m 2^e, m in [0.5, 1): floor(log2 |t|) = e - 1
    return np.ldexp(1.0, np.maximum(e - 1, emin) - p)


def truncated(t, dtype):
    """t rounded toward zero to the 2-byte type (float64 values)."""
    t = np.asarray(t, dtype=np.float64)
    if dtype == torch.bfloat16:
        f = t.astype(np.float32)
        f = np.where(np.abs(f.astype(np.float64)) > np.abs(t), np.nextafter(f, np.float32(0)), f).astype(np.float32)
        return (f.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        h = t.astype(np.float16)
    h = np.where(np.abs(h.astype(np.float64)) > np.abs(t), np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float64)


def _check_rounding(what, y, t, scale, peak, s, dtype):
    """y (the kernel's 2-byte result, as float64) against t: the element bar, its guard, and the bias check."""
    assert s <= S_MAX
    y, t = np.asarray(y, dtype=np.float64), np.asarray(t, dtype=np.float64)
    scale, peak = np.broadcast_to(scale, t.shape), np.broadcast_to(peak, t.shape)
    u = ulp2(t, dtype)
    bar = 0.5 * u + s * scale
    err = np.abs(y - t)
    _note("%s: (|y - t| - ulp2 / 2) / scale" % what, np.max((err - 0.5 * u) / np.maximum(scale, 1e-300)))
    finite, n_out = bool(np.all(np.isfinite(y))), int(np.sum(~(err <= bar)))
    assert finite and n_out == 0, \
        "%s: %d of %d elements outside the bar, worst %.3g ulp" % (what, n_out, t.size, float(np.max(err / u)))
    outside = np.abs(truncated(t, dtype) - t) > bar
    assert outside.mean() >= 0.10 if t.size >= 1000 else outside.any(), "%s: a truncating store would pass" % what
    sel = np.abs(t) > peak / 8.0
    _, first = np.unique(t[sel], return_index=True)          # (a threshold repeats over the bins of its band: one draw)
    n = first.size
    assert n >= 30, "%s: %d distinct values in the bias check" % (what, n)
    m = float(np.mean((np.sign(t[sel]) * (y[sel] - t[sel]) / u[sel])[first]))
    bias_bar = max(0.05, 5.5 / np.sqrt(12.0 * n))            # (0.05 from n = 1008 on; see the module docstring)
    _note("%s: |mean signed error| / its bar" % what, abs(m) / bias_bar)
    BIAS[what] = BIAS.get(what, []) + [(n, m)]
    assert abs(m) <= bias_bar, "%s: mean signed rounding error %.3f ulp over %d values (bar %.3f)" % (what, m, n, bias_bar)


def _frame_peak(t):
    return np.max(np.abs(t), axis=2, keepdims=True)


def _as_blocks(a, N):
    B, S, C = a.shape
    return a.reshape(B, S // N, N, C)


def _block_scale(t):
    """The scale of a synthesis result [B, blocks, N, C]: the largest peak |t| of its block and the two beside it.  Block n
    is the overlap-add of frames n - 1 and n, whose samples are blocks n - 1 ... n + 1: the float32 error of block n follows
    their size, not what is left of them in a block that cancels (the first block of a round trip peaks at 1e-14)."""
    p = _frame_peak(t)
    q = np.pad(p, ((0, 0), (1, 1), (0, 0), (0, 0)))
    return np.maximum(p, np.maximum(q[:, :-2], q[:, 2:]))


def _to16(a, dtype):
    """float64 array -> the 2-byte tensor nearest to it (on the host), and the float64 values it holds."""
    t = torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dtype)
    return t, t.double().numpy()


def _filter_bank_case(N, C, dtype, x_scale=1.0, X_scale=None):
    """transform on 2-byte PCM, inverse_transform on the 2-byte spectra it returned (or on uniform spectra times X_scale):
    both against the oracle, with the float32 kernels' error on the same inputs noted."""
    rng = np.random.default_rng(N + C)
    B, K = 3, 5
    m = audiocodec_amd.MDCTransformer(N, compute_dtype=dtype)
    m32 = audiocodec_amd.MDCTransformer(N)
    o = MDCTOracle(N, "vorbis", np.float64)
    x16, x = _to16(rng.uniform(-1, 1, (B, K * N, C)) * x_scale, dtype)
    X = m.transform(x16.cuda())
    assert X.dtype == dtype
    Xo = o.transform(x)
    e32 = rel_peak(np64(m32.transform(dev(x.astype(np.float32)))), Xo)
    if X_scale is None:
        X16, Xv = X.cpu(), np64(X)
    else:
        X16, Xv = _to16(rng.uniform(-1, 1, (B, K + 1, N, C)) * X_scale, dtype)
    y = m.inverse_transform(X16.cuda())
    assert y.dtype == dtype
    yo = _as_blocks(o.inverse_transform(Xv), N)
    y32 = _as_blocks(np64(m32.inverse_transform(dev(Xv.astype(np.float32)))), N)
    e32i = float(np.max(np.abs(y32 - yo) / _block_scale(yo)))
    _note("float32 analysis vs oracle (of the frame's peak)", e32)
    _note("float32 synthesis vs oracle (of the block scale)", e32i)
    assert 4 * max(e32, e32i) <= S_FB
    return (np64(X), Xo, _frame_peak(Xo)), (_as_blocks(np64(y), N), yo, _block_scale(yo))


@pytest.mark.parametrize("N,C", [(1024, 2), (2048, 1), (960, 2), (256, 1), (12, 3), (250, 1)])
def test_bfloat16_filter_bank_rounds_to_nearest(N, C):
    """Bf16Fmt::enc2 of the wave-level kernels (1024, 2048), the stores of the LDS-FFT tier (960, 256), stv of the generic
    kernels (12, 250)."""
    for name, (y, t, pk) in zip(("transform", "inverse"), _filter_bank_case(N, C, torch.bfloat16)):
        _check_rounding("bfloat16 %s" % name, y, t, pk, pk, S_FB, torch.bfloat16)


@pytest.mark.parametrize("N,C", [(1024, 2), (960, 2), (12, 3), (250, 1)])
def test_float16_filter_bank_rounds_to_nearest(N, C):
    for name, (y, t, pk) in zip(("transform", "inverse"), _filter_bank_case(N, C, torch.float16)):
        _check_rounding("float16 %s" % name, y, t, pk, pk, S_FB, torch.float16)


def _unit_peaks(N, C):
    """The oracle's peak output for the unit-scale inputs of _filter_bank_case (analysis of uniform PCM, synthesis of uniform
    spectra): what the input scales of the subnormal and overflow cases are chosen from."""
    rng = np.random.default_rng(N + C)
    o = MDCTOracle(N, "vorbis", np.float64)
    a = np.abs(o.transform(rng.uniform(-1, 1, (3, 5 * N, C)))).max()
    b = np.abs(o.inverse_transform(rng.uniform(-1, 1, (3, 6, N, C))))
    return float(a), b


@pytest.mark.parametrize("N,C", [(1024, 2), (960, 2), (12, 3), (250, 1)])
def test_float16_subnormal_results_are_not_flushed(N, C):
    """Inputs scaled (by a power of two, then rounded to float16) so that the results peak near 1e-4 and most lie below
    2^-14, the smallest normal float16: the same bar, with ulp2 = 2^-24 there; a flushed result misses it by orders of
    magnitude."""
    a, b = _unit_peaks(N, C)
    xs, Xs = 2.0 ** np.floor(np.log2(1e-4 / a)), 2.0 ** np.floor(np.log2(1e-4 / b.max()))
    for name, (y, t, pk) in zip(("transform", "inverse"), _filter_bank_case(N, C, torch.float16, xs, Xs)):
        at = np.abs(t)
        assert at.max() <= 2e-4 and np.mean(at < 2.0 ** -14) >= 0.25 and np.mean((at > 1e-7) & (at < 2.0 ** -14)) >= 0.25
        assert np.mean((np.abs(y) > 0) & (np.abs(y) < 2.0 ** -14)) >= 0.25      # (subnormal results are there)
        _check_rounding("float16 subnormal %s" % name, y, t, pk, pk, S_FB, torch.float16)


@pytest.mark.parametrize("N,C", [(1024, 2), (960, 2), (12, 3), (250, 1)])
def test_float16_overflow_goes_to_infinity_of_the_right_sign(N, C):
    """The synthesis of float16 spectra scaled so that a share of the samples exceeds 65520, the midpoint between the largest
    float16 and 2^16: those are +-Inf with the oracle's sign, the others finite and inside the bar.  (An element within the
    slack above 65520 may also be the largest finite value: it then meets the bar, which is asserted.  The analysis cannot
    overflow: |X| <= peak |x| / sqrt(2).)"""
    dtype = torch.float16
    _, b = _unit_peaks(N, C)
    Xs = 2.0 ** np.ceil(np.log2(65520.0 / np.quantile(b, 0.92)))
    rng = np.random.default_rng(N + C)
    X16, Xv = _to16(rng.uniform(-1, 1, (3, 6, N, C)) * Xs, dtype)
    assert np.all(np.isfinite(Xv))
    m = audiocodec_amd.MDCTransformer(N, compute_dtype=dtype)
    y = _as_blocks(np64(m.inverse_transform(X16.cuda())), N)
    t = _as_blocks(MDCTOracle(N, "vorbis", np.float64).inverse_transform(Xv), N)
    y32 = _as_blocks(np64(audiocodec_amd.MDCTransformer(N).inverse_transform(dev(Xv.astype(np.float32)))), N)
    slack = S_FB * np.broadcast_to(_block_scale(t), t.shape)
    e32 = float(np.max(np.abs(y32 - t) / _block_scale(t)))
    _note("float32 synthesis vs oracle (of the block scale)", e32)
    assert 4 * e32 <= S_FB
    at, u = np.abs(t), ulp2(t, dtype)
    bar = 0.5 * u + slack
    over = at > 65520.0
    assert 0.01 <= over.mean() <= 0.50, over.mean()
    inside = np.abs(y - t) <= bar
    is_inf = np.isinf(y) & (np.sign(y) == np.sign(t))
    assert np.all(is_inf[over] | inside[over]) and np.mean(is_inf[over]) >= 0.99
    assert np.all(is_inf[at > 65520.0 + slack])
    below = at < 65504.0 - u
    assert np.all(np.isfinite(y[below])) and np.all(inside[below])
    assert not np.any(np.isnan(y))
    tr = truncated(t, dtype)                         # (truncation never reaches Inf: it fails on every overflowing element)
    assert np.all(np.isfinite(tr[over]))


def _psy_spectrum(seed, B, F, N, C):
    rng = np.random.default_rng(seed)
    env = np.logspace(-4, 0, N).reshape(1, 1, N, 1)
    return rng.uniform(-1, 1, (B, F, N, C)) * env * rng.uniform(1e-2, 1, (B, F, 1, C))


@pytest.mark.parametrize("sr,N,M,C,generic", [(48000, 1024, 64, 2, False), (44100, 256, 48, 3, False), (16000, 512, 32, 2, True)])
def test_bfloat16_masking_model_rounds_to_nearest(sr, N, M, C, generic):
    """tonality and global_masking_threshold on bfloat16 tensors: the wave-level model with the float32 spreading product
    (the plain-bfloat16 product's own 5e-3 must not enter), the run-structured model, and the generic kernels (forced)."""
    dtype = torch.bfloat16
    B, F = 3, 6
    X16, X = _to16(_psy_spectrum(N + M + C, B, F, N, C), dtype)
    spreading = "f32" if (N, M) == (1024, 64) else None
    _lib.load().ac_set_force_generic(1 if generic else 0)
    try:
        p = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M, compute_dtype=dtype, spreading=spreading)
        p32 = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M, spreading=spreading)
        Xd = X16.cuda()
        t = p.tonality(Xd)
        thr = p.global_masking_threshold(Xd, t, 0.1)
        assert t.dtype == dtype and thr.dtype == dtype
        X32 = dev(X.astype(np.float32))
        t32 = p32.tonality(X32)
        thr32 = p32.global_masking_threshold(X32, t.float(), 0.1)
    finally:
        _lib.load().ac_set_force_generic(0)
    o = PsychoOracle(sr, N, M, compute_dtype=np.float64)
    to = o.tonality(X)
    tb = np64(t)
    thro = o.global_masking_threshold(X, tb, 0.1)
    et, ethr = rel_elem(np64(t32), to), rel_elem(np64(thr32), thro)
    _note("float32 tonality vs oracle (rel_elem)", et)
    _note("float32 threshold vs oracle (rel_elem)", ethr)
    assert 4 * et <= S_TON and 4 * ethr <= S_THR
    _check_rounding("bfloat16 tonality", tb, to, np.abs(to), np.abs(to), S_TON, dtype)
    _check_rounding("bfloat16 threshold", np64(thr), thro, np.abs(thro), _frame_peak(thro), S_THR, dtype)
    # the coarse bars this supersedes (test_bfloat16_masking_model)
    assert np.max(np.abs(tb - to)) <= 4e-3 and rel_elem(np64(thr), thro) <= 6e-3


def test_bfloat16_fused_encode_rounds_to_nearest():
    """The fused bfloat16 encode at 1024 stereo (float32 spreading product): X against the oracle on the PCM, tonality and
    thresholds against the oracle on the bfloat16 X and tonality the kernel stored."""
    dtype, N, C, B, K = torch.bfloat16, 1024, 2, 3, 6
    x16, x = _to16(np.random.default_rng(N + C).uniform(-1, 1, (B, K * N, C)), dtype)
    codec = audiocodec_amd.AudioCodec(48000, N, compute_dtype=dtype, spreading="f32")
    codec32 = audiocodec_amd.AudioCodec(48000, N, spreading="f32")
    X, t, thr = codec.encode(x16.cuda(), drown=0.1)
    assert X.dtype == t.dtype == thr.dtype == dtype
    om, op = MDCTOracle(N, "vorbis", np.float64), PsychoOracle(48000, N, 64, compute_dtype=np.float64)
    Xo = om.transform(x)
    Xb, tb = np64(X), np64(t)
    to = op.tonality(Xb)
    thro = op.global_masking_threshold(Xb, tb, 0.1)
    X32, t32, thr32 = codec32.encode(dev(x.astype(np.float32)), drown=0.1)
    X64 = np64(X32)
    t64 = op.tonality(X64)
    e = (rel_peak(X64, Xo), rel_elem(np64(t32), t64), rel_elem(np64(thr32), op.global_masking_threshold(X64, np64(t32), 0.1)))
    _note("float32 analysis vs oracle (of the frame's peak)", e[0])
    _note("float32 tonality vs oracle (rel_elem)", e[1])
    _note("float32 threshold vs oracle (rel_elem)", e[2])
    assert 4 * e[0] <= S_FB and 4 * e[1] <= S_TON and 4 * e[2] <= S_THR
    pk = _frame_peak(Xo)
    _check_rounding("bfloat16 fused encode X", Xb, Xo, pk, pk, S_FB, dtype)
    _check_rounding("bfloat16 fused encode tonality", tb, to, np.abs(to), np.abs(to), S_TON, dtype)
    _check_rounding("bfloat16 fused encode threshold", np64(thr), thro, np.abs(thro), _frame_peak(thro), S_THR, dtype)
    assert rel_peak(Xb, Xo) <= 4e-3 and np.max(np.abs(tb - to)) <= 4e-3 and rel_elem(np64(thr), thro) <= 6e-3


def test_bfloat16_amplitude_to_db_rounds_to_nearest():
    """amplitude_to_dB on bfloat16 amplitudes against 10 log10(max(1e-14, a^2)) + 120 in float64, scale |t|.  Amplitudes
    1e-4 ... 1 (40 ... 120 dB) and the floor (0 and 1e-8: -20 dB): at 1e-6 the formula cancels to 0 dB, where the rounding
    of its float32 multiply-add (120 * 2^-24) is not small against |t| and no bar relative to |t| can hold."""
    dtype = torch.bfloat16
    rng = np.random.default_rng(3)
    a = 10.0 ** rng.uniform(-4, 0, (3, 2, 1024, 1)) * rng.choice([-1.0, 1.0], (3, 2, 1024, 1))
    a[0, 0, :4, 0] = (0.0, 1e-8, -1e-8, 1.0)
    a16, av = _to16(a, dtype)
    p = audiocodec_amd.PsychoacousticModel(48000, compute_dtype=dtype)
    dB = p.amplitude_to_dB(a16.cuda())
    assert dB.dtype == dtype
    ref = 10.0 * np.log10(np.maximum(1e-14, av ** 2)) + 120.0
    e32 = rel_elem(np64(audiocodec_amd.PsychoacousticModel(48000).amplitude_to_dB(dev(av.astype(np.float32)))), ref)
    _note("float32 amplitude_to_dB vs formula (rel_elem)", e32)
    assert 4 * e32 <= S_DB
    assert np.all(np64(dB)[0, 0, :3, 0] == -20.0)
    _check_rounding("bfloat16 amplitude_to_dB", np64(dB), ref, np.abs(ref), np.max(np.abs(ref)), S_DB, dtype)
    assert np.max(np.abs(np64(dB) - ref)) <= 0.5            # the coarse bar this supersedes


# ---- C. the noise generator -----------------------------------------------------------------------------------------
SEEDS = (0, 5, 2 ** 64 - 1, 1234567)
N_NOISE = 1 << 20


@pytest.fixture(scope="module")
def model():
    return audiocodec_amd.PsychoacousticModel(48000, 1024)


@pytest.mark.parametrize("seed", SEEDS)
def test_add_noise_draws_the_restated_stream(model, seed):
    """6 add_noise(0, 1, seed): 2^20 elements through the public call (the 16-byte body of k_add_noise), 2^20 + 3 through the
    flat form the backward pass uses (its scalar tail)."""
    shape = (4, 256, 1024, 1)
    g = 6.0 * np64(model.add_noise(torch.zeros(shape, device="cuda"), torch.ones(shape, device="cuda"), seed=seed)).ravel()
    assert NOISE_BAR <= 1e-4
    ref = nr.normals(seed, N_NOISE)
    e = float(np.max(np.abs(g - ref)))
    _note("6 add_noise(0, 1) vs restatement (abs)", e)
    assert e <= NOISE_BAR
    n = N_NOISE + 3
    tail = 6.0 * np64(model._add_noise(None, torch.ones(n, device="cuda"), seed))
    e = float(np.max(np.abs(tail - nr.normals(seed, n))))
    _note("6 add_noise(0, 1) vs restatement (abs)", e)
    assert e <= NOISE_BAR
    assert np.array_equal(tail[:N_NOISE], g)


def test_add_noise_masks_the_seed_to_64_bits(model):
    shape = (1, 2, 1024, 2)
    z, o = torch.zeros(shape, device="cuda"), torch.ones(shape, device="cuda")
    a, b = model.add_noise(z, o, seed=-1), model.add_noise(z, o, seed=2 ** 64 - 1)
    assert torch.equal(a, b) and not torch.equal(a, model.add_noise(z, o, seed=1))
    assert float(np.max(np.abs(6.0 * np64(a).ravel() - nr.normals(2 ** 64 - 1, a.numel())))) <= NOISE_BAR
    codec = audiocodec_amd.AudioCodec(48000, 1024)
    x = torch.rand(1, 3 * 1024, 2, device="cuda") * 2 - 1
    assert torch.equal(codec.encode_ex(x, noise_seed=-1)[3], codec.encode_ex(x, noise_seed=2 ** 64 - 1)[3])


def test_fused_noisy_epilogue_draws_the_restated_stream():
    """encode_ex(noise_seed) at 1024 stereo, one launch: (noisy - X) / thr * 6 against the restatement.  noisy is one fused
    multiply-add rounded to float32, so the quotient carries 6 * 2^-24 max(|X|, |noisy|) / thr (half an ulp of noisy; twice
    that is allowed, for the subtraction and the rounding of g / 6) on top of the generator's bar."""
    N, C, B, K = 1024, 2, 3, 6
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.empty(B, K * N, C, device="cuda").uniform_(-1, 1, generator=gen)
    codec = audiocodec_amd.AudioCodec(48000, N)
    assert codec.encode_launches(C) == 1
    for seed in (5, 2 ** 64 - 1):
        X, _, thr, noisy, _ = codec.encode_ex(x, drown=0.3, noise_seed=seed)
        X, thr, noisy = np64(X).ravel(), np64(thr).ravel(), np64(noisy).ravel()
        ref = nr.normals(seed, X.size)
        bar = NOISE_BAR + 6.0 * 2.0 ** -23 * np.maximum(np.abs(X), np.abs(noisy)) / thr + 2.0 ** -22 * np.abs(ref)
        assert np.median(bar) <= 1e-3 and np.quantile(bar, 0.99) <= 0.05     # (the bar sees an O(1) error everywhere)
        err = np.abs((noisy - X) / thr * 6.0 - ref)
        _note("fused epilogue vs restatement (units of its bar)", np.max(err / bar))
        assert np.all(err <= bar)


def test_float64_and_bfloat16_noise_streams():
    """compute_dtype float64: X + thr g / 6 in float64 with the float32 g of the same seed; bfloat16: the same in float32,
    stored at the half-ulp bar of part B (slack: the generator's bar times thr / 6, and 2^-22 |t| for the float32
    multiply-add)."""
    N, seed = 1024, 1234567
    rng = np.random.default_rng(9)
    X = _psy_spectrum(9, 3, 4, N, 2)
    thr = np.abs(X) * rng.uniform(0.01, 1.0, X.shape) + 1e-6
    ref = nr.normals(seed, X.size).reshape(X.shape)
    p64 = audiocodec_amd.PsychoacousticModel(48000, N, compute_dtype=torch.float64)
    y = np64(p64.add_noise(dev(X), dev(thr), seed=seed))
    assert np.all(np.abs(y - (X + thr * ref / 6.0)) <= thr * NOISE_BAR / 6.0 + 1e-14 * (np.abs(X) + thr))
    dtype = torch.bfloat16
    X16, Xv = _to16(X, dtype)
    thr16, thrv = _to16(thr, dtype)
    pb = audiocodec_amd.PsychoacousticModel(48000, N, compute_dtype=dtype)
    yb = pb.add_noise(X16.cuda(), thr16.cuda(), seed=seed)
    assert yb.dtype == dtype
    t = Xv + thrv * ref / 6.0
    err, u = np.abs(np64(yb) - t), ulp2(t, dtype)
    bar = 0.5 * u + thrv * NOISE_BAR / 6.0 + 2.0 ** -22 * (np.abs(Xv) + thrv)
    assert np.all(err <= bar)
    assert np.mean(np.abs(truncated(t, dtype) - t) > bar) >= 0.10
    m = float(np.mean(np.sign(t) * (np64(yb) - t) / u))
    _note("bfloat16 add_noise: |mean signed error| (ulp)", abs(m))
    assert abs(m) <= 0.05
