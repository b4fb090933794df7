"""The perceptual quantiser: int16 codes + int8 per-band scale factors, and the synthesis from codes.

The file holds its own numpy restatement of the definition (rules 1-5 of the section), in float32 with np.rint; the GPU
kernels are checked against it bit for bit, and the fused synthesis from codes against dequantize + decode bit for bit.
"""

import ctypes
import math

import numpy as np
import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib

SQRT3 = np.float32(math.sqrt(3.0))
C4 = np.array([2.0 ** (r / 4) for r in range(4)], dtype=np.float32)
IC4 = np.array([2.0 ** (-r / 4) for r in range(4)], dtype=np.float32)
S_ALL = np.arange(-127, 128, dtype=np.int32)


# ---- numpy restatement ---------------------------------------------------------------------------------------------
def np_offsets(sr, N, M):
    """Rule 1: bin i -> band min(M-1, floor(bark(f_i) / w)), in float64 (libm asinh, bin by bin)."""
    w = 6.0 * math.asinh(sr / 2.0 / 600.0) / M
    band = np.array([min(M - 1, int(math.floor(6.0 * math.asinh(((i + 0.5) * (sr / 2.0) / N) / 600.0) / w)))
                     for i in range(N)], dtype=np.int64)
    return np.searchsorted(band, np.arange(M + 1), side="left").astype(np.int32)


def np_step(s):
    s = np.asarray(s, dtype=np.int32)
    return np.ldexp(C4[s & 3], (s >> 2).astype(np.int32)).astype(np.float32)


def np_inv(s):
    s = np.asarray(s, dtype=np.int32)
    return np.ldexp(IC4[s & 3], (-(s >> 2)).astype(np.int32)).astype(np.float32)


CRIT = (np_step(S_ALL) * SQRT3).astype(np.float32)   # fp32(step(s) * SQRT3), strictly increasing in s


def np_quantize(X, thr, off):
    """Rules 3 and 4 on X, thr [B, F, N, C] float32 -> codes int16, sf int8 [B, F, M, C]."""
    X = np.asarray(X, dtype=np.float32)
    thr = np.asarray(thr, dtype=np.float32)
    B, F, N, C = X.shape
    M = len(off) - 1
    sf = np.zeros((B, F, M, C), dtype=np.int8)
    codes = np.zeros(X.shape, dtype=np.int16)
    for j in range(M):
        a, b = off[j], off[j + 1]
        if a == b:
            continue
        xs, ts = X[:, :, a:b, :], thr[:, :, a:b, :]
        bad = ~(np.isfinite(xs) & np.isfinite(ts)).all(axis=2)
        with np.errstate(invalid="ignore"):
            m = np.where(bad, np.float32(1), ts.min(axis=2))
        s = (np.searchsorted(CRIT, m, side="right") - 128).astype(np.int32)
        s = np.maximum(s, -127)
        s = np.where(bad, -128, s)
        sf[:, :, j, :] = s
        inv = np_inv(np.where(bad, 0, s))[:, :, None, :]
        with np.errstate(invalid="ignore", over="ignore"):
            q = np.clip(np.rint((xs * inv).astype(np.float32)), -32767, 32767)
        q = np.where(bad[:, :, None, :], 0, q)
        codes[:, :, a:b, :] = q.astype(np.int16)
    return codes, sf


def np_dequantize(codes, sf, off):
    """Rule 5: fp32(q * step(sf)); NaN for sf = -128."""
    M = len(off) - 1
    band = np.repeat(np.arange(M), np.diff(off))
    s = sf[:, :, band, :].astype(np.int32)
    st = np.where(s == -128, np.float32(np.nan), np_step(np.where(s == -128, 0, s)))
    return (codes.astype(np.float32) * st).astype(np.float32)


def check_guarantee(X, thr, codes, sf, Xh, off):
    """Rule 6 on every bin whose code did not saturate and whose band is representable."""
    M = len(off) - 1
    band = np.repeat(np.arange(M), np.diff(off))
    s = sf[:, :, band, :].astype(np.int32)
    ok = (np.abs(codes) < 32767) & (s != -128)
    st = np_step(np.where(s == -128, 0, s)).astype(np.float64)
    err = np.abs(Xh.astype(np.float64) - X.astype(np.float64))
    ax = np.abs(X.astype(np.float64))
    assert np.all(err[ok] <= 0.5 * st[ok] * (1 + 1e-6) + 1e-6 * ax[ok])
    tight = ok & (s > -127)   # (sf = -127 may be forced by a band minimum below the smallest step)
    bound = thr.astype(np.float64) / (2 * math.sqrt(3)) * (1 + 1e-6) + 1e-6 * ax
    assert np.all(err[tight] <= bound[tight])


# ---- CPU -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,N,M", [(48000, 1024, 64), (48000, 2048, 64), (44100, 256, 48), (32768, 64, 64),
                                    (96000, 2048, 64), (48000, 960, 64)])
def test_scale_band_offsets(sr, N, M):
    p = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M)
    off = p.scale_band_offsets
    assert off.dtype == np.int32 and off.shape == (M + 1,)
    assert off[0] == 0 and off[M] == N
    assert np.all(np.diff(off) >= 0)
    np.testing.assert_array_equal(off, np_offsets(sr, N, M))


def test_scale_bands_host_rejects_bad_arguments():
    lib = _lib.load()
    out = np.zeros(65, dtype=np.int32)
    p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.ac_psy_scale_bands_host(48000.0, 0, 64, p) == _lib.AC_EINVAL
    assert lib.ac_psy_scale_bands_host(-1.0, 1024, 64, p) == _lib.AC_EINVAL
    assert lib.ac_psy_scale_bands_host(48000.0, 1024, 64, None) == _lib.AC_EINVAL


def test_step_tables():
    assert (np.array([-5]) >> 2)[0] == -2 and (np.array([-5]) & 3)[0] == 3
    assert np.all(np.diff(CRIT) > 0)
    assert np_step(0) == 1 and np_step(4) == 2 and np_step(-4) == 0.5
    np.testing.assert_allclose(np_step(S_ALL).astype(np.float64) * np_inv(S_ALL), 1.0, rtol=2e-7)


def _adversarial(rng, N=256, M=48, sr=44100):
    off = np_offsets(sr, N, M)
    B, F, C = 2, 6, 2
    X = (rng.standard_normal((B, F, N, C)) * 10.0 ** rng.uniform(-6, 0, (B, F, 1, C))).astype(np.float32)
    thr = (np.abs(rng.standard_normal((B, F, N, C))) * 1e-3 + 1e-7).astype(np.float32)
    thr[0, 1] = np.float32(math.sqrt(1e-14))           # the smallest threshold the masking model gives
    X[0, 2] = 0.0                                       # zero row
    # values exactly at the half-steps of their band's step (ties: round half to even)
    codes0, sf0 = np_quantize(X, thr, off)
    band = np.repeat(np.arange(M), np.diff(off))
    st = np_step(np.where(sf0 == -128, 0, sf0).astype(np.int32))[:, :, band, :]
    k = rng.integers(-50, 50, (N, C)).astype(np.float32)
    X[1, 0] = ((k + 0.5) * st[1, 0]).astype(np.float32)
    X[1, 1, : N // 2] = 1e4                             # saturating codes
    X[1, 2, 5, 0] = np.nan
    thr[1, 3, 7, 1] = np.inf
    X[1, 4, 100, 0] = -np.inf
    return X, thr, off


def test_restatement_obeys_the_guarantee():
    rng = np.random.default_rng(7)
    for _ in range(3):
        X, thr, off = _adversarial(rng)
        codes, sf = np_quantize(X, thr, off)
        Xh = np_dequantize(codes, sf, off)
        check_guarantee(X, thr, codes, sf, Xh, off)
        assert sf[1, 2, :, 0].min() == -128 and sf[1, 3, :, 1].min() == -128
        band = np.repeat(np.arange(len(off) - 1), np.diff(off))
        bad = sf[:, :, band, :] == -128
        assert np.all(codes[bad] == 0) and np.all(np.isnan(Xh[bad]))
        assert np.abs(codes[1, 1]).max() == 32767
        assert np.all(np.isfinite(Xh[~bad]))   # every representable bin dequantises to a finite value


# ---- GPU -----------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _encoded(N, C, B=2, K=5, seed=0, sr=48000, M=64):
    codec = audiocodec_amd.AudioCodec(sr, N, bark_bands_n=M)
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-1, 1, (B, K * N, C)) * np.linspace(0.01, 1, K * N)[None, :, None]).astype(np.float32)
    X, _, thr = codec.encode(_dev(x))
    return codec, x, X, thr


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("N,C", [(12, 2), (64, 2), (256, 2), (512, 2), (960, 2), (1024, 2), (2048, 2), (4096, 2),
                                 (1024, 1), (1024, 3), (1024, 6), (960, 1), (256, 3), (64, 6), (2048, 1)])
def test_quantize_bit_exact(N, C):
    codec, _, X, thr = _encoded(N, C)
    psy = codec.psy
    off = psy.scale_band_offsets
    Xn, tn = X.cpu().numpy(), thr.cpu().numpy()
    # injected rows: zeros, saturating values, NaN / Inf samples
    Xn[0, 1] = 0.0
    Xn[1, 2, : N // 2] *= 1e9
    Xn[0, 3, N // 3, 0] = np.nan
    tn[1, 0, N - 1, C - 1] = np.inf
    Xn[1, 3, 0, 0] = -np.inf
    codes, sf = psy.quantize(_dev(Xn), _dev(tn))
    rc, rs = np_quantize(Xn, tn, off)
    np.testing.assert_array_equal(sf.cpu().numpy(), rs)
    np.testing.assert_array_equal(codes.cpu().numpy(), rc)
    assert (rs == -128).any() and (np.abs(rc) == 32767).any()
    Xh = psy.dequantize(codes, sf).cpu().numpy()
    ref = np_dequantize(rc, rs, off)
    np.testing.assert_array_equal(Xh.view(np.uint32)[~np.isnan(ref)], ref.view(np.uint32)[~np.isnan(ref)])
    assert np.array_equal(np.isnan(Xh), np.isnan(ref))


@gpu
@pytest.mark.parametrize("N,M,C", [(256, 4096, 2), (1024, 600, 7)])
def test_quantize_channel_groups(N, M, C):
    """Band slots of all channels that do not fit one workgroup's LDS: the channels split over groups (the last one partial
    at 600 bands x 7 channels: groups of 6)."""
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=N, bark_bands_n=M)
    off = psy.scale_band_offsets
    rng = np.random.default_rng(N + M + C)
    X = (rng.standard_normal((2, 3, N, C)) * 10.0 ** rng.uniform(-4, 0, (2, 3, 1, C))).astype(np.float32)
    thr = (np.abs(rng.standard_normal((2, 3, N, C))) * 1e-3 + 1e-7).astype(np.float32)
    X[1, 2, N - 1, C - 1] = np.nan
    codes, sf = psy.quantize(_dev(X), _dev(thr))
    rc, rs = np_quantize(X, thr, off)
    np.testing.assert_array_equal(sf.cpu().numpy(), rs)
    np.testing.assert_array_equal(codes.cpu().numpy(), rc)
    assert (rs == -128).any()


@gpu
def test_dequantize_bit_exact_on_random_codes():
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=1024, bark_bands_n=64)
    off = psy.scale_band_offsets
    rng = np.random.default_rng(3)
    codes = rng.integers(-32767, 32768, (3, 4, 1024, 2)).astype(np.int16)
    sf = rng.integers(-128, 128, (3, 4, 64, 2)).astype(np.int8)
    Xh = psy.dequantize(_dev(codes), _dev(sf)).cpu().numpy()
    ref = np_dequantize(codes, sf, off)
    assert np.array_equal(np.isnan(Xh), np.isnan(ref))
    keep = ~np.isnan(ref)
    np.testing.assert_array_equal(Xh.view(np.uint32)[keep], ref.view(np.uint32)[keep])


def decode_quantized_bit_equal(N, C, launches, sr=48000):
    """The body of test_decode_quantized_bit_equal at a sample rate; returns (codec, codes, sf) for further checks."""
    codec, _, X, thr = _encoded(N, C, B=3, K=7, sr=sr)
    assert codec.decode_quantized_launches(C) == launches
    codes, sf = codec.psy.quantize(X, thr)
    Xh = codec.psy.dequantize(codes, sf)
    assert torch.equal(codec.decode_quantized(codes, sf), codec.decode(Xh))
    if N in (1024, 2048, 960):   # (16-bit PCM sizes of both paths)
        assert torch.equal(codec.decode_quantized(codes, sf, pcm16=True), codec.decode(Xh, pcm16=True))
    return codec, codes, sf


@gpu
@pytest.mark.parametrize("N,C,launches", [(1024, 2, 1), (1024, 1, 1), (2048, 2, 1), (2048, 1, 1), (960, 2, 2), (1024, 3, 2),
                                          (512, 1, 2)])
def test_decode_quantized_bit_equal(N, C, launches):
    decode_quantized_bit_equal(N, C, launches)


@gpu
def test_decode_quantized_chip_filling():
    """One bench-sized launch of the fused synthesis against the independent dequantize + inverse path."""
    codec, _, X, thr = _encoded(1024, 2, B=96, K=468, seed=5)
    assert codec.decode_quantized_launches(2) == 1
    codes, sf = codec.psy.quantize(X, thr)
    del X, thr
    a = codec.decode_quantized(codes, sf)
    b = codec.decode(codec.psy.dequantize(codes, sf))
    assert torch.equal(a, b)


@gpu
@pytest.mark.parametrize("N,C,pcm16", [(1024, 2, False), (960, 1, True), (2048, 3, False)])
def test_encode_quantized_end_to_end(N, C, pcm16):
    codec, x, X, thr = _encoded(N, C, B=2, K=6, seed=11)
    xin = _dev(np.round(x * 32767).astype(np.int16)) if pcm16 else _dev(x)
    if pcm16:
        X, _, thr = codec.encode(xin)
    codes, sf = codec.encode_quantized(xin)
    rc, rs = codec.psy.quantize(X, thr)
    assert torch.equal(codes, rc) and torch.equal(sf, rs)
    off = codec.psy.scale_band_offsets
    Xh = codec.psy.dequantize(codes, sf).cpu().numpy()
    check_guarantee(X.cpu().numpy(), thr.cpu().numpy(), codes.cpu().numpy(), sf.cpu().numpy(), Xh, off)


@gpu
def test_error_paths():
    codec, x, X, thr = _encoded(1024, 2, B=1, K=2)
    psy = codec.psy
    codes, sf = psy.quantize(X, thr)
    with pytest.raises(ValueError):
        psy.quantize(X.double(), thr.double())
    with pytest.raises(ValueError):
        psy.quantize(X, thr[:, :-1])
    with pytest.raises(ValueError):
        psy.dequantize(codes.int(), sf)
    with pytest.raises(ValueError):
        psy.dequantize(codes, sf.short())
    with pytest.raises(ValueError):
        psy.dequantize(codes, sf[:, :, :-1])
    with pytest.raises(ValueError):
        codec.decode_quantized(codes.float(), sf)
    with pytest.raises(ValueError):
        psy.dequantize(codes.cpu(), sf.cpu())
    Xg = X.clone().requires_grad_()
    with pytest.raises(ValueError, match="add_noise"):
        psy.quantize(Xg, thr)
    with pytest.raises(ValueError, match="add_noise"):
        codec.encode_quantized(_dev(x).requires_grad_())
    for dt in (torch.float64, torch.bfloat16):
        other = audiocodec_amd.AudioCodec(48000, 1024, compute_dtype=dt)
        with pytest.raises(NotImplementedError, match="float32"):
            other.psy.quantize(X.to(dt), thr.to(dt))
        with pytest.raises(NotImplementedError, match="float32"):
            other.decode_quantized(codes, sf)
    # a view that starts 2 bytes into its allocation: the Python layer copies it, the C ABI refuses it
    store = torch.empty(codes.numel() + 1, dtype=torch.int16, device=codes.device)
    view = store[1:].view(codes.shape)
    view.copy_(codes)
    assert view.data_ptr() % 16 == 2
    assert torch.equal(psy.dequantize(view, sf), psy.dequantize(codes, sf))
    lib = _lib.load()
    Xh = torch.empty(X.shape, dtype=torch.float32, device=X.device)
    st = lib.ac_dequantize(psy._plan(X.device), ctypes.c_void_p(view.data_ptr()), ctypes.c_void_p(sf.data_ptr()),
                           ctypes.c_void_p(Xh.data_ptr()), 1, X.shape[1], 2, None)
    assert st == _lib.AC_EINVAL
    st = lib.ac_decode_quantized(codec.mdct._plan(X.device), psy._plan(X.device), ctypes.c_void_p(codes.data_ptr()),
                                 ctypes.c_void_p(sf.data_ptr()), None, None, None, 1, X.shape[1], 2, None)
    assert st == _lib.AC_EINVAL


@gpu
def test_side_stream():
    codec, _, X, thr = _encoded(1024, 2, B=4, K=20)
    ref_codes, ref_sf = codec.psy.quantize(X, thr)
    ref_x = codec.decode_quantized(ref_codes, ref_sf)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        codes, sf = codec.psy.quantize(X, thr)
        x = codec.decode_quantized(codes, sf)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(codes, ref_codes) and torch.equal(sf, ref_sf) and torch.equal(x, ref_x)
