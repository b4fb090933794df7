"""The quantising fused encode at filters_n = 1024 (k_fwd_fast_q): ``ac_encode_fused_ex`` with
``AC_EMIT_CODES`` and ``AudioCodec.encode_quantized`` on top of it.

The reference of every GPU comparison is ``psy.quantize(X, thr)`` on the X and thr of ``codec.encode(x)`` -- two launches
through float32 tensors in HBM -- and every comparison is bit for bit (``torch.equal``; float tensors that may hold NaN are
compared as their int32 patterns).  One case also holds the numpy restatement of tests/test_quantizer.py against them.
"""

import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib
from conftest import ROOT

import chip_scale_inputs as csi
from test_quantizer import np_quantize

gpu = pytest.mark.gpu
N0 = 1024


# ---- CPU: the interface (needs the built library) ----------------------------------------------------------------
def test_header_defines_the_flag():
    text = open(os.path.join(ROOT, "include", "audiocodec_amd.h")).read()
    assert re.search(r"\bAC_EMIT_CODES\s*=\s*4\b", text)
    assert _lib.AC_EMIT_CODES == 4


def test_library_exports_the_launch_query():
    lib = _lib.load()
    assert "ac_encode_quantized_launches" in _lib.PROTOTYPES
    assert lib.ac_encode_quantized_launches(None, None, 2) == 0
    assert lib.ac_version() == 171


def test_codec_has_the_launch_query():
    assert callable(getattr(audiocodec_amd.AudioCodec, "encode_quantized_launches", None))


# ---- GPU ---------------------------------------------------------------------------------------------------------
def _bits(a):
    return a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _where(a, b):
    """For a failing comparison's message: how many elements differ, the first of them, and how many of them are NaN in both."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return "shape / dtype %s %s against %s %s" % (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    bad = _bits(a) != _bits(b)
    n = int(bad.sum())
    if not n:
        return "equal"
    idx = tuple(int(i) for i in torch.nonzero(bad)[0])
    both_nan = int((bad & torch.isnan(a) & torch.isnan(b)).sum()) if a.dtype.is_floating_point else 0
    return "%d of %d elements differ (%d NaN in both), first at %s: %r against %r" % (
        n, a.numel(), both_nan, idx, _bits(a)[idx].item(), _bits(b)[idx].item())


def _pcm(N, C, B, K, seed=0, inject=True):
    """The ramped noise of test_quantizer._encoded; with ``inject`` (B >= 3, K >= 4): two all-zero blocks in clip 1 (frame 2
    of it is all zero), a NaN sample in clip 0 and an Inf sample in clip 2."""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-1, 1, (B, K * N, C)) * np.linspace(0.01, 1, K * N)[None, :, None]).astype(np.float32)
    if inject:
        assert B >= 3 and K >= 4
        x[1, N:3 * N] = 0.0
        x[0, 2 * N + 17, 0] = np.nan
        x[2, 3 * N + 5, C - 1] = np.inf
    return torch.from_numpy(x).cuda()


def _reference(codec, x, drown=0.0):
    X, t, thr = codec.encode(x, drown)
    codes, sf = codec.psy.quantize(X, thr)
    return X, t, thr, codes, sf


def _emit_codes(codec, x, want, drown=0.0):
    """ac_encode_fused_ex(AC_EMIT_CODES) with X / t / thr given where ``want`` names them: (status, X, t, thr, codes, sf)"""
    lib = _lib.load()
    B, S, C = x.shape
    N, M = codec.filters_n, codec.psy.bark_bands_n
    K = S // N
    dev = x.device
    out = {"X": torch.full((B, K + 1, N, C), 7.0, device=dev) if "X" in want else None,
           "t": torch.full((B, K + 1, 1, C), 7.0, device=dev) if "t" in want else None,
           "thr": torch.full((B, K + 1, N, C), 7.0, device=dev) if "thr" in want else None}
    codes = torch.full((B, K + 1, N, C), 77, dtype=torch.int16, device=dev)
    sf = torch.full((B, K + 1, M, C), 77, dtype=torch.int8, device=dev)

    def p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    st = lib.ac_encode_fused_ex(codec.mdct._plan(dev), codec.psy._plan(dev), p(x), p(out["X"]), p(out["t"]), p(out["thr"]),
                                float(drown), _lib.AC_EMIT_CODES, p(codes), p(sf), 0, B, K, C, None)
    torch.cuda.synchronize()
    return st, out["X"], out["t"], out["thr"], codes, sf


SMALL = [  # C, spreading, B, K, drown, inject
    (1, None, 3, 5, 0.0, True), (2, None, 3, 5, 0.0, True), (1, "f32", 3, 5, 0.0, True), (2, "f32", 3, 5, 0.0, True),
    (2, None, 3, 5, 0.5, True), (1, None, 3, 5, 0.5, True), (2, None, 1, 1, 0.0, False), (1, None, 1, 1, 0.0, False),
    (2, None, 2, 0, 0.0, False), (1, "f32", 3, 0, 0.0, False)]


@gpu
@pytest.mark.parametrize("C,spreading,B,K,drown,inject", SMALL)
def test_small_shapes_bit_exact(C, spreading, B, K, drown, inject):
    """Both edge frames of every clip (6 frames per clip), a half-empty mono pair (B odd), an all-zero frame, NaN and Inf."""
    codec = audiocodec_amd.AudioCodec(48000, N0, spreading=spreading)
    assert codec.encode_quantized_launches(C) == 1
    x = _pcm(N0, C, B, K, seed=C + 2 * B + K, inject=inject)
    X, _, thr, rc, rs = _reference(codec, x, drown)
    codes, sf = codec.encode_quantized(x, drown)
    assert codes.dtype == torch.int16 and codes.shape == (B, K + 1, N0, C)
    assert sf.dtype == torch.int8 and sf.shape == (B, K + 1, 64, C)
    assert torch.equal(sf, rs)
    assert torch.equal(codes, rc)
    if inject:
        assert bool((sf == -128).any())
        assert float(X[1, 2].abs().max()) == 0.0 and int(codes[1, 2].abs().max()) == 0
        assert int(codes.abs().max()) > 0
    if (C, spreading, drown, inject) == (2, None, 0.0, True):   # ... and the numpy restatement on the same tensors
        nc, ns = np_quantize(X.cpu().numpy(), thr.cpu().numpy(), codec.psy.scale_band_offsets)
        np.testing.assert_array_equal(sf.cpu().numpy(), ns)
        np.testing.assert_array_equal(codes.cpu().numpy(), nc)


@gpu
@pytest.mark.parametrize("C", [1, 2])
def test_optional_outputs(C):
    """X, t and thr under AC_EMIT_CODES: each equals encode()'s where given, and any subset may be NULL."""
    codec = audiocodec_amd.AudioCodec(48000, N0)
    x = _pcm(N0, C, 3, 5, seed=40 + C)
    X, t, thr, rc, rs = _reference(codec, x)
    for k in range(4):
        for want in itertools.combinations(("X", "t", "thr"), k):
            st, gX, gt, gthr, codes, sf = _emit_codes(codec, x, want)
            assert st == _lib.AC_OK, (want, _lib.load().ac_last_error())
            assert torch.equal(sf, rs) and torch.equal(codes, rc), want
            for name, got, ref in (("X", gX, X), ("t", gt, t), ("thr", gthr, thr)):
                assert (got is None) == (name not in want)
                assert got is None or _same(got, ref), (want, name, _where(got, ref))


def _flags_refused(codec, x):
    lib = _lib.load()
    B, S, C = x.shape
    K = S // codec.filters_n
    dev = x.device
    X = torch.empty((B, K + 1, codec.filters_n, C), device=dev)
    t = torch.empty((B, K + 1, 1, C), device=dev)
    codes = torch.empty(X.shape, dtype=torch.int16, device=dev)
    sf = torch.empty((B, K + 1, codec.psy.bark_bands_n, C), dtype=torch.int8, device=dev)
    p = lambda a: ctypes.c_void_p(a.data_ptr())   # noqa: E731
    return lib.ac_encode_fused_ex(codec.mdct._plan(dev), codec.psy._plan(dev), p(x), p(X), p(t), p(X), 0.0,
                                  _lib.AC_EMIT_CODES | _lib.AC_EMIT_NOISY, p(codes), p(sf), 0, B, K, C, None)


@gpu
def test_flag_is_exclusive():
    codec = audiocodec_amd.AudioCodec(48000, N0)
    assert _flags_refused(codec, _pcm(N0, 2, 1, 1, inject=False)) == _lib.AC_EINVAL


FALLBACK = [(960, 2, None), (1024, 3, None), (2048, 2, None), (1024, 2, "bf16_mfma")]


@gpu
@pytest.mark.parametrize("N,C,spreading", FALLBACK)
def test_fallback_is_the_composition(N, C, spreading):
    codec = audiocodec_amd.AudioCodec(48000, N, spreading=spreading)
    assert codec.encode_quantized_launches(C) == 2
    x = _pcm(N, C, 3, 5, seed=N + C)
    X, t, thr, rc, rs = _reference(codec, x)
    codes, sf = codec.encode_quantized(x)
    assert torch.equal(codes, rc) and torch.equal(sf, rs)
    st, gX, gt, gthr, codes, sf = _emit_codes(codec, x, ("X", "t", "thr"))
    assert st == _lib.AC_OK, _lib.load().ac_last_error()
    assert torch.equal(codes, rc) and torch.equal(sf, rs) and _same(gX, X) and _same(gt, t) and _same(gthr, thr)
    for want in (("t", "thr"), ("X", "thr"), ("X", "t"), ()):
        st = _emit_codes(codec, x, want)[0]
        assert st == _lib.AC_EINVAL, want
        assert b"intermediates" in _lib.load().ac_last_error()


@gpu
def test_pcm16_input_takes_two_launches():
    codec = audiocodec_amd.AudioCodec(48000, N0)
    x = _pcm(N0, 2, 3, 5, seed=9, inject=False)
    pcm = torch.round(x * 32767).to(torch.int16)
    X, _, thr = codec.encode(pcm)
    rc, rs = codec.psy.quantize(X, thr)
    codes, sf = codec.encode_quantized(pcm)
    assert torch.equal(codes, rc) and torch.equal(sf, rs)


@gpu
def test_nofuse_hook(monkeypatch):
    codec = audiocodec_amd.AudioCodec(48000, N0)
    x = _pcm(N0, 2, 3, 5, seed=21)
    fused = codec.encode_quantized(x)
    assert codec.encode_quantized_launches(2) == 1
    monkeypatch.setenv("AC_ENCODE_QUANT_NOFUSE", "1")
    assert codec.encode_quantized_launches(2) == 2 and codec.encode_quantized_launches(1) == 2
    two = codec.encode_quantized(x)
    assert torch.equal(two[0], fused[0]) and torch.equal(two[1], fused[1])
    assert _emit_codes(codec, x, ("t", "thr"))[0] == _lib.AC_EINVAL
    monkeypatch.delenv("AC_ENCODE_QUANT_NOFUSE")
    assert codec.encode_quantized_launches(2) == 1


@gpu
@pytest.mark.parametrize("C", [2, 1])
def test_chip_filling(C, monkeypatch):
    """>= 2048 workgroups of 4 waves x 4 frames, against the two launches in the same process."""
    codec = audiocodec_amd.AudioCodec(48000, N0)
    K = csi.blocks_per_clip(N0)
    B = csi.clips_for(N0, C, tasks_per_workgroup=16)
    pairs = B if C == 2 else (B + 1) // 2
    assert pairs * (K + 1) >= 16 * csi.MIN_WORKGROUPS
    x = csi.structured(B, K, N0, C, seed=300 + C)
    assert codec.encode_quantized_launches(C) == 1
    codes, sf = codec.encode_quantized(x)
    monkeypatch.setenv("AC_ENCODE_QUANT_NOFUSE", "1")
    assert codec.encode_quantized_launches(C) == 2
    rc, rs = codec.encode_quantized(x)
    assert torch.equal(sf, rs)
    assert torch.equal(codes, rc)
    assert int(codes.abs().max()) > 0


@pytest.fixture(scope="module")
def harness():
    from stream_order import Harness
    return Harness()


@gpu
@pytest.mark.parametrize("check", ["delayed_producer", "busy_default"])
def test_stream_contract(harness, check):
    """The contract ac_encode_fused_ex's row of test_stream_contract.py holds the older flags to, on the new one."""
    codec = audiocodec_amd.AudioCodec(48000, N0)
    assert codec.encode_quantized_launches(2) == 1
    x = _pcm(N0, 2, 4, 20, seed=77, inject=False)
    case = ([x], lambda x: codec.encode_quantized(x))
    getattr(harness, check)("encode_quantized[1024-2]", case)
