"""Concealment of lost rows in decode_packed: ``decode_packed(data, index, pcm16, lost=..., max_age=...)``.

A lost row is read from the last row of its clip and channel that arrived, at most ``max_age`` frames back, with every scale
factor lowered by 4 per frame of age (the spectrum halved, exactly); a row without such a source is silence.  Three
statements of it are held to each other, bit for bit (NaN payloads included), float32 and 16-bit PCM:

  * the kernel k_inv_fast_pl (one launch, where ``decode_packed_launches`` is 1);
  * the composition in torch ops (``psy.conceal_plan``, ``psy.unpack`` at its row starts, ``psy.conceal_fade``,
    ``decode_quantized``), which is what runs everywhere else;
  * ``decode_quantized`` on the codes and scale factors tests/conceal_reference.py (numpy, written frame by frame from the
    definition) makes of ``psy.unpack``'s output.
"""

import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib
from conceal_reference import FADE, MAX_AGE, np_conceal, np_conceal_plan, np_fade, np_src_index
from conftest import ROOT
from pack_reference import np_pack
from stream_order import Harness, same_bits
from test_encode_cbr import _input
from test_pack import _encoded
from test_quantizer import np_step

N0 = 1024
NOFUSE = "AC_DECODE_PACKED_NOFUSE"
AGES = (0, 1, 8, 31)


# ---- CPU -----------------------------------------------------------------------------------------------------------
def _lost(F, frames, B=1, C=1):
    lost = np.zeros((B, F, C), dtype=np.uint8)
    lost[:, list(frames)] = 1
    return lost


@pytest.mark.parametrize("max_age", [1, 3, 8, 31])
def test_plan_runs_of_max_age_and_one_more(max_age):
    F = 2 * max_age + 5
    # frame 0 arrives, then a run of exactly max_age lost rows: the last one is max_age old
    src, age = np_conceal_plan(_lost(F, range(1, 1 + max_age)), max_age)
    assert age[0, :, 0].tolist()[:max_age + 2] == list(range(max_age + 1)) + [0]
    assert (src[0, :max_age + 1, 0] == 0).all() and src[0, max_age + 1, 0] == max_age + 1
    # a run of max_age + 1: its last row is muted, the others are not
    src, age = np_conceal_plan(_lost(F, range(1, 2 + max_age)), max_age)
    assert (src[0, 1:max_age + 1, 0] == 0).all() and src[0, max_age + 1, 0] == -1 and age[0, max_age + 1, 0] == 0
    assert src[0, max_age + 2, 0] == max_age + 2


def test_plan_frame_0_lost_is_muted():
    src, age = np_conceal_plan(_lost(5, [0, 1]), 8)
    assert src[0, :, 0].tolist() == [-1, -1, 2, 3, 4] and not age.any()


def test_plan_max_age_0_is_zero_filling_and_31_is_the_limit():
    lost = _lost(40, [3, 4, 10])
    src, age = np_conceal_plan(lost, 0)
    assert np.array_equal(src[0, :, 0], np.where(lost[0, :, 0] != 0, -1, np.arange(40))) and not age.any()
    src, age = np_conceal_plan(_lost(40, range(1, 40)), 31)
    assert age[0, :32, 0].tolist() == list(range(32)) and (src[0, 32:, 0] == -1).all()
    with pytest.raises(AssertionError):
        np_conceal_plan(lost, 32)


def test_plan_channels_and_clips_are_independent():
    lost = np.zeros((2, 4, 2), dtype=np.uint8)
    lost[1, 0, 0] = 1        # frame 0 of clip 1 must not take clip 0's last frame
    lost[0, 2:, 1] = 1       # ... nor channel 1 anything from channel 0
    src, age = np_conceal_plan(lost, 8)
    assert src[1, 0, 0] == -1 and src[1, 1:, 0].tolist() == [1, 2, 3] and src[1, :, 1].tolist() == [0, 1, 2, 3]
    assert src[0, :, 1].tolist() == [0, 1, 1, 1] and age[0, :, 1].tolist() == [0, 0, 1, 2] and src[0, :, 0].tolist() == [0, 1, 2, 3]
    index = np.arange(16, dtype=np.int64).reshape(2, 4, 2) * 100
    got, a8 = np_src_index(index, lost, 99999, 8)
    assert got[1, 0, 0] == 99999 and got[0, 3, 1] == index[0, 1, 1] and a8.dtype == np.uint8 and got.dtype == np.int64


def test_fade_is_an_exact_halving_per_frame():
    """step(s - 4a) == ldexp(step(s), -a) in float32 for every s in [-127, 127] and a in [0, 31] with s - 4a >= -127."""
    assert FADE == 4 and MAX_AGE == 31
    n = 0
    for a in range(MAX_AGE + 1):
        s = np.arange(-127 + FADE * a, 128)
        got, want = np_step(s - FADE * a), np.ldexp(np_step(s), -a).astype(np.float32)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), a
        assert (got > 0).all() and np.isfinite(got).all()
        n += len(s)
    assert n > 6000
    # the clamp at -127 and the -128 pass-through
    sf = np.array([-128, -127, -126, -124, -123, -120, 0, 127], dtype=np.int8).reshape(1, 1, 8, 1)
    assert np_fade(sf, np.array([[[0]]])).ravel().tolist() == sf.ravel().tolist()
    assert np_fade(sf, np.array([[[1]]])).ravel().tolist() == [-128, -127, -127, -127, -127, -124, -4, 123]
    assert np_fade(sf, np.array([[[2]]])).ravel().tolist() == [-128, -127, -127, -127, -127, -127, -8, 119]
    assert np_fade(sf, np.array([[[31]]])).ravel().tolist() == [-128, -127, -127, -127, -127, -127, -124, 3]


def test_abi_has_the_conceal_struct_and_constants():
    text = open(os.path.join(ROOT, "include", "audiocodec_amd.h")).read()
    m = re.search(r"typedef struct ac_conceal \{(.*?)\} ac_conceal;", text, re.S)
    assert m, "ac_conceal is not declared"
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    assert [" ".join(f.split()) for f in body.split(";") if f.strip()] == ["const uint8_t* lost", "int32_t max_age"]
    assert re.search(r"#define\s+AC_CONCEAL_FADE\s+4\b", text) and re.search(r"#define\s+AC_CONCEAL_MAX_AGE\s+31\b", text)
    assert (_lib.AC_CONCEAL_FADE, _lib.AC_CONCEAL_MAX_AGE) == (4, 31)
    P = _lib.Conceal
    assert [f[0] for f in P._fields_] == ["lost", "max_age"]
    assert (P.lost.offset, P.max_age.offset, P.lost.size, P.max_age.size) == (0, 8, 8, 4) and ctypes.sizeof(P) == 16
    sig = inspect.signature(audiocodec_amd.AudioCodec.decode_packed)
    for name, default in (("lost", None), ("max_age", 8)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default
    assert callable(audiocodec_amd.PsychoacousticModel.conceal_plan)


# ---- GPU -----------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _signal(C, Kp):
    """Packed rows of seeded noise with one NaN sample (sf = -128 bands), [3, Kp, C], with their unpacked codes and sf."""
    codec, x = _encoded(N0, C, B=3, K=max(Kp - 1, 1), seed=20 + Kp, nan=Kp > 1)
    data, index = codec.encode_packed(_dev(x[:, :(Kp - 1) * N0]))
    assert tuple(index.shape) == (3, Kp, C)
    codes, sf = codec.psy.unpack(data, index)
    return codec, data, index, codes.cpu().numpy(), sf.cpu().numpy()


def _runs(B, Kp, C, max_age, longer):
    """Per channel and clip: a good frame, then runs of max_age (+ 1 with `longer`) lost rows with one good row between them."""
    lost = np.zeros((B, Kp, C), dtype=np.uint8)
    n = max_age + (1 if longer else 0)
    for b in range(B):
        for c in range(C):
            f = 1 + (b + c) % 2
            while f < Kp:
                lost[b, f:f + n, c] = 1
                f += n + 1
    return lost


def _patterns(B, Kp, C, max_age):
    rng = np.random.default_rng(1000 * Kp + 10 * max_age + C)
    frame0 = np.zeros((B, Kp, C), dtype=np.uint8)
    frame0[:, 0] = 1
    return {"none": np.zeros((B, Kp, C), dtype=np.uint8), "all": np.ones((B, Kp, C), dtype=np.uint8), "frame 0": frame0,
            "runs of max_age": _runs(B, Kp, C, max_age, False), "runs of max_age + 1": _runs(B, Kp, C, max_age, True),
            "30 %": (rng.random((B, Kp, C)) < 0.3).astype(np.uint8)}


def _numpy_decode(codec, codes, sf, lost, max_age, pcm16):
    """decode_quantized on the rows tests/conceal_reference.py makes of the unpacked rows (numpy arrays)."""
    c2, s2 = np_conceal(codes, sf, lost, max_age)
    return codec.decode_quantized(_dev(c2), _dev(s2), pcm16=pcm16)


def _composition(codec, data, index, pcm16, lost, max_age):
    os.environ[NOFUSE] = "1"
    try:
        assert codec.decode_packed_launches(index.shape[2]) == 1 + codec.decode_quantized_launches(index.shape[2])
        return codec.decode_packed(data, index, pcm16, lost=lost, max_age=max_age)
    finally:
        del os.environ[NOFUSE]


def _hold(codec, data, index, lost, max_age, codes=None, sf=None, what=""):
    """The kernel, the composition and the numpy-concealed decode_quantized on one input; returns the float32 PCM."""
    C = index.shape[2]
    assert codec.decode_packed_launches(C) == 1
    if codes is None:
        codes, sf = (t.cpu().numpy() for t in codec.psy.unpack(data, index))
    lost_d = _dev(lost)
    out = None
    for pcm16 in (False, True):
        fused = codec.decode_packed(data, index, pcm16, lost=lost_d, max_age=max_age)
        comp = _composition(codec, data, index, pcm16, lost_d, max_age)
        ref = _numpy_decode(codec, codes, sf, lost, max_age, pcm16)
        assert fused.dtype == (torch.int16 if pcm16 else torch.float32)
        assert same_bits(comp, ref), "composition != numpy: %s max_age=%d pcm16=%s" % (what, max_age, pcm16)
        assert same_bits(fused, comp), "kernel != composition: %s max_age=%d pcm16=%s" % (what, max_age, pcm16)
        out = fused if not pcm16 else out
    return out


@gpu
@pytest.mark.parametrize("Kp", [1, 2, 7, 12])
@pytest.mark.parametrize("C", [1, 2])
def test_fused_against_the_composition(C, Kp, monkeypatch):
    """B = 3 (mono: the last pair has no second signal); every loss pattern at every max_age, both PCM formats.  Also: the
    plan of the torch helper against numpy, none lost == the plain decode, all lost == +0, and locality."""
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, data, index, codes, sf = _signal(C, Kp)
    plain = {p: codec.decode_packed(data, index, pcm16=p) for p in (False, True)}
    for max_age in AGES:
        for name, lost in _patterns(3, Kp, C, max_age).items():
            src, age = codec.psy.conceal_plan(index, _dev(lost), data.numel(), max_age)
            want_src, want_age = np_src_index(index.cpu().numpy(), lost, data.numel(), max_age)
            assert src.dtype == torch.int64 and age.dtype == torch.uint8
            assert np.array_equal(src.cpu().numpy(), want_src) and np.array_equal(age.cpu().numpy(), want_age), (name, max_age)
            out = _hold(codec, data, index, lost, max_age, codes, sf, name)
            out16 = codec.decode_packed(data, index, True, lost=_dev(lost), max_age=max_age)
            if name == "none":
                assert same_bits(out, plain[False]) and same_bits(out16, plain[True])
                assert same_bits(codec.decode_packed(data, index, lost=_dev(lost).bool(), max_age=max_age), plain[False])
            if name == "all":      # +0 everywhere: not -0, not NaN
                assert int((out.view(torch.int32) != 0).sum()) == 0 and int((out16 != 0).sum()) == 0
            # locality: block n overlap-adds frames n - 1 and n; where both arrived (or do not exist) it is the plain block
            ok = np.ones((3, Kp + 2, C), dtype=bool)
            ok[:, 1:-1] = lost == 0
            clean = _dev(ok[:, :-1] & ok[:, 1:])                                   # [3, Kp + 1, C]
            for got, ref in ((out, plain[False]), (out16, plain[True])):
                g, r = (t.view(3, Kp + 1, N0, C).movedim(2, 3)[clean] for t in (got, ref))
                assert same_bits(g, r), (name, max_age)


@gpu
@pytest.mark.parametrize("C,B,K", [(2, 64, 64), (1, 129, 96)])
def test_production_strip_length(C, B, K, monkeypatch):
    """Enough strips for the strips of 2 (stereo) and 3 (mono) blocks of the bench workload (test_decode_packed_fused): the
    source row of a lost row lies strips back, in another wave's or another workgroup's strip."""
    monkeypatch.delenv(NOFUSE, raising=False)
    codec = audiocodec_amd.AudioCodec(48000, N0)
    g = torch.Generator("cuda").manual_seed(B + K)
    x = (torch.rand((B, K * N0, C), device="cuda", generator=g) * 2 - 1) * torch.linspace(0.01, 1, K * N0, device="cuda")[None, :, None]
    data, index = codec.encode_packed(x)
    pairs = B if C == 2 else (B + 1) // 2
    assert pairs * ((K + 2 + (3 - C)) // (4 - C)) >= 2048
    lost = torch.rand((B, K + 1, C), device="cuda", generator=g) < 0.3
    lost[0, 5:40] = True
    for max_age in (8, 31):
        for pcm16 in (False, True):
            fused = codec.decode_packed(data, index, pcm16, lost=lost, max_age=max_age)
            assert same_bits(fused, _composition(codec, data, index, pcm16, lost, max_age)), (max_age, pcm16)


@gpu
def test_crafted_scale_factors(monkeypatch):
    """Rows built with psy.pack from chosen codes and sf: bands at sf = -126 .. -120 (the clamp at -127 is met at ages 1 and
    2), and a band with sf = -128 in a source row: NaN in float32 in every frame concealed from it, 0 in 16-bit PCM."""
    monkeypatch.delenv(NOFUSE, raising=False)
    codec = audiocodec_amd.AudioCodec(48000, N0)
    rng = np.random.default_rng(5)
    B, F, C = 2, 8, 2
    codes = rng.integers(-300, 301, (B, F, N0, C)).astype(np.int16)
    sf = rng.integers(-30, 10, (B, F, 64, C)).astype(np.int8)
    sf[:, :, 10:17] = np.arange(-126, -119, dtype=np.int8)[None, None, :, None]
    sf[:, :, 40] = -127
    sf[1, 4, 20, 1] = -128                         # the source of frames 5, 6, 7 of (clip 1, channel 1)
    data, index = codec.psy.pack(_dev(codes), _dev(sf))
    lost = np.zeros((B, F, C), dtype=np.uint8)
    lost[:, 1:4, 0] = 1                            # ages 1, 2, 3 from frame 0
    lost[:, 5:8, 1] = 1                            # ages 1, 2, 3 from frame 4
    c2, s2 = np_conceal(codes, sf, lost, 8)
    assert s2[0, 1, 10:17, 0].tolist() == [-127, -127, -127, -127, -126, -125, -124]
    assert s2[0, 2, 10:17, 0].tolist() == [-127] * 7 and s2[1, 7, 20, 1] == -128 and s2[0, 3, 40, 0] == -127
    out = _hold(codec, data, index, lost, 8, what="crafted sf")
    out16 = codec.decode_packed(data, index, True, lost=_dev(lost), max_age=8)
    blocks = out.view(B, F + 1, N0, C)
    assert bool(torch.isnan(blocks[1, 4:, :, 1]).all())                  # frames 4 .. 7: blocks 4 .. 8
    assert bool(torch.isfinite(blocks[1, :4, :, 1]).all()) and bool(torch.isfinite(blocks[:, :, :, 0]).all())
    assert int(out16.view(B, F + 1, N0, C)[1, 4:, :, 1].abs().max()) == 0
    assert int(out16.view(B, F + 1, N0, C)[1, :4, :, 1].abs().max()) > 0
    # The faded spectrum is the source's times 2^-age, exactly, where the clamp is not met, and so is its PCM (a power of two
    # commutes with every rounding of the synthesis): frame 0 alone in a clip of three frames, the other two empty rows.
    # Block 1 of the plain decode is the second half of frame 0 against an empty frame; with frames 1 .. age lost, block
    # age + 1 is the second half of frame 0 / 2^age against an empty frame (or the end of the clip).
    one = np.zeros((1, 3, N0, 1), dtype=np.int16)
    one[0, 0] = codes[0, 0, :, :1]
    s1 = np.zeros((1, 3, 64, 1), dtype=np.int8)
    s1[0, 0] = np.maximum(sf[0, 0, :, :1], -100)
    d1, i1 = codec.psy.pack(_dev(one), _dev(s1))
    src = codec.decode_packed(d1, i1).view(4, N0)
    assert int((src[1] != 0).sum()) > N0 // 2 and int((src[2:] != 0).sum()) == 0
    for age in (1, 2):
        l1 = np.zeros((1, 3, 1), dtype=np.uint8)
        l1[0, 1:1 + age] = 1
        faded = codec.decode_packed(d1, i1, lost=_dev(l1), max_age=8).view(4, N0)
        assert same_bits(faded[:1], src[:1])
        assert torch.equal(faded[age + 1], torch.ldexp(src[1], torch.tensor(-age, device="cuda"))), age


@gpu
def test_marked_row_as_a_source(monkeypatch):
    """A row that did not fit its slot (every width 31, `fits` False) as the source of the rows after it."""
    monkeypatch.delenv(NOFUSE, raising=False)
    cbr = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(320)
    x = _input(2, 3, 7, 11, True)
    data, index, fits = cbr.encode_packed_rows(x)
    assert tuple(index.shape) == (3, 8, 2)
    marked = [tuple(int(i) for i in w) for w in torch.nonzero(~fits[:, :7])]
    assert marked and bool(fits.any()), "no marked row with a frame after it"
    lost = np.zeros((3, 8, 2), dtype=np.uint8)
    for b, f, c in marked:
        lost[b, f + 1:, c] = 1
    out = _hold(cbr, data, index, lost, 8, what="marked source")
    b, f, c = marked[0]
    assert bool(torch.isnan(out.view(3, 9, N0, 2)[b, f + 1:, :, c]).all())


@gpu
@pytest.mark.parametrize("trim", [0, 3])
def test_source_rows_at_odd_starts(trim, monkeypatch):
    """Sources at the last row of data (not a plain load), off the 4-byte phase, before 0 and past the end (the inputs of
    test_decode_packed_fused.test_damaged_input), each followed by lost rows; and an index that is a permuted, strided view."""
    monkeypatch.delenv(NOFUSE, raising=False)
    codec = audiocodec_amd.AudioCodec(48000, N0)
    off = codec.psy.scale_band_offsets
    rng = np.random.default_rng(40 + trim)
    codes = rng.integers(-2, 3, (2, 4, N0, 2)).astype(np.int16)
    sf = rng.integers(-20, 20, (2, 4, 64, 2)).astype(np.int8)
    data, index = np_pack(codes, sf, off)
    idx = index.reshape(-1)
    n = len(data) - trim
    big = torch.full((n + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    big[:n] = _dev(data[:n])
    last, odd, neg, past, far = int(idx[-1]), int(idx[5]) + 1, -8, n, n + 10 ** 6
    # [2, 10, 2]: every special start followed by a lost row (whose own start is a good row's: it must not be read)
    starts = np.empty((2, 10, 2), dtype=np.int64)
    starts[0, :, 0] = [last, idx[0], odd, idx[1], neg, idx[2], past, idx[3], far, idx[4]]
    starts[0, :, 1] = [idx[6], last, last, odd, odd, neg, neg, n - 2, n - 2, idx[7]]
    starts[1, :, 0] = [odd, idx[8], idx[9], last, idx[10], idx[11], far, idx[12], last, last]
    starts[1, :, 1] = [idx[13], idx[14], idx[15], neg, idx[0], idx[1], int(idx[6]) + 2, idx[2], idx[3], last]
    lost = np.zeros((2, 10, 2), dtype=np.uint8)
    lost[0, 1::2, 0] = 1
    lost[0, 2::2, 1] = 1
    lost[1, [1, 2, 4, 5, 7, 9], 0] = 1
    lost[1, [4, 5, 7, 8], 1] = 1
    for max_age in (1, 8):
        _hold(codec, big[:n], _dev(starts), lost, max_age, what="odd starts")
        _hold(codec, big[:n], _dev(starts.reshape(4, 10, 1)[:3]), lost.reshape(4, 10, 1)[:3], max_age, what="odd starts, mono")
    # a permuted, strided view of index and of lost: the same rows as the contiguous tensors
    wide = _dev(np.ascontiguousarray(np.repeat(starts.transpose(2, 1, 0), 2, axis=1)))     # [2, 20, 2]
    view = wide.permute(2, 1, 0)[:, ::2]
    lview = _dev(np.ascontiguousarray(np.repeat(lost.transpose(2, 1, 0), 2, axis=1))).permute(2, 1, 0)[:, ::2]
    assert not view.is_contiguous() and not lview.is_contiguous() and torch.equal(view, _dev(starts))
    for pcm16 in (False, True):
        a = codec.decode_packed(big[:n], view, pcm16, lost=lview, max_age=8)
        assert same_bits(a, codec.decode_packed(big[:n], _dev(starts), pcm16, lost=_dev(lost), max_age=8))
        assert same_bits(a, _composition(codec, big[:n], view, pcm16, lview, 8))


@gpu
@pytest.mark.parametrize("N,C,B,Kp,nofuse", [(512, 3, 2, 5, False), (1024, 2, 2, 5, True)])
def test_where_the_fused_form_is_not_served(N, C, B, Kp, nofuse, monkeypatch):
    """The composition against the numpy-concealed decode_quantized: a configuration no kernel reads packed rows for, and
    filters_n = 1024 behind the switch."""
    monkeypatch.delenv(NOFUSE, raising=False)
    if nofuse:
        monkeypatch.setenv(NOFUSE, "1")
    codec, x = _encoded(N, C, B=B, K=Kp - 1, seed=3)
    data, index = codec.encode_packed(_dev(x))
    assert tuple(index.shape) == (B, Kp, C) and codec.decode_packed_launches(C) == 1 + codec.decode_quantized_launches(C)
    codes, sf = (t.cpu().numpy() for t in codec.psy.unpack(data, index))
    assert (sf == -128).any()
    for max_age in (0, 2, 8):
        for name, lost in _patterns(B, Kp, C, max_age).items():
            for pcm16 in ((False, True) if C <= 2 else (False,)):   # (no 16-bit PCM synthesis for three channels at 512)
                got = codec.decode_packed(data, index, pcm16, lost=_dev(lost), max_age=max_age)
                assert same_bits(got, _numpy_decode(codec, codes, sf, lost, max_age, pcm16)), (name, max_age, pcm16)


@pytest.fixture(scope="module")
def harness():
    assert torch.cuda.is_available(), "the stream contract is checked on the GPU"
    return Harness()


@gpu
@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("nofuse", [False, True])
def test_the_concealing_call_only_enqueues(nofuse, pcm16, harness, monkeypatch):
    """decode_packed with `lost` keeps to its stream and does not wait for the device: `lost` (and data and index) produced
    behind a delay on the call's stream, and the call on a side stream while the default stream sleeps (tests/stream_order.py);
    the one launch and the composition."""
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, x = _encoded(N0, 2, B=4, K=20, seed=8, nan=False)
    data, index = codec.encode_packed(_dev(x))
    lost = _dev((np.random.default_rng(2).random((4, 21, 2)) < 0.3).astype(np.uint8))
    ref0 = _composition(codec, data, index, pcm16, lost, 8)
    if nofuse:
        monkeypatch.setenv(NOFUSE, "1")
    assert codec.decode_packed_launches(2) == (1 + codec.decode_quantized_launches(2) if nofuse else 1)
    case = ((data, index, lost), lambda data, index, lost: codec.decode_packed(data, index, pcm16, lost=lost, max_age=8))
    name = "decode_packed[lost,%s,%s]" % ("pcm16" if pcm16 else "f32", "composition" if nofuse else "one launch")
    ref = harness.reference(case)
    assert same_bits(ref[0], ref0)
    harness.delayed_producer(name, case, ref)
    harness.busy_default(name, case, ref)


@gpu
def test_errors(monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, data, index, _, _ = _signal(2, 7)
    lost = torch.zeros((3, 7, 2), dtype=torch.uint8, device="cuda")
    ref = codec.decode_packed(data, index)
    for nofuse in (False, True):
        if nofuse:
            monkeypatch.setenv(NOFUSE, "1")
        for bad in (-1, 32):
            with pytest.raises(ValueError, match="max_age"):
                codec.decode_packed(data, index, lost=lost, max_age=bad)
        with pytest.raises(TypeError, match="max_age"):
            codec.decode_packed(data, index, lost=lost, max_age=2.0)
        for shape in ((3, 6, 2), (3, 7, 1), (3, 7, 2, 1), (42,)):
            with pytest.raises(ValueError, match="lost"):
                codec.decode_packed(data, index, lost=torch.zeros(shape, dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError, match="lost lives on cpu"):
            codec.decode_packed(data, index, lost=lost.cpu())
        with pytest.raises(ValueError, match="lost has dtype"):
            codec.decode_packed(data, index, lost=lost.to(torch.int32))
        with pytest.raises(TypeError, match="lost"):
            codec.decode_packed(data, index, lost=[0] * 42)
        assert same_bits(codec.decode_packed(data, index, lost=lost), ref)      # nothing faulted, nothing is left behind
    monkeypatch.delenv(NOFUSE)
    # the C ABI: max_age out of range is AC_EINVAL, a NULL lost is no loss, the switch sends the call to AC_EUNSUPPORTED
    lib = _lib.load()
    dev = data.device
    out = torch.zeros_like(ref)
    rows = _lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr())
    plans = (codec.mdct._plan(dev), codec.psy._plan(dev))

    def call(conceal):
        return lib.ac_decode_quantized(*plans, ctypes.addressof(rows), None, ctypes.c_void_p(out.data_ptr()), None,
                                       ctypes.addressof(conceal), 3, 7, 2, None)
    for bad in (-1, 32):
        assert call(_lib.Conceal(lost.data_ptr(), bad)) == _lib.AC_EINVAL and b"max_age" in lib.ac_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
    assert call(_lib.Conceal(None, 8)) == 0
    torch.cuda.synchronize()
    assert same_bits(out, ref)
    monkeypatch.setenv(NOFUSE, "1")
    assert call(_lib.Conceal(lost.data_ptr(), 8)) == _lib.AC_EUNSUPPORTED and b"ac_unpack" in lib.ac_last_error()
