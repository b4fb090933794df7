"""Concealment of lost rows in a stream ("Streams"): ``StreamingMDCT.decode_packed_chunk(data, index,
pcm16, lost=..., max_age=...)`` carries the last row that arrived, and the frames since it, from chunk to chunk.

The definition is by frame index, so it is exact: however a signal of K' frames is split into chunks, the concatenated outputs
are blocks 0 .. K'-1 of ``decode_packed(data, index, lost=, max_age=)`` on the whole signal, bit for bit, float32 and 16-bit
PCM.  Four statements of it are held to each other:

  * the kernel k_inv_fast_pls (one launch per chunk, where ``packed_chunk_launches(decode=True, conceal=True)`` is 1);
  * the composition in torch ops with the state in tensors (``AC_DECODE_PACKED_NOFUSE=1``, and every other configuration);
  * the one-shot ``decode_packed`` with ``lost``, and ``decode_quantized`` on the numpy-concealed codes (test_conceal.py);
  * tests/stream_conceal_reference.py, the state machine in numpy, chunk by chunk: its rows dequantised and put through
    ``inverse_chunk`` of a second stream.
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
from audiocodec_amd.codec import StreamingMDCT
from conceal_reference import np_conceal, np_conceal_plan
from conftest import ROOT
from pack_reference import np_pack
from stream_conceal_reference import (CARRIED, NO_SOURCE, np_chunk_plan, np_conceal_chunk, np_fresh_gap, np_fresh_state,
                                      np_stream_plan)
from stream_order import Harness, same_bits
from test_encode_cbr import _input

N0 = 1024
NOFUSE = "AC_DECODE_PACKED_NOFUSE"
AGES = (0, 1, 8, 31)
HEADER = os.path.join(ROOT, "include", "audiocodec_amd.h")


def _bounds(splits):
    out, a = [], 0
    for k in splits:
        out.append((a, a + k))
        a += k
    return out


# ---- CPU: the state machine in numpy, on hand-written patterns ----------------------------------------------------------
def _lost(F, frames, B=1, C=1):
    lost = np.zeros((B, F, C), dtype=np.uint8)
    lost[:, list(frames)] = 1
    return lost


@pytest.mark.parametrize("max_age", [1, 3, 8, 31])
def test_run_across_a_boundary_of_max_age_and_one_more(max_age):
    """Frame 2 arrives, then a run that crosses the boundary at frame 4: its last row is max_age old, or one more."""
    F = max_age + 8
    for extra in (0, 1):
        lost = _lost(F, range(3, 3 + max_age + extra))
        src, age, gaps = np_stream_plan(lost, (4, F - 4), (max_age, max_age))
        want_src, want_age = np_conceal_plan(lost, max_age)
        assert np.array_equal(src, want_src) and np.array_equal(age, want_age)
        end = 2 + max_age + extra                       # the last row of the run
        if extra == 0:
            assert src[0, end, 0] == 2 and age[0, end, 0] == max_age
        else:
            assert src[0, end, 0] == -1 and age[0, end, 0] == 0 and src[0, end - 1, 0] == (2 if max_age > 0 else -1)
        assert gaps[0][0, 0] == 1 and gaps[1][0, 0] == 0
    # the rule itself, on one chunk: the carried row at age g + f + 1
    src, age, gap, last = np_chunk_plan(_lost(max_age + 2, range(max_age + 2)), np.array([[0]]), max_age)
    assert src[0, :, 0].tolist() == [CARRIED] * max_age + [-1, -1] and age[0, :, 0].tolist() == list(range(1, max_age + 1)) + [0, 0]
    assert gap[0, 0] == min(32, max_age + 2) and last[0, 0] == -1


@pytest.mark.parametrize("g", [0, 5, 31])
def test_a_chunk_whose_rows_are_all_lost(g):
    k = 6
    src, age, gap, last = np_chunk_plan(np.ones((1, k, 1)), np.array([[g]]), 31)
    reach = max(0, min(k, 31 - g))                     # rows with g + f + 1 <= 31
    assert src[0, :, 0].tolist() == [CARRIED] * reach + [-1] * (k - reach)
    assert age[0, :, 0].tolist() == [g + f + 1 for f in range(reach)] + [0] * (k - reach)
    assert gap[0, 0] == min(32, g + k) and last[0, 0] == -1
    src, age, _, _ = np_chunk_plan(np.ones((1, k, 1)), np.array([[g]]), 8)
    assert src[0, :, 0].tolist() == [CARRIED if g + f + 1 <= 8 else -1 for f in range(k)]


def test_the_gap_saturates_at_32():
    assert NO_SOURCE == 32
    _, _, gap, _ = np_chunk_plan(np.ones((1, 40, 1)), np.array([[0]]), 31)
    assert gap[0, 0] == 32
    gap = np.array([[0]])
    seen = []
    for _ in range(4):
        src, _, gap, _ = np_chunk_plan(np.ones((1, 8, 1)), gap, 31)
        seen.append(int(gap[0, 0]))
    assert seen == [8, 16, 24, 32] and src[0, :, 0].tolist() == [CARRIED] * 7 + [-1]   # ages 25 .. 31, then out of reach
    src, _, gap, _ = np_chunk_plan(np.ones((1, 3, 1)), gap, 31)                           # 32 stays 32: nothing to read
    assert gap[0, 0] == 32 and (src == -1).all()
    # a row that arrived early in a long chunk is out of reach at its end
    _, _, gap, last = np_chunk_plan(_lost(40, range(3, 40)), np_fresh_gap(1, 1), 31)
    assert last[0, 0] == 2 and gap[0, 0] == 32
    _, _, gap, _ = np_chunk_plan(_lost(40, range(9, 40)), np_fresh_gap(1, 1), 31)
    assert gap[0, 0] == 31


def test_frame_0_of_a_fresh_stream_lost_and_max_age_0():
    src, age, gaps = np_stream_plan(_lost(5, [0, 1]), (2, 3), (8, 8))
    assert src[0, :, 0].tolist() == [-1, -1, 2, 3, 4] and not age.any() and gaps[0][0, 0] == 32 and gaps[1][0, 0] == 0
    lost = _lost(12, [3, 4, 5, 10])
    src, age, _ = np_stream_plan(lost, (5, 7), (0, 0))
    assert np.array_equal(src[0, :, 0], np.where(lost[0, :, 0] != 0, -1, np.arange(12))) and not age.any()


def test_a_different_max_age_per_chunk():
    """Each row takes the max_age of its own call; the state does not depend on it."""
    lost = _lost(12, range(2, 11))                       # frames 0, 1 and 11 arrive
    src, age, gaps = np_stream_plan(lost, (4, 4, 4), (1, 8, 3))
    assert src[0, :, 0].tolist() == [0, 1, 1, -1, 1, 1, 1, 1, -1, -1, -1, 11]
    assert age[0, :, 0].tolist() == [0, 0, 1, 0, 3, 4, 5, 6, 0, 0, 0, 0]
    assert [int(g[0, 0]) for g in gaps] == [2, 6, 0]
    assert [int(g[0, 0]) for g in np_stream_plan(lost, (4, 4, 4), (31, 0, 31))[2]] == [2, 6, 0]


def test_clips_and_channels_are_independent():
    lost = np.zeros((2, 6, 2), dtype=np.uint8)
    lost[0, 2:, 0] = 1         # (0, 0): carried across the boundary at 3
    lost[1, :3, 1] = 1         # (1, 1): nothing arrives in chunk 1
    src, age, gaps = np_stream_plan(lost, (3, 3), (8, 8))
    assert src[0, :, 0].tolist() == [0, 1, 1, 1, 1, 1] and age[0, :, 0].tolist() == [0, 0, 1, 2, 3, 4]
    assert src[1, :, 1].tolist() == [-1, -1, -1, 3, 4, 5] and src[0, :, 1].tolist() == list(range(6))
    assert gaps[0].tolist() == [[1, 0], [0, 32]] and gaps[1].tolist() == [[4, 0], [0, 0]]


@pytest.mark.parametrize("seed", range(6))
def test_random_patterns_chunked_equal_the_one_shot_plan(seed):
    rng = np.random.default_rng(seed)
    B, C, F = 2, 2, int(rng.integers(20, 70))
    lost = (rng.random((B, F, C)) < rng.choice([0.3, 0.7, 0.95])).astype(np.uint8)
    for max_age in AGES + (5,):
        want = np_conceal_plan(lost, max_age)
        for _ in range(4):
            cuts = np.sort(rng.choice(np.arange(1, F), size=int(rng.integers(0, 6)), replace=False))
            splits = tuple(int(v) for v in np.diff(np.concatenate(([0], cuts, [F]))))
            src, age, _ = np_stream_plan(lost, splits, (max_age,) * len(splits))
            assert np.array_equal(src, want[0]) and np.array_equal(age, want[1]), (max_age, splits)


def test_np_conceal_chunk_moves_rows_and_state():
    rng = np.random.default_rng(1)
    codes = rng.integers(-9, 10, (1, 3, 8, 2)).astype(np.int16)
    sf = rng.integers(-20, 20, (1, 3, 4, 2)).astype(np.int8)
    lost = np.zeros((1, 3, 2), dtype=np.uint8)
    lost[0, 1:, 0] = 1
    c2, s2, state = np_conceal_chunk(codes, sf, lost, np_fresh_state(1, 8, 4, 2), 8)
    assert np.array_equal(c2[0, 2, :, 0], codes[0, 0, :, 0]) and np.array_equal(s2[0, 2, :, 0], np.maximum(sf[0, 0, :, 0] - 8, -127))
    assert np.array_equal(state[0][0, :, 0], codes[0, 0, :, 0]) and np.array_equal(state[0][0, :, 1], codes[0, 2, :, 1])
    assert state[2].tolist() == [[2, 0]]
    c3, s3, state = np_conceal_chunk(codes, sf, np.ones((1, 3, 2), dtype=np.uint8), state, 4)
    assert np.array_equal(c3[0, 1, :, 0], codes[0, 0, :, 0]) and np.array_equal(s3[0, 1, :, 0], np.maximum(sf[0, 0, :, 0] - 16, -127))
    assert not c3[0, 2, :, 0].any() and not s3[0, 2, :, 0].any()            # age 5 > 4: muted
    assert np.array_equal(c3[0, 0, :, 1], codes[0, 2, :, 1]) and state[2].tolist() == [[5, 3]]


# ---- CPU: the ABI surface ---------------------------------------------------------------------------------------------
def test_abi_has_the_flag_the_struct_and_the_keyword_arguments():
    text = open(HEADER).read()
    assert re.search(r"\benum\s*\{\s*AC_CONCEAL\s*=\s*128\s*\}", text) and _lib.AC_CONCEAL == 128
    assert _lib.AC_PACKED | _lib.AC_CONCEAL == 144
    m = re.search(r"typedef\s+struct\s+ac_stream_packed_lost_in\s*\{(.*?)\}\s*ac_stream_packed_lost_in\s*;", text, flags=re.S)
    assert m, "ac_stream_packed_lost_in is not declared"
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    assert [" ".join(f.split()) for f in body.split(";") if f.strip()] == ["ac_stream_packed_in in", "const uint8_t* lost", "int32_t max_age"]
    P = _lib.StreamPackedLostIn
    assert [f[0] for f in P._fields_] == ["inner", "lost", "max_age"]
    assert (P.inner.offset, P.lost.offset, P.max_age.offset) == (0, 40, 48) and ctypes.sizeof(P) == 56
    assert P.inner.size == ctypes.sizeof(_lib.StreamPackedIn) == 40 and P.lost.size == 8 and P.max_age.size == 4
    assert re.search(r"#define\s+AC_VERSION\s+171\b", text) and "do not conceal yet" not in open(os.path.join(ROOT, "README.md")).read()
    sig = inspect.signature(StreamingMDCT.decode_packed_chunk)
    assert list(sig.parameters)[:6] == ["self", "data", "index", "pcm16", "out", "stream"]
    for name, default in (("lost", None), ("max_age", 8)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default
    sig = inspect.signature(StreamingMDCT.packed_chunk_launches)
    assert sig.parameters["conceal"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["conceal"].default is False


def test_library_keeps_its_version_and_rejects_null_arguments():
    lib = _lib.load()
    assert lib.ac_version() == 171
    assert lib.ac_stream_packed_launches(None, None, 2) == 0
    dtype = _lib.AC_PACKED | _lib.AC_CONCEAL
    assert lib.ac_stream_inverse_typed(None, None, None, dtype, 1, None) == _lib.AC_EINVAL
    assert b"stream is NULL" in lib.ac_last_error()
    rows = _lib.StreamPackedLostIn()
    assert lib.ac_stream_inverse_typed(None, ctypes.addressof(rows), None, dtype, 0, None) == _lib.AC_EINVAL
    # the flag alone, or beside anything but AC_PACKED, is no format
    for bad in (_lib.AC_CONCEAL, _lib.AC_CONCEAL | 1):
        assert lib.ac_stream_inverse_typed(None, None, None, bad, 1, None) == _lib.AC_EINVAL
        assert b"dtype" in lib.ac_last_error()
    assert lib.ac_stream_encode_typed(None, None, None, None, None, None, 0.0, dtype, 1, None) == _lib.AC_EINVAL


# ---- GPU ------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _cbr(N=N0):
    return audiocodec_amd.AudioCodec(48000, N).with_bitrate(64000)


@functools.lru_cache(maxsize=None)
def _signal(C, Kp, B=3):
    """Rows of encode_packed_rows at 64 kbit/s, [B, Kp, C] (with the large samples of test_encode_cbr: non-finite bands and a
    marked row among them), and what psy.unpack reads of them."""
    cbr = _cbr()
    data, index, fits = cbr.encode_packed_rows(_input(C, B, Kp - 1, 7 * Kp + C, True))
    assert tuple(index.shape) == (B, Kp, C) and not bool(fits.all())
    codes, sf = (t.cpu().numpy() for t in cbr.psy.unpack(data, index))
    assert (sf == -128).any()
    return cbr, data, index, codes, sf


def _pcm_store(x):
    """AudioCodec.decode's 16-bit store: 0 if NaN else clamp(rint(fp32(32768 x)), -32768, 32767)."""
    return torch.nan_to_num(x * 32768.0, nan=0.0).round().clamp(-32768.0, 32767.0).to(torch.int16)


def _chunks(st, data, index, lost, splits, ages, pcm16, conceal=True):
    """The chunk calls of one split on stream object `st`; pcm16 and ages: one value, or one per chunk."""
    n = len(splits)
    ages = (ages,) * n if isinstance(ages, int) else ages
    pcm16 = (pcm16,) * n if isinstance(pcm16, bool) else pcm16
    outs = []
    for (a, b), m, p in zip(_bounds(splits), ages, pcm16):
        kw = dict(lost=lost[:, a:b].contiguous(), max_age=m) if conceal else {}
        outs.append(st.decode_packed_chunk(data, index[:, a:b].contiguous(), pcm16=p, **kw))
        assert outs[-1].dtype == (torch.int16 if p else torch.float32)
        assert outs[-1].shape == (index.shape[0], (b - a) * st.mdct.filters_n, index.shape[2])
    return outs


class _composed:
    """AC_DECODE_PACKED_NOFUSE=1 around a block (the library reads it per call); what was there before comes back."""

    def __enter__(self):
        self.before = os.environ.get(NOFUSE)
        os.environ[NOFUSE] = "1"

    def __exit__(self, *exc):
        if self.before is None:
            del os.environ[NOFUSE]
        else:
            os.environ[NOFUSE] = self.before
        return False


def _numpy_chunks(codec, st, calls):
    """tests/stream_conceal_reference.py chunk by chunk: calls = [(data, index, lost (numpy), max_age, pcm16)]; the carried
    row is what psy.unpack reads of the call that saw it.  `st`: a stream of its own, for inverse_chunk."""
    B, _, C = calls[0][1].shape
    state = np_fresh_state(B, codec.psy.filter_bands_n, codec.psy.bark_bands_n, C)
    outs = []
    for data, index, lost, max_age, pcm16 in calls:
        codes, sf = (t.cpu().numpy() for t in codec.psy.unpack(data, index.contiguous()))
        c2, s2, state = np_conceal_chunk(codes, sf, lost, state, max_age)
        x = st.inverse_chunk(codec.psy.dequantize(_dev(c2), _dev(s2)))
        outs.append(_pcm_store(x) if pcm16 else x)
    return outs, state


def _patterns(B, Kp, C, max_age, splits):
    """Loss patterns [B, Kp, C] for one split; clips and channels take different boundaries where there are several."""
    rng = np.random.default_rng(1000 * Kp + 10 * max_age + C + len(splits))
    cuts = [a for a, _ in _bounds(splits)[1:]] or [Kp // 2]      # (one chunk: any frame serves as the "boundary")
    z = lambda: np.zeros((B, Kp, C), dtype=np.uint8)             # noqa: E731
    out = {"none": z(), "all": np.ones((B, Kp, C), dtype=np.uint8), "30 %": (rng.random((B, Kp, C)) < 0.3).astype(np.uint8)}
    ends = z()
    for p in cuts:                                               # a run of two ending exactly at every boundary
        ends[:, max(p - 2, 0):p] = 1
    out["runs ending at the boundaries"] = ends
    for name, back, n in (("from frame 0 of a chunk, max_age", 0, max_age), ("from frame 0 of a chunk, max_age + 1", 0, max_age + 1),
                          ("across the boundary, max_age", 1, max_age), ("across the boundary, max_age + 1", 1, max_age + 1)):
        runs = z()
        for b in range(B):
            for c in range(C):
                p = cuts[(b + c) % len(cuts)] - back
                runs[b, max(p, 0):max(p, 0) + n, c] = 1
        out["a run " + name] = runs
    if len(splits) >= 3:                                         # an entire chunk lost between two good ones
        whole = z()
        a, b = _bounds(splits)[len(splits) // 2]
        whole[:, a:b] = 1
        out["a whole chunk"] = whole
    return out


@functools.lru_cache(maxsize=None)
def _references(C, Kp, max_age, name, splits_key, pcm16):
    """Blocks [0, Kp) of the one-shot decode_packed with `lost`, checked once against decode_quantized of the numpy-concealed
    codes.  (splits_key names the split the pattern was made for.)"""
    cbr, data, index, codes, sf = _signal(C, Kp)
    lost = _patterns(3, Kp, C, max_age, splits_key)[name]
    one = cbr.decode_packed(data, index, pcm16, lost=_dev(lost), max_age=max_age)
    c2, s2 = np_conceal(codes, sf, lost, max_age)
    assert same_bits(one, cbr.decode_quantized(_dev(c2), _dev(s2), pcm16=pcm16)), (name, max_age, pcm16)
    return one[:, :Kp * N0].contiguous()


SPLITS = [(12, (12,)), (12, (1,) * 12), (12, (5, 7)), (12, (2, 3, 7)), (45, (40, 5)), (45, (3, 40, 2))]


@gpu
@pytest.mark.parametrize("Kp,splits", SPLITS, ids=["-".join(map(str, s)) if len(s) < 12 else "1x12" for _, s in SPLITS])
@pytest.mark.parametrize("C", [1, 2])
def test_chunked_equals_one_shot(C, Kp, splits, monkeypatch):
    """B = 3 (mono: the last pair has no second signal).  Every pattern at every max_age, float32 and 16-bit PCM: the kernel's
    chunks against the one-shot call on the whole signal, against the composition on a second stream, and (through the
    one-shot call) against decode_quantized of the numpy-concealed codes."""
    monkeypatch.delenv(NOFUSE, raising=False)
    cbr, data, index, codes, sf = _signal(C, Kp)
    fused, comp = cbr.stream(3, C), cbr.stream(3, C)
    assert fused.packed_chunk_launches(decode=True, conceal=True) == 1
    for max_age in AGES:
        for name, lost in _patterns(3, Kp, C, max_age, splits).items():
            src, age, _ = np_stream_plan(lost, splits, (max_age,) * len(splits))       # the numpy state machine on this split
            want = np_conceal_plan(lost, max_age)
            assert np.array_equal(src, want[0]) and np.array_equal(age, want[1]), (name, max_age)
            lost_d = _dev(lost)
            for pcm16 in (False, True):
                ref = _references(C, Kp, max_age, name, splits, pcm16)
                fused.reset()
                got = torch.cat(_chunks(fused, data, index, lost_d, splits, max_age, pcm16), dim=1)
                assert same_bits(got, ref), "kernel != one-shot: %s max_age=%d pcm16=%s" % (name, max_age, pcm16)
                comp.reset()
                with _composed():
                    assert comp.packed_chunk_launches(decode=True, conceal=True) == 3
                    other = torch.cat(_chunks(comp, data, index, lost_d, splits, max_age, pcm16), dim=1)
                assert same_bits(other, ref), "composition != one-shot: %s max_age=%d pcm16=%s" % (name, max_age, pcm16)
                if name == "all":      # +0 everywhere: not -0, not NaN
                    assert int((got.view(torch.int16 if pcm16 else torch.int32) != 0).sum()) == 0


@gpu
@pytest.mark.parametrize("C", [1, 2])
def test_a_different_max_age_and_output_per_chunk(C, monkeypatch):
    """Each row takes the max_age of its own call, and int16 and float32 outputs may alternate: against the numpy state
    machine chunk by chunk, and the composition."""
    monkeypatch.delenv(NOFUSE, raising=False)
    cbr, data, index, _, _ = _signal(C, 12)
    splits, ages, pcm = (2, 3, 3, 4), (1, 8, 0, 31), (False, True, True, False)
    lost = np.zeros((3, 12, C), dtype=np.uint8)
    lost[:, 1:11] = 1
    lost[1, 6, C - 1] = 0
    lost_d = _dev(lost)
    fused, comp, plain = cbr.stream(3, C), cbr.stream(3, C), cbr.stream(3, C)
    got = _chunks(fused, data, index, lost_d, splits, ages, pcm)
    with _composed():
        other = _chunks(comp, data, index, lost_d, splits, ages, pcm)
    want, _ = _numpy_chunks(cbr, plain, [(data, index[:, a:b], lost[:, a:b], m, p) for (a, b), m, p in zip(_bounds(splits), ages, pcm)])
    for i, (g, o, w) in enumerate(zip(got, other, want)):
        assert same_bits(g, w), "kernel != numpy, chunk %d" % i
        assert same_bits(o, w), "composition != numpy, chunk %d" % i
    # max_age 8 conceals; max_age 0 mutes (clip 0, after the block that still holds the tail of the frame before)
    assert int((got[1] != 0).sum()) > 0 and int((got[2][0, N0:] != 0).sum()) == 0


@gpu
@pytest.mark.parametrize("C,B,Kp", [(2, 64, 64), (1, 129, 96)])
def test_production_strip_length(C, B, Kp, monkeypatch):
    """The shapes of test_conceal.py::test_production_strip_length as two chunks (13, Kp - 13): the wave that writes the state
    owns a strip of 2 (stereo) or 3 (mono) blocks, and the carried row is read by waves of other workgroups."""
    monkeypatch.delenv(NOFUSE, raising=False)
    cbr = _cbr()
    g = torch.Generator("cuda").manual_seed(B + Kp)
    K = Kp - 1
    x = (torch.rand((B, K * N0, C), device="cuda", generator=g) * 2 - 1) * torch.linspace(0.01, 1, K * N0, device="cuda")[None, :, None]
    data, index, _ = cbr.encode_packed_rows(x)
    assert tuple(index.shape) == (B, Kp, C)
    lost = torch.rand((B, Kp, C), device="cuda", generator=g) < 0.3
    lost[0, 5:40] = True
    lost[1, 11:20] = True
    lost[2, 13:30] = True
    st = cbr.stream(B, C)
    for max_age in (8, 31):
        for pcm16 in (False, True):
            st.reset()
            got = torch.cat(_chunks(st, data, index, lost.view(torch.uint8), (13, Kp - 13), max_age, pcm16), dim=1)
            ref = cbr.decode_packed(data, index, pcm16, lost=lost, max_age=max_age)[:, :Kp * N0]
            assert same_bits(got, ref), (max_age, pcm16)


def _two_chunks(codec, first, second, lost2, max_age=8, what=""):
    """Chunk 1 = (data, index) with nothing lost, chunk 2 = (data, index) with lost2: the kernel, the composition and the numpy
    state machine (the carried row being psy.unpack of chunk 1's own data and index).  Returns the kernel's float32 chunk 2."""
    B, _, C = first[1].shape
    lost1 = np.zeros(tuple(first[1].shape), dtype=np.uint8)
    out = None
    for pcm16 in (False, True):
        fused, comp, plain = codec.stream(B, C), codec.stream(B, C), codec.stream(B, C)
        assert fused.packed_chunk_launches(decode=True, conceal=True) == 1
        got = [fused.decode_packed_chunk(d, i, pcm16, lost=_dev(l), max_age=max_age) for (d, i), l in ((first, lost1), (second, lost2))]
        with _composed():
            other = [comp.decode_packed_chunk(d, i, pcm16, lost=_dev(l), max_age=max_age) for (d, i), l in ((first, lost1), (second, lost2))]
        want, _ = _numpy_chunks(codec, plain, [(first[0], first[1], lost1, max_age, pcm16), (second[0], second[1], lost2, max_age, pcm16)])
        for n in range(2):
            assert same_bits(other[n], want[n]), "composition != numpy: %s chunk %d pcm16=%s" % (what, n, pcm16)
            assert same_bits(got[n], want[n]), "kernel != numpy: %s chunk %d pcm16=%s" % (what, n, pcm16)
        out = got[1] if not pcm16 else out
    return out


@gpu
def test_crafted_scale_factors_and_a_marked_row_carried_across_a_boundary(monkeypatch):
    """The last good row of chunk 1 holds sf = -126 .. -120 (the clamp at -127 is met at ages 1 and 2 in chunk 2) and, in one
    signal, a band with sf = -128; or it is a marked row.  Chunk 2 starts with lost rows, and lives in another data tensor."""
    monkeypatch.delenv(NOFUSE, raising=False)
    codec = audiocodec_amd.AudioCodec(48000, N0)
    rng = np.random.default_rng(5)
    B, F, C = 2, 4, 2
    codes = rng.integers(-300, 301, (B, 2 * F, N0, C)).astype(np.int16)
    sf = rng.integers(-30, 10, (B, 2 * F, 64, C)).astype(np.int8)
    sf[:, :, 10:17] = np.arange(-126, -119, dtype=np.int8)[None, None, :, None]
    sf[:, :, 40] = -127
    sf[1, F - 1, 20, 1] = -128
    first = codec.psy.pack(_dev(codes[:, :F]), _dev(sf[:, :F]))
    second = codec.psy.pack(_dev(codes[:, F:]), _dev(sf[:, F:]))
    lost2 = np.zeros((B, F, C), dtype=np.uint8)
    lost2[:, :3] = 1
    out = _two_chunks(codec, first, second, lost2, what="crafted sf").view(B, F, N0, C)
    assert bool(torch.isnan(out[1, :, :, 1]).all()) and bool(torch.isfinite(out[:, :, :, 0]).all())
    # the carried row times 2^-age, exactly: one row alone, then lost rows in the next chunk
    one = np.zeros((1, 1, N0, 1), dtype=np.int16)
    one[0, 0] = codes[0, 0, :, :1]
    s1 = np.maximum(sf[:1, :1, :, :1], -100)
    d1, i1 = codec.psy.pack(_dev(one), _dev(s1))
    empty = torch.zeros((8,), dtype=torch.uint8, device="cuda")
    i2 = torch.full((1, 3, 1), 8, dtype=torch.int64, device="cuda")
    st = codec.stream(1, 1)
    st.decode_packed_chunk(d1, i1, lost=torch.zeros((1, 1, 1), dtype=torch.uint8, device="cuda"))
    src = st.decode_packed_chunk(empty, i2).view(3, N0)                       # the second half of the row, then silence
    assert int((src[0] != 0).sum()) > N0 // 2 and int((src[1:] != 0).sum()) == 0
    for age in (1, 2):
        st.reset()
        st.decode_packed_chunk(d1, i1, lost=torch.zeros((1, 1, 1), dtype=torch.uint8, device="cuda"))
        l2 = torch.zeros((1, 3, 1), dtype=torch.uint8, device="cuda")
        l2[0, :age] = 1
        faded = st.decode_packed_chunk(empty, i2, lost=l2, max_age=8).view(3, N0)
        assert torch.equal(faded[age], torch.ldexp(src[0], torch.tensor(-age, device="cuda"))), age
    # a marked row (every width 31) as the carried row
    cbr = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(320)
    data, index, fits = cbr.encode_packed_rows(_input(2, 3, 7, 11, True))
    marked = [tuple(int(i) for i in w) for w in torch.nonzero(~fits[:, :7])]
    assert marked and bool(fits.any())
    b, f, c = marked[0]
    lost2 = np.zeros((3, 7 - f, 2), dtype=np.uint8)
    lost2[b, :, c] = 1
    out = _two_chunks(cbr, (data, index[:, :f + 1].contiguous()), (data, index[:, f + 1:].contiguous()), lost2, what="marked row")
    assert bool(torch.isnan(out.view(3, 7 - f, N0, 2)[b, :, :, c]).all())


@gpu
@pytest.mark.parametrize("trim", [0, 3])
def test_carried_rows_at_odd_starts(trim, monkeypatch):
    """The last good row of chunk 1 is the last row of data (trimmed: off the 4-byte phase, ending at nbytes), starts before 0
    or past the end; then a permuted, strided index.  Chunk 2 lies in a buffer of 0xFF bytes apart from its own rows."""
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
    # chunk 1 [2, 3, 2]: its last row is the special one; chunk 2 [2, 3, 2] starts with lost rows
    for tails in ((last, odd, neg, past), (far, last, n - 2, odd), (int(idx[6]) + 2, neg, last, last)):
        starts = np.empty((2, 3, 2), dtype=np.int64)
        starts[:, :2] = idx[:8].reshape(2, 2, 2)
        starts[:, 2] = np.array(tails).reshape(2, 2)
        lost2 = np.zeros((2, 3, 2), dtype=np.uint8)
        lost2[:, :2] = 1
        lost2[1, 2, 0] = 1
        second = (torch.full((n + 64,), 0xFF, dtype=torch.uint8, device="cuda"), _dev(idx[8:14].reshape(2, 3, 1).repeat(2, axis=2)))
        second[0][:n] = big[:n]
        _two_chunks(codec, (big[:n], _dev(starts)), second, lost2, what="odd starts %s" % (tails,))
        _two_chunks(codec, (big[:n], _dev(starts.reshape(4, 3, 1)[:3])), (second[0], second[1].reshape(4, 3, 1)[:3].contiguous()),
                    lost2.reshape(4, 3, 1)[:3], what="odd starts, mono %s" % (tails,))
    # a permuted, strided view of index and of lost in both chunks: the same rows as the contiguous tensors
    starts = np.empty((2, 6, 2), dtype=np.int64)
    starts[:, :, 0] = [[idx[0], idx[1], last, idx[2], idx[3], idx[4]], [odd, idx[8], idx[9], idx[10], last, idx[11]]]
    starts[:, :, 1] = [[idx[6], idx[7], odd, idx[12], idx[13], last], [idx[14], neg, idx[15], idx[0], idx[1], idx[2]]]
    lost = np.zeros((2, 6, 2), dtype=np.uint8)
    lost[:, 3:5] = 1
    wide = _dev(np.ascontiguousarray(np.repeat(starts.transpose(2, 1, 0), 2, axis=1)))        # [2, 12, 2]
    view = wide.permute(2, 1, 0)[:, ::2]
    lview = _dev(np.ascontiguousarray(np.repeat(lost.transpose(2, 1, 0), 2, axis=1))).permute(2, 1, 0)[:, ::2]
    assert not view.is_contiguous() and not lview.is_contiguous() and torch.equal(view, _dev(starts))
    a, b = codec.stream(2, 2), codec.stream(2, 2)
    for pcm16 in (False, True):
        for lo, hi in ((0, 3), (3, 6)):
            got = a.decode_packed_chunk(big[:n], view[:, lo:hi], pcm16, lost=lview[:, lo:hi], max_age=8)
            ref = b.decode_packed_chunk(big[:n], _dev(starts[:, lo:hi]), pcm16, lost=_dev(lost[:, lo:hi]), max_age=8)
            assert same_bits(got, ref), (pcm16, lo)
        a.reset()
        b.reset()


@gpu
@pytest.mark.parametrize("nofuse", [False, True])
def test_state_rules(nofuse, monkeypatch):
    """reset(), a chunk without `lost` and inverse_chunk leave no source; a stream that never passes `lost` is what it was;
    `lost` all false is the plain chunk; k = 0 leaves the state alone."""
    monkeypatch.delenv(NOFUSE, raising=False)
    C, Kp = 2, 12
    cbr, data, index, codes, sf = _signal(C, Kp)
    if nofuse:
        monkeypatch.setenv(NOFUSE, "1")
    one = cbr.decode_packed(data, index)[:, :Kp * N0]
    none = torch.zeros((3, Kp, C), dtype=torch.uint8, device="cuda")
    st = cbr.stream(3, C)
    assert st.packed_chunk_launches(decode=True, conceal=True) == (3 if nofuse else 1)
    # never `lost`: the blocks of decode_packed, as before
    assert same_bits(torch.cat(_chunks(st, data, index, none, (5, 7), 8, False, conceal=False), dim=1), one)
    # `lost` all false: the same, bool or uint8
    st.reset()
    assert same_bits(torch.cat(_chunks(st, data, index, none, (5, 7), 8, False), dim=1), one)
    st.reset()
    assert same_bits(torch.cat(_chunks(st, data, index, none.bool(), (2, 3, 7), 31, False), dim=1), one)
    # what leaves no source: chunk 2 (all lost) is then silence after the overlap, block 5 = the tail of frame 4 alone
    all2 = torch.ones((3, 7, C), dtype=torch.uint8, device="cuda")
    idx1, idx2 = index[:, :5].contiguous(), index[:, 5:].contiguous()

    def second(between):
        st.reset()
        first = st.decode_packed_chunk(data, idx1, lost=none[:, :5].contiguous())
        between()
        return first, st.decode_packed_chunk(data, idx2, lost=all2, max_age=8)

    first, kept = second(lambda: None)
    want = cbr.decode_packed(data, index, lost=torch.cat((none[:, :5], all2), dim=1), max_age=8)[:, 5 * N0:Kp * N0]
    assert same_bits(first, one[:, :5 * N0]) and same_bits(kept, want) and int((kept[:, N0:2 * N0] != 0).sum()) > 0
    _, kept0 = second(lambda: st.decode_packed_chunk(data, index[:, :0].contiguous(), lost=none[:, :0].contiguous()))   # k = 0
    assert same_bits(kept0, kept)
    # ... after a reset the tail is gone too: all +0
    _, after_reset = second(st.reset)
    assert int((after_reset.view(torch.int32) != 0).sum()) == 0
    # ... a chunk without `lost`, or inverse_chunk, advances the overlap and leaves no source: the muted decode of chunk 3
    idx2a, idx2b = index[:, 5:8].contiguous(), index[:, 8:].contiguous()
    all3 = torch.ones((3, 4, C), dtype=torch.uint8, device="cuda")
    muted = cbr.decode_packed(data, index[:, :8].contiguous())[:, 8 * N0:]                 # block 8: the tail of frame 7 alone
    zeros = torch.zeros((3, 3 * N0, C), device="cuda")
    for between in (lambda: st.decode_packed_chunk(data, idx2a),
                    lambda: st.inverse_chunk(cbr.psy.dequantize(*cbr.psy.unpack(data, idx2a)))):
        st.reset()
        st.decode_packed_chunk(data, idx1, lost=none[:, :5].contiguous())
        mid = between()
        assert same_bits(mid, one[:, 5 * N0:8 * N0])
        got = st.decode_packed_chunk(data, idx2b, lost=all3, max_age=31)
        assert same_bits(got, torch.cat((muted, zeros), dim=1))
    # int16 and float32 may alternate, k = 0 in between
    st.reset()
    lost = torch.zeros((3, Kp, C), dtype=torch.uint8, device="cuda")
    lost[:, 4:9] = 1
    got = _chunks(st, data, index, lost, (5, 0, 7), 8, (True, False, False))
    ref16 = cbr.decode_packed(data, index, True, lost=lost, max_age=8)
    ref32 = cbr.decode_packed(data, index, False, lost=lost, max_age=8)
    assert same_bits(got[0], ref16[:, :5 * N0]) and got[1].shape[1] == 0 and same_bits(got[2], ref32[:, 5 * N0:Kp * N0])


@gpu
@pytest.mark.parametrize("N,C,nofuse", [(512, 3, False), (1024, 2, True)])
def test_where_the_one_launch_is_not_served(N, C, nofuse, monkeypatch):
    """filters_n = 512 with three channels, and filters_n = 1024 behind the switch: the composition, equal to the one-shot
    composition and to the numpy state machine."""
    monkeypatch.delenv(NOFUSE, raising=False)
    if nofuse:
        monkeypatch.setenv(NOFUSE, "1")
    B, Kp = 3, 12
    cbr = _cbr(N)
    data, index, _ = cbr.encode_packed_rows(_input(C, B, Kp - 1, 3, True, N=N))
    st, plain = cbr.stream(B, C), cbr.stream(B, C)
    assert st.packed_chunk_launches(decode=True, conceal=True) == 3 and cbr.decode_packed_launches(C) != 1
    for max_age in (0, 2, 31):
        for splits in ((5, 7), (2, 3, 7), (1,) * 12):
            for name, lost in _patterns(B, Kp, C, max_age, splits).items():
                st.reset()
                got = torch.cat(_chunks(st, data, index, _dev(lost), splits, max_age, False), dim=1)
                ref = cbr.decode_packed(data, index, lost=_dev(lost), max_age=max_age)[:, :Kp * N]
                assert same_bits(got, ref), (name, max_age, splits)
    lost = _patterns(B, Kp, C, 8, (5, 7))["a run across the boundary, max_age"]
    st.reset()
    got = _chunks(st, data, index, _dev(lost), (5, 7), 8, False)
    want, _ = _numpy_chunks(cbr, plain, [(data, index[:, a:b], lost[:, a:b], 8, False) for a, b in _bounds((5, 7))])
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])


@pytest.fixture(scope="module")
def harness():
    assert torch.cuda.is_available(), "the stream contract is checked on the GPU"
    return Harness()


@gpu
@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("nofuse", [False, True])
def test_the_concealing_chunk_call_only_enqueues(nofuse, pcm16, harness, monkeypatch):
    """decode_packed_chunk with `lost` keeps to its stream and does not wait for the device (tests/stream_order.py): two
    chunks after a reset, so that every run of the case starts from the same state and the second chunk reads the carried
    row; the one launch and the composition."""
    monkeypatch.delenv(NOFUSE, raising=False)
    B, C, Kp = 4, 2, 20
    cbr = _cbr()
    data, index, _ = cbr.encode_packed_rows(_input(C, B, Kp - 1, 8, False))
    lost = _dev((np.random.default_rng(2).random((B, Kp, C)) < 0.3).astype(np.uint8))
    lost[:, 9:12] = 1
    ref0 = cbr.decode_packed(data, index, pcm16, lost=lost, max_age=8)[:, :Kp * N0]
    if nofuse:
        monkeypatch.setenv(NOFUSE, "1")
    st = cbr.stream(B, C)
    assert st.packed_chunk_launches(decode=True, conceal=True) == (3 if nofuse else 1)

    def fn(data, index, lost):
        st.reset()
        a = st.decode_packed_chunk(data, index[:, :10].contiguous(), pcm16, lost=lost[:, :10].contiguous(), max_age=8)
        b = st.decode_packed_chunk(data, index[:, 10:].contiguous(), pcm16, lost=lost[:, 10:].contiguous(), max_age=8)
        return a, b
    case = ((data, index, lost), fn)
    name = "decode_packed_chunk[lost,%s,%s]" % ("pcm16" if pcm16 else "f32", "composition" if nofuse else "one launch")
    ref = harness.reference(case)
    assert same_bits(torch.cat(ref, dim=1), ref0)
    harness.delayed_producer(name, case, ref)
    harness.busy_default(name, case, ref)
    # out= and stream=: the same bits, written where the caller said
    side = harness.fresh()
    out = torch.empty_like(ref[0])
    st.reset()
    torch.cuda.synchronize()
    got = st.decode_packed_chunk(data, index[:, :10].contiguous(), pcm16, out=out, stream=side, lost=lost[:, :10].contiguous())
    side.synchronize()
    assert got is out and same_bits(out, ref[0])


@gpu
def test_errors(monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    cbr, data, index, _, _ = _signal(2, 12)
    idx = index[:, :7].contiguous()
    lost = torch.zeros((3, 7, 2), dtype=torch.uint8, device="cuda")
    ref = cbr.decode_packed(data, index)[:, :12 * N0]
    st = cbr.stream(3, 2)
    for nofuse in (False, True):
        if nofuse:
            monkeypatch.setenv(NOFUSE, "1")
        st.reset()
        for bad in (-1, 32):
            with pytest.raises(ValueError, match="max_age"):
                st.decode_packed_chunk(data, idx, lost=lost, max_age=bad)
        with pytest.raises(TypeError, match="max_age"):
            st.decode_packed_chunk(data, idx, lost=lost, max_age=2.0)
        for shape in ((3, 6, 2), (3, 7, 1), (3, 7, 2, 1), (42,)):
            with pytest.raises(ValueError, match="lost"):
                st.decode_packed_chunk(data, idx, lost=torch.zeros(shape, dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError, match="lost lives on cpu"):
            st.decode_packed_chunk(data, idx, lost=lost.cpu())
        with pytest.raises(ValueError, match="lost has dtype"):
            st.decode_packed_chunk(data, idx, lost=lost.to(torch.int32))
        with pytest.raises(TypeError, match="lost"):
            st.decode_packed_chunk(data, idx, lost=[0] * 42)
        # nothing moved: the stream still starts at block 0
        got = torch.cat((st.decode_packed_chunk(data, idx, lost=lost), st.decode_packed_chunk(data, index[:, 7:].contiguous())), dim=1)
        assert same_bits(got, ref)
    monkeypatch.delenv(NOFUSE)
    with pytest.raises(ValueError, match="decode=True"):
        st.packed_chunk_launches(conceal=True)
    # the C ABI
    lib = _lib.load()
    psy = cbr.psy._plan(data.device)
    dtype = _lib.AC_PACKED | _lib.AC_CONCEAL
    out = torch.zeros((3, 7 * N0, 2), device="cuda")

    def call(lost_ptr, max_age, pcm16=0, x=None, k=7, index_ptr=None):
        rows = _lib.StreamPackedLostIn(
            _lib.StreamPackedIn(_lib.PackedRows(data.data_ptr(), data.numel(), idx.data_ptr() if index_ptr is None else index_ptr),
                                psy.value, pcm16), lost_ptr, max_age)
        return lib.ac_stream_inverse_typed(st._handle, ctypes.addressof(rows), ctypes.c_void_p(out.data_ptr() if x is None else x),
                                           dtype, k, None)
    lost[:, 5:] = 1
    st.reset()
    first = st.decode_packed_chunk(data, idx, lost=lost, max_age=8)                   # leaves gap 2 and the tail of a faded row
    for bad in (-1, 32):
        assert call(lost.data_ptr(), bad) == _lib.AC_EINVAL and b"max_age" in lib.ac_last_error()
    assert call(None, 8) == _lib.AC_EINVAL and b"lost is NULL" in lib.ac_last_error()
    assert call(lost.data_ptr(), 8, pcm16=2) == _lib.AC_EINVAL and b"pcm16" in lib.ac_last_error()
    assert call(lost.data_ptr(), 8, x=out.data_ptr() + 4) == _lib.AC_EINVAL
    assert call(lost.data_ptr(), 8, index_ptr=idx.data_ptr() + 8) == _lib.AC_EINVAL
    assert call(None, -1, k=0) == _lib.AC_EINVAL and call(lost.data_ptr(), 8, k=0) == _lib.AC_OK
    monkeypatch.setenv(NOFUSE, "1")
    assert lib.ac_stream_packed_launches(st._handle, psy, 2) == 3
    assert call(lost.data_ptr(), 8) == _lib.AC_EUNSUPPORTED and b"ac_unpack" in lib.ac_last_error()
    monkeypatch.delenv(NOFUSE)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
    # d_tail and the concealment state are where the first chunk left them: the rest of the signal, its first rows lost
    lost2 = torch.zeros((3, 5, 2), dtype=torch.uint8, device="cuda")
    lost2[:, :3] = 1
    got = st.decode_packed_chunk(data, index[:, 7:].contiguous(), lost=lost2, max_age=8)
    whole = cbr.decode_packed(data, index, lost=torch.cat((lost, lost2), dim=1), max_age=8)
    assert same_bits(torch.cat((first, got), dim=1), whole[:, :12 * N0])
    assert int((got[:, 2 * N0:3 * N0] != 0).sum()) > 0                                  # frame 9: age 5 from frame 4, carried
