"""decode_packed() in one launch: the synthesis that reads the packed bitstream itself (k_inv_fast_p).

The oracle is always the composition on the same tensors, ``decode_quantized(*psy.unpack(data, index), pcm16)`` -- existing
code, which tests/test_pack.py holds to the numpy restatement of the format -- and every comparison is bit for bit (NaN
payloads included), for float32 and 16-bit PCM outputs.
"""

import ctypes
import os

import numpy as np
import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib
from conftest import ROOT
from pack_reference import np_pack, np_row_bits, np_widths
from stream_order import Harness, same_bits
from test_pack import _encoded, _set_field, designed, np_row_bits_from_header


# ---- CPU -----------------------------------------------------------------------------------------------------------
def test_library_exports_the_packed_decode():
    lib = _lib.load()
    assert "ac_decode_packed_launches" in _lib.PROTOTYPES and hasattr(lib, "ac_decode_packed_launches")
    assert lib.ac_decode_packed_launches(None, None, 2) == 0
    assert lib.ac_version() == 171


def test_header_declares_the_packed_rows():
    text = open(os.path.join(ROOT, "include", "audiocodec_amd.h")).read()
    assert "typedef struct ac_packed_rows" in text and "} ac_packed_rows;" in text
    body = text[text.index("typedef struct ac_packed_rows"):text.index("} ac_packed_rows;")]
    for field in ("const uint8_t* data;", "int64_t nbytes;", "const int64_t* index;"):
        assert field in body, field
    assert "AC_API int ac_decode_packed_launches(const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C);" in text
    # the ctypes mirror has the header's layout
    assert [n for n, _ in _lib.PackedRows._fields_] == ["data", "nbytes", "index"] and ctypes.sizeof(_lib.PackedRows) == 24


def test_codec_has_decode_packed_launches():
    assert callable(audiocodec_amd.AudioCodec.decode_packed_launches)


# ---- GPU -----------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
NOFUSE = "AC_DECODE_PACKED_NOFUSE"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _hold_to_composition(codec, data, index, fused=True):
    """decode_packed against unpack + decode_quantized on the same tensors, both PCM formats; returns the float32 PCM."""
    C = index.shape[2]
    assert codec.decode_packed_launches(C) == (1 if fused else 1 + codec.decode_quantized_launches(C))
    codes, sf = codec.psy.unpack(data, index)
    out = None
    for pcm16 in (False, True):
        ref = codec.decode_quantized(codes, sf, pcm16=pcm16)
        got = codec.decode_packed(data, index, pcm16=pcm16)
        assert got.dtype == (torch.int16 if pcm16 else torch.float32)
        assert same_bits(got, ref), "pcm16=%s: %d elements differ" % (
            pcm16, int((got.view(torch.int16 if pcm16 else torch.int32) != ref.view(torch.int16 if pcm16 else torch.int32)).sum()))
        out = got if not pcm16 else out
    return out


@gpu
def test_launch_table(monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    plans = [(1024, 64, 1, True), (1024, 64, 2, True), (1024, 64, 3, False), (960, 64, 2, False), (2048, 64, 2, False),
             (1024, 32, 2, False)]
    codecs = {}
    for N, M, C, fused in plans:
        codec = codecs.setdefault((N, M), audiocodec_amd.AudioCodec(48000, N, bark_bands_n=M))
        assert codec.decode_packed_launches(C) == (1 if fused else 1 + codec.decode_quantized_launches(C)), (N, M, C)
    # the switch, read per call: the composition everywhere, the same results
    codec, x = _encoded(1024, 2, B=2, K=3, seed=1)
    data, index = codec.encode_packed(_dev(x))
    fused = [codec.decode_packed(data, index, pcm16=p) for p in (False, True)]
    monkeypatch.setenv(NOFUSE, "1")
    for N, M, C, _ in plans:
        assert codecs[(N, M)].decode_packed_launches(C) == 1 + codecs[(N, M)].decode_quantized_launches(C), (N, M, C)
    unfused = [codec.decode_packed(data, index, pcm16=p) for p in (False, True)]
    _hold_to_composition(codec, data, index, fused=False)
    monkeypatch.delenv(NOFUSE)
    assert codec.decode_packed_launches(2) == 1
    for a, b in zip(fused, unfused):
        assert same_bits(a, b)


@gpu
@pytest.mark.parametrize("bitrate", [None, 64000])
@pytest.mark.parametrize("C,B,K", [(1, 3, 7), (2, 3, 7), (1, 3, 0), (2, 2, 0), (1, 3, 1), (2, 2, 1)])
def test_encoded_signals(C, B, K, bitrate, monkeypatch):
    """Seeded noise with a rising envelope and one NaN sample (sf = -128 bands); C = 1 with B = 3: the last pair has no
    second signal; K = 0 and K = 1: the shortest clips (one and two frames)."""
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, x = _encoded(1024, C, B=B, K=max(K, 1), seed=4 + K, nan=K > 0)
    if K == 0:
        x = x[:, :0]
    if bitrate:
        codec = codec.with_bitrate(bitrate)
    data, index = codec.encode_packed(_dev(x))
    assert tuple(index.shape) == (B, K + 1, C)
    if K > 0:
        assert (codec.psy.unpack(data, index)[1] == -128).any()
    _hold_to_composition(codec, data, index)


def _designed_rows(C, sample_rate=48000):
    """Rows of every width 0..16 and 31 with the extreme codes, rows of the least and of the greatest length between them."""
    psy = audiocodec_amd.PsychoacousticModel(sample_rate, filter_bands_n=1024, bark_bands_n=64)
    off = psy.scale_band_offsets
    B, F = 5, 40
    codes, sf = designed(np.random.default_rng(17 + C), off, B, F, C)
    codes[:, 2::5] = 0            # the least length: every band of width 0 ...
    sf[:, 2::5] = 5               # (... whatever sf says, unless it says -128)
    codes[:, 3::5] = -32768       # the greatest: every band at 16 bits
    sf[:, 3::5] = 3
    codes[0, 3, ::2] = 32767
    codes[0, 3, 1::4] = -32767
    return psy, off, codes, sf


@gpu
@pytest.mark.parametrize("C", [1, 2])
def test_designed_rows(C, monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    psy, off, codes, sf = _designed_rows(C)
    w = np_widths(codes, sf, off)
    L = np.diff(off)
    assert set(np.unique(w[..., L > 0, :]).tolist()) == set(range(17)) | {31}
    assert (codes == -32768).any() and (codes == 32767).any() and (codes == -32767).any()
    bits = np_row_bits(codes, sf, off)
    assert bits.min() == 5 * 64 and bits.max() == 16 * 1024 + 13 * int((L > 0).sum())
    assert (L > 0).all() and bits.max() == 17216
    _, index_np = np_pack(codes, sf, off)
    assert set((index_np.reshape(-1) % 128).tolist()) == set(range(0, 128, 4)), "row starts at every 4-byte phase of a line"
    codec = audiocodec_amd.AudioCodec(48000, 1024)
    data, index = psy.pack(_dev(codes), _dev(sf))
    assert np.array_equal(index.cpu().numpy(), index_np)
    out = _hold_to_composition(codec, data, index)
    assert torch.isnan(out).any() and torch.isfinite(out).any()


@gpu
@pytest.mark.parametrize("C,B,K", [(2, 64, 64), (1, 129, 96)])
def test_production_strip_length(C, B, K, monkeypatch):
    """Enough strips (>= 2 x 4 waves x 256 CUs) for the strips of 2 (stereo) and 3 (mono) blocks of the bench workload: the
    hand-over between the waves of a workgroup and the extra DCT-IV of its first wave; an odd signal count in mono."""
    monkeypatch.delenv(NOFUSE, raising=False)
    codec = audiocodec_amd.AudioCodec(48000, 1024)
    g = torch.Generator("cuda").manual_seed(B + K)
    x = (torch.rand((B, K * 1024, C), device="cuda", generator=g) * 2 - 1) * torch.linspace(0.01, 1, K * 1024, device="cuda")[None, :, None]
    data, index = codec.encode_packed(x)
    pairs = B if C == 2 else (B + 1) // 2
    assert pairs * ((K + 2 + (3 - C)) // (4 - C)) >= 2048
    _hold_to_composition(codec, data, index)


@gpu
def test_random_access(monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, x = _encoded(1024, 2, B=2, K=8, seed=6)
    data, index = codec.encode_packed(_dev(x))
    for view in (index[:, 3:7], index[..., [1, 0]], index[:, 1:8:3], index[:, 3:7, :1], index[:, 1:8:3, 1:]):
        _hold_to_composition(codec, data, view)
    assert not index[:, 1:8:3].is_contiguous()
    whole = codec.decode_packed(data, index)
    swapped = codec.decode_packed(data, index[..., [1, 0]])
    assert same_bits(swapped, whole[..., [1, 0]].contiguous())


@gpu
@pytest.mark.parametrize("trim", [0, 3])
def test_damaged_input(trim, monkeypatch):
    """data is a view big[:n] of an allocation whose tail holds 0xFF (test_pack.test_unpack_clamps_to_the_buffer): a last row
    whose header claims more than n leaves, width fields of 17 and 29, and row starts at n, far past it, before 0, two bytes
    before the end and off the 4-byte phase -- inputs the format defines a result for."""
    monkeypatch.delenv(NOFUSE, raising=False)
    codec = audiocodec_amd.AudioCodec(48000, 1024)
    off = codec.psy.scale_band_offsets
    rng = np.random.default_rng(11 + trim)
    codes = rng.integers(-2, 3, (2, 3, 1024, 2)).astype(np.int16)
    sf = rng.integers(-20, 20, (2, 3, 64, 2)).astype(np.int8)
    data, index = np_pack(codes, sf, off)
    data = data.copy()
    idx = index.reshape(-1)
    for j in (50, 60, 63):                     # the last row: its widest bands at 16 bits
        _set_field(data, int(idx[-1]) * 8 + 5 * j, 16, 5)
    _set_field(data, int(idx[2]) * 8 + 5 * 7, 17, 5)     # damaged width fields
    _set_field(data, int(idx[3]) * 8 + 5 * 9, 29, 5)
    n = len(data) - trim
    need = int(idx[-1]) + int(np.ceil(np_row_bits_from_header(data, int(idx[-1]), off) / 8))
    assert need > n
    big = torch.full((n + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    big[:n] = _dev(data[:n])
    odd = index[:1].copy()
    odd.reshape(-1)[:] = [n, n + 10 ** 6, -8, n - 2, int(idx[5]) + 1, int(idx[6]) + 2]
    every = np.concatenate([index, odd])       # [3, 3, 2]
    out = _hold_to_composition(codec, big[:n], _dev(every))
    assert torch.isnan(out[0]).any()           # (the bands of width 17 / 29)
    _hold_to_composition(codec, big[:n], _dev(every.reshape(6, 3, 1)))
    _hold_to_composition(codec, big[:n], _dev(every.reshape(6, 3, 1)[:5]))   # an odd signal count


@pytest.fixture(scope="module")
def harness():
    assert torch.cuda.is_available(), "the stream contract is checked on the GPU"
    return Harness()


@gpu
@pytest.mark.parametrize("pcm16", [False, True])
def test_stream_contract_of_the_fused_route(pcm16, harness, monkeypatch):
    """decode_packed at (1024, 2) keeps to its stream: its inputs produced behind a delay on the call's stream, and the
    call on a side stream while the default stream sleeps (tests/stream_order.py)."""
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, x = _encoded(1024, 2, B=4, K=20, seed=8, nan=False)
    data, index = codec.encode_packed(_dev(x))
    assert codec.decode_packed_launches(2) == 1
    case = ((data, index), lambda data, index: codec.decode_packed(data, index, pcm16=pcm16))
    name = "decode_packed[%s]" % ("pcm16" if pcm16 else "f32")
    ref = harness.reference(case)
    assert same_bits(ref[0], codec.decode_quantized(*codec.psy.unpack(data, index), pcm16=pcm16))
    harness.delayed_producer(name, case, ref)
    harness.busy_default(name, case, ref)


@gpu
def test_c_abi_without_a_fused_kernel(monkeypatch):
    """sf == NULL where no kernel reads packed rows: AC_EUNSUPPORTED, and the message names ac_unpack."""
    monkeypatch.delenv(NOFUSE, raising=False)
    lib = _lib.load()
    codec, x = _encoded(960, 2, B=1, K=2, nan=False)
    data, index = codec.encode_packed(_dev(x))
    dev = data.device
    assert codec.decode_packed_launches(2) == 3
    out = torch.zeros((1, 4 * 960, 2), device="cuda")
    rows = _lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr())
    mdct, psy = codec.mdct._plan(dev), codec.psy._plan(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = lib.ac_decode_quantized(mdct, psy, ctypes.addressof(rows), None, p(out), None, None, 1, 3, 2, None)
    assert st == _lib.AC_EUNSUPPORTED and b"ac_unpack" in lib.ac_last_error()
    # codes == NULL stays an error, with or without sf
    assert lib.ac_decode_quantized(mdct, psy, None, None, p(out), None, None, 1, 3, 2, None) == _lib.AC_EINVAL
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
    # ... and where the kernel serves, the switch sends the same call to AC_EUNSUPPORTED
    c2, x2 = _encoded(1024, 2, B=1, K=2, nan=False)
    d2, i2 = c2.encode_packed(_dev(x2))
    r2 = _lib.PackedRows(d2.data_ptr(), d2.numel(), i2.data_ptr())
    o2 = torch.empty((1, 4 * 1024, 2), device="cuda")
    args = (c2.mdct._plan(dev), c2.psy._plan(dev), ctypes.addressof(r2), None, p(o2), None, None, 1, 3, 2, None)
    assert lib.ac_decode_quantized(*args) == 0
    torch.cuda.synchronize()
    assert same_bits(o2, c2.decode_quantized(*c2.psy.unpack(d2, i2)))
    monkeypatch.setenv(NOFUSE, "1")
    assert lib.ac_decode_quantized(*args) == _lib.AC_EUNSUPPORTED and b"ac_unpack" in lib.ac_last_error()
