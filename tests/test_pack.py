"""The packed bitstream of quantised spectra: pack, unpack and the decoder that reads it.

tests/pack_reference.py restates the format in numpy from its rules; the kernels are checked against it byte for byte,
including damaged rows and reads that the kernels must clamp to the buffer.
"""

import ctypes

import numpy as np
import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib
from pack_reference import bit_length, np_canon, np_pack, np_row_bits, np_unpack, np_widths, unzz, zz

PLANS = [(48000, 1024, 64), (48000, 2048, 64), (44100, 1024, 64), (48000, 960, 64), (48000, 128, 64), (64, 64, 64),
         (48000, 8192, 256)]


def _offsets(sr, N, M):
    return audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M).scale_band_offsets


def designed(rng, off, B, F, C):
    """Codes whose bands have the widths 0..16 on purpose (every width in every row once M >= 17), with the extreme codes
    -32768 / 32767 in the 16-bit bands, sf = -128 bands (non-zero codes under them) and random sf everywhere else."""
    N, M = int(off[-1]), len(off) - 1
    b, f, j, c = np.meshgrid(np.arange(B), np.arange(F), np.arange(M), np.arange(C), indexing="ij")
    w = (j + 7 * c + 3 * f + 5 * b) % 17
    band = np.repeat(np.arange(M), np.diff(off))
    wb = w[:, :, band, :]
    z = rng.integers(0, 1 << 16, (B, F, N, C)) & ((1 << wb) - 1)
    first = np.zeros(N, dtype=bool)
    first[off[:-1][np.diff(off) > 0]] = True
    z[:, :, first, :] = (1 << wb[:, :, first, :]) - 1          # the band's width, exactly
    last = np.zeros(N, dtype=bool)
    last[off[1:][np.diff(off) > 0] - 1] = True
    z = np.where(last[None, None, :, None] & (wb == 16), 65534, z)   # 32767 next to -32768
    odd = ((np.arange(N)[None, None, :, None] + np.arange(F)[None, :, None, None]) % 2) == 1
    z = np.where((first & last)[None, None, :, None] & (wb == 16), np.where(odd, 65534, 65535), z)   # one-bin bands
    codes = unzz(z)
    sf = rng.integers(-127, 128, (B, F, M, C)).astype(np.int8)
    sf[rng.random(sf.shape) < 0.07] = -128
    return codes, sf


# ---- CPU -----------------------------------------------------------------------------------------------------------
def test_worked_example():
    off = np.array([0, 0, 2, 5, 8])
    codes = np.array([0, 0, -1, 3, 0, 0, 0, 0], np.int16).reshape(1, 1, 8, 1)
    sf = np.array([0, -3, 5, -128], np.int8).reshape(1, 1, 4, 1)
    np.testing.assert_array_equal(np_widths(codes, sf, off).ravel(), [0, 0, 3, 31])
    data, index = np_pack(codes, sf, off)
    np.testing.assert_array_equal(data.view("<u4"), [0x105F8C00, 0x00000003])
    assert index.tolist() == [[[0]]] and np_row_bits(codes, sf, off).tolist() == [[[37]]]
    c, s = np_unpack(data, index, off, 8)
    np.testing.assert_array_equal(c.ravel(), [0, 0, -1, 3, 0, 0, 0, 0])
    np.testing.assert_array_equal(s.ravel(), [0, 0, 5, -128])


def test_zigzag():
    q = np.array([0, -1, 1, -2, 2, 32767, -32768, -32767], np.int16)
    np.testing.assert_array_equal(zz(q), [0, 1, 2, 3, 4, 65534, 65535, 65533])
    allq = np.arange(-32768, 32768).astype(np.int16)
    np.testing.assert_array_equal(unzz(zz(allq)), allq)
    # the kernels' one zigzag is the 32-bit form: equal to the format's 16-bit form for every int16
    q32 = allq.astype(np.int32)
    np.testing.assert_array_equal(zz(allq), (q32 << 1) ^ (q32 >> 31))
    np.testing.assert_array_equal(bit_length([0, 1, 2, 3, 4, 65535]), [0, 1, 2, 2, 3, 16])


@pytest.mark.parametrize("sr,N,M", [(48000, 128, 64), (48000, 1024, 64), (64, 64, 64)])
def test_restatement_round_trip(sr, N, M):
    off = _offsets(sr, N, M)
    rng = np.random.default_rng(N + M)
    codes, sf = designed(rng, off, 2, 3, 3)
    w = np_widths(codes, sf, off)
    L = np.diff(off)
    assert set(np.unique(w[..., L > 0, :]).tolist()) == set(range(17)) | {31}
    assert (codes == -32768).any() and (codes == 32767).any()
    data, index = np_pack(codes, sf, off)
    c, s = np_unpack(data, index, off, N)
    rc, rs = np_canon(codes, sf, off)
    np.testing.assert_array_equal(c, rc)
    np.testing.assert_array_equal(s, rs)
    if (L == 0).any():
        empty = rs[..., L == 0, :]
        assert ((empty == 0) | (empty == -128)).all() and ((sf[..., L == 0, :] != 0) & (empty == 0)).any()
    # the canonical form is a fixed point
    c2, s2 = np_unpack(*np_pack(rc, rs, off), off, N)
    np.testing.assert_array_equal(c2, rc)
    np.testing.assert_array_equal(s2, rs)


def test_row_length():
    off = _offsets(48000, 128, 64)
    codes, sf = designed(np.random.default_rng(1), off, 2, 4, 2)
    bits = np_row_bits(codes, sf, off)
    data, index = np_pack(codes, sf, off)
    starts = index.reshape(-1)
    lens = np.diff(np.append(starts, len(data)))
    np.testing.assert_array_equal(lens, (bits.reshape(-1) + 31) // 32 * 4)
    assert (starts % 4 == 0).all()
    # the closed form, band by band
    w = np_widths(codes, sf, off)
    L = np.diff(off)
    st = (w >= 1) & (w <= 16)
    np.testing.assert_array_equal(bits, 5 * 64 + (st * (8 + w * L[:, None])).sum(axis=2))
    # worst case: every band at 16 bits
    full = np.full((1, 1, 128, 1), -32768, np.int16)
    assert np_row_bits(full, np.zeros((1, 1, 64, 1), np.int8), off).item() == 16 * 128 + 5 * 64 + 8 * int((L > 0).sum())


def test_library_exports_the_pack_entry_points():
    lib = _lib.load()
    for name in ("ac_pack_index", "ac_pack", "ac_unpack", "ac_pack_scratch_bytes"):
        assert name in _lib.PROTOTYPES
        assert hasattr(lib, name)
    # a scratch of 8 bytes per tile of 2048 rows, none for a single tile
    assert lib.ac_pack_scratch_bytes(1, 1, 1) == 0 and lib.ac_pack_scratch_bytes(0, 5, 2) == 0
    assert lib.ac_pack_scratch_bytes(1, 1024, 2) == 0
    assert lib.ac_pack_scratch_bytes(256, 469, 2) == 8 * ((256 * 469 * 2 + 2047) // 2048)
    # bad arguments are refused before anything reaches a device
    assert lib.ac_pack_index(None, None, None, None, None, None, 1, 1, 1, None) == _lib.AC_EINVAL
    assert lib.ac_pack(None, None, None, None, None, 1, 1, 1, None) == _lib.AC_EINVAL
    assert lib.ac_unpack(None, None, 0, None, None, None, 1, 1, 1, None) == _lib.AC_EINVAL
    assert callable(audiocodec_amd.PsychoacousticModel.pack) and callable(audiocodec_amd.PsychoacousticModel.unpack)
    assert callable(audiocodec_amd.AudioCodec.encode_packed) and callable(audiocodec_amd.AudioCodec.decode_packed)


# ---- GPU -----------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_pack(psy, codes, sf):
    off = psy.scale_band_offsets
    data, index = psy.pack(_dev(codes), _dev(sf))
    rd, ri = np_pack(codes, sf, off)
    np.testing.assert_array_equal(index.cpu().numpy(), ri)
    assert data.dtype == torch.uint8 and data.dim() == 1 and data.numel() == len(rd)
    np.testing.assert_array_equal(data.cpu().numpy(), rd)
    c, s = psy.unpack(data, index)
    rc, rs = np_canon(codes, sf, off)
    np.testing.assert_array_equal(s.cpu().numpy(), rs)
    np.testing.assert_array_equal(c.cpu().numpy(), rc)
    return data, index


@gpu
@pytest.mark.parametrize("sr,N,M", PLANS)
@pytest.mark.parametrize("C", [1, 2, 3, 6])
def test_pack_designed_codes(sr, N, M, C):
    psy = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M)
    B, F = (1, 2) if N == 8192 else (2, 3)
    codes, sf = designed(np.random.default_rng(N + M + C), psy.scale_band_offsets, B, F, C)
    _check_pack(psy, codes, sf)


@gpu
def test_pack_many_bands():
    """M >= 200 at N = 8192: a band scan longer than the workgroup, and the largest staged rows."""
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=8192, bark_bands_n=300)
    codes, sf = designed(np.random.default_rng(2), psy.scale_band_offsets, 1, 2, 2)
    codes[0, 1, :, 1] = -32768          # a worst-case row: every band at 16 bits
    sf[0, 1, :, 1] = 3
    _check_pack(psy, codes, sf)


@gpu
def test_pack_at_the_plan_limits():
    """N = 8192, M = 4096: the largest LDS staging of one channel (a group of one channel, above 32 KB)."""
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=8192, bark_bands_n=4096)
    codes, sf = designed(np.random.default_rng(3), psy.scale_band_offsets, 1, 2, 2)
    codes[0, 0, :, 0] = -32768
    sf[0, 0, :, 0] = 1
    _check_pack(psy, codes, sf)


@gpu
@pytest.mark.parametrize("B,F,C", [(1, 1, 1), (1, 1, 6), (3, 700, 2), (8, 150, 2)])
def test_pack_row_counts(B, F, C):
    """One row; rows that end inside a scan tile; and enough rows (several tiles of the scan) to fill the chip."""
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=960, bark_bands_n=64)
    codes, sf = designed(np.random.default_rng(B * F * C), psy.scale_band_offsets, B, F, C)
    _check_pack(psy, codes, sf)


@gpu
def test_pack_index_scan_of_many_tiles():
    """More scan tiles (of 2048 rows) than one workgroup of the top-level scan holds: the index against the row bits."""
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=64, bark_bands_n=16)
    off = psy.scale_band_offsets
    rng = np.random.default_rng(9)
    B, F, C = 3, 100000, 2
    codes = (rng.integers(-3, 4, (B, F, 64, C)) * (rng.random((B, F, 1, C)) < 0.5)).astype(np.int16)
    sf = np.zeros((B, F, 16, C), np.int8)
    data, index = psy.pack(_dev(codes), _dev(sf))
    lens = (np_row_bits(codes, sf, off).reshape(-1) + 31) // 32 * 4
    ref = np.concatenate([[0], np.cumsum(lens)[:-1]])
    np.testing.assert_array_equal(index.cpu().numpy().reshape(-1), ref)
    assert data.numel() == lens.sum()
    c, s = psy.unpack(data, index)
    assert torch.equal(c, _dev(codes))


def _encoded(N, C, B=2, K=5, seed=0, sr=48000, M=64, nan=True):
    codec = audiocodec_amd.AudioCodec(sr, N, bark_bands_n=M)
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-1, 1, (B, K * N, C)) * np.linspace(0.01, 1, K * N)[None, :, None]).astype(np.float32)
    if nan:
        x[B - 1, K * N // 2, C - 1] = np.nan
    return codec, x


@gpu
@pytest.mark.parametrize("sr,N,M,C", [(48000, 1024, 64, 2), (44100, 1024, 64, 1), (48000, 960, 64, 3), (48000, 2048, 64, 2),
                                      (48000, 128, 64, 6), (48000, 8192, 256, 2)])
def test_pack_quantized_output(sr, N, M, C):
    codec, x = _encoded(N, C, sr=sr, M=M, K=3 if N == 8192 else 5)
    codes, sf = codec.encode_quantized(_dev(x))
    assert (sf == -128).any()
    data, index = _check_pack(codec.psy, codes.cpu().numpy(), sf.cpu().numpy())
    d2, i2 = codec.encode_packed(_dev(x))
    assert torch.equal(d2, data) and torch.equal(i2, index)


@gpu
@pytest.mark.parametrize("N,C,launches", [(1024, 2, 1), (1024, 1, 1), (960, 2, 2), (1024, 3, 2)])
def test_decode_packed_bit_equal(N, C, launches):
    codec, x = _encoded(N, C, B=3, K=7, seed=4)
    assert codec.decode_quantized_launches(C) == launches
    codes, sf = codec.encode_quantized(_dev(x))
    data, index = codec.psy.pack(codes, sf)
    for pcm16 in (False, True):
        a = codec.decode_packed(data, index, pcm16=pcm16)
        b = codec.decode_quantized(codes, sf, pcm16=pcm16)
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.int32) if not pcm16 else a, b.view(torch.int32) if not pcm16 else b)


@gpu
def test_random_access():
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=1024, bark_bands_n=64)
    codes, sf = designed(np.random.default_rng(5), psy.scale_band_offsets, 2, 9, 3)
    data, index = psy.pack(_dev(codes), _dev(sf))
    rc, rs = np_canon(codes, sf, psy.scale_band_offsets)
    perm = [2, 0, 1]
    c, s = psy.unpack(data, index[:, 3:7, perm])
    np.testing.assert_array_equal(c.cpu().numpy(), rc[:, 3:7][..., perm])
    np.testing.assert_array_equal(s.cpu().numpy(), rs[:, 3:7][..., perm])
    view = index[:, 1:8:3]                    # a strided view: every third frame
    assert not view.is_contiguous()
    c, s = psy.unpack(data, view)
    np.testing.assert_array_equal(c.cpu().numpy(), rc[:, 1:8:3])
    np.testing.assert_array_equal(s.cpu().numpy(), rs[:, 1:8:3])


def _set_field(buf, bitpos, value, width):
    for k in range(width):
        byte, bit = (bitpos + k) >> 3, (bitpos + k) & 7
        buf[byte] = (int(buf[byte]) & ~(1 << bit) & 0xFF) | (((value >> k) & 1) << bit)


@gpu
@pytest.mark.parametrize("trim", [0, 3])
def test_unpack_clamps_to_the_buffer(trim):
    """data is a view big[:n] of an allocation whose tail holds 0xFF; the last row's header asks for more bytes than n
    leaves, and another row carries a width field of 17..30.  Bits at or past n must read as 0, not as the tail's ones."""
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=1024, bark_bands_n=64)
    off = psy.scale_band_offsets
    rng = np.random.default_rng(11 + trim)
    codes = rng.integers(-2, 3, (2, 3, 1024, 2)).astype(np.int16)
    sf = rng.integers(-20, 20, (2, 3, 64, 2)).astype(np.int8)
    data, index = np_pack(codes, sf, off)
    data = data.copy()
    idx = index.reshape(-1)
    for j in (50, 60, 63):                     # the last row: its widest bands at 16 bits
        _set_field(data, int(idx[-1]) * 8 + 5 * j, 16, 5)
    _set_field(data, int(idx[2]) * 8 + 5 * 7, 17 + trim * 4, 5)   # a damaged width field
    n = len(data) - trim
    need = int(idx[-1]) + int(np.ceil(np_row_bits_from_header(data, int(idx[-1]), off) / 8))
    assert need > n
    big = torch.full((n + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    big[:n] = _dev(data[:n])
    c, s = psy.unpack(big[:n], _dev(index))
    rc, rs = np_unpack(data[:n], index, off, 1024)
    np.testing.assert_array_equal(s.cpu().numpy(), rs)
    np.testing.assert_array_equal(c.cpu().numpy(), rc)
    assert rs[0, 1, 7, 0] == -128 and rc[0, 1, off[7]:off[8], 0].max() == 0   # (row 2 = (b 0, f 1, c 0))


def np_row_bits_from_header(data, start, off):
    """Bits a row's header claims: 5M + sum over widths 1..16 of (8 + w len)."""
    M = len(off) - 1
    L = np.diff(off)
    total = 5 * M
    for j in range(M):
        w = 0
        for k in range(5):
            p = start * 8 + 5 * j + k
            w |= ((int(data[p >> 3]) >> (p & 7)) & 1) << k if (p >> 3) < len(data) else 0
        if 1 <= w <= 16:
            total += 8 + w * int(L[j])
    return total


@gpu
def test_empty_batch():
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=1024, bark_bands_n=64)
    codes = torch.zeros((0, 3, 1024, 2), dtype=torch.int16, device="cuda")
    sf = torch.zeros((0, 3, 64, 2), dtype=torch.int8, device="cuda")
    data, index = psy.pack(codes, sf)
    assert data.numel() == 0 and tuple(index.shape) == (0, 3, 2)
    c, s = psy.unpack(data, index)
    assert tuple(c.shape) == (0, 3, 1024, 2) and tuple(s.shape) == (0, 3, 64, 2)


@gpu
def test_error_paths():
    codec, x = _encoded(1024, 2, B=1, K=2, nan=False)
    psy = codec.psy
    codes, sf = codec.encode_quantized(_dev(x))
    data, index = psy.pack(codes, sf)
    for bad in (lambda: psy.pack(codes.int(), sf), lambda: psy.pack(codes, sf.short()), lambda: psy.pack(codes, sf[:, :, :-1]),
                lambda: psy.pack(codes[:, :, :-2], sf), lambda: psy.pack(codes.cpu(), sf.cpu()),
                lambda: psy.unpack(data.float(), index), lambda: psy.unpack(data.view(2, -1), index),
                lambda: psy.unpack(data, index.int()), lambda: psy.unpack(data, index[..., None]),
                lambda: psy.unpack(data.cpu(), index), lambda: psy.unpack(data, index.cpu()),
                lambda: codec.decode_packed(data.to(torch.int8), index)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="add_noise"):
        codec.encode_packed(_dev(x).requires_grad_())
    other = audiocodec_amd.AudioCodec(48000, 1024, compute_dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="float32"):
        other.psy.pack(codes, sf)
    with pytest.raises(NotImplementedError, match="float32"):
        other.psy.unpack(data, index)
    with pytest.raises(NotImplementedError, match="float32"):
        other.decode_packed(data, index)
    lib = _lib.load()
    plan = psy._plan(codes.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    total = torch.empty(1, dtype=torch.int64, device="cuda")
    assert lib.ac_pack_index(plan, p(codes), p(sf), None, p(total), None, 1, 3, 2, None) == _lib.AC_EINVAL
    assert lib.ac_pack_index(plan, p(codes), p(sf), p(index), None, None, 1, 3, 2, None) == _lib.AC_EINVAL
    assert lib.ac_pack_index(plan, p(codes), p(sf), p(index), p(total), None, -1, 3, 2, None) == _lib.AC_EINVAL
    assert lib.ac_pack(plan, p(codes), p(sf), p(index), None, 1, 3, 2, None) == _lib.AC_EINVAL
    assert lib.ac_unpack(plan, p(data), -1, p(index), p(codes), p(sf), 1, 3, 2, None) == _lib.AC_EINVAL
    assert lib.ac_unpack(plan, ctypes.c_void_p(data.data_ptr() + 1), data.numel() - 1, p(index), p(codes), p(sf), 1, 3, 2,
                         None) == _lib.AC_EINVAL
    # an unaligned view of data: the Python layer copies it
    store = torch.zeros(data.numel() + 1, dtype=torch.uint8, device="cuda")
    store[1:] = data
    c1, s1 = psy.unpack(store[1:], index)
    c0, s0 = psy.unpack(data, index)
    assert torch.equal(c1, c0) and torch.equal(s1, s0)


@gpu
def test_packed_size_on_uniform_input():
    """The bench's input (uniform noise in [-1, 1]): the stream is below a quarter of the bytes of codes + sf."""
    codec = audiocodec_amd.AudioCodec(48000, 1024)
    x = torch.rand((4, 40 * 1024, 2), device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1
    codes, sf = codec.encode_quantized(x)
    data, index = codec.psy.pack(codes, sf)
    raw = codes.numel() * 2 + sf.numel()
    assert data.numel() < raw / 4
    assert torch.equal(codec.decode_packed(data, index), codec.decode_quantized(codes, sf))
