"""Requantising and transrating: ``PsychoacousticModel.requantize_to_budget`` (the ``thr == NULL`` form
of ``ac_quantize_budget``, k_requantize_budget), ``AudioCodec.transrate_packed_rows`` (the ``AC_IN_PACKED | AC_EMIT_PACKED``
form of ``ac_encode_fused_ex``) and the one launch at filters_n = 1024 that reads, requantises and packs a row in one wave
(k_transrate_p).

Every GPU comparison of the one launch is ``torch.equal`` against the composition -- ``unpack``, ``requantize_to_budget`` at
offset 0 upwards, rows longer than their slot marked, ``ac_pack`` at the fixed row starts into zero-filled data -- which runs
everywhere while ``AC_TRANSRATE_NOFUSE=1`` is set; the composition is compared byte for byte with the numpy restatement of
``transrate_reference.py``.  The rows come from ``encode_quantized()`` / ``encode_packed_rows()`` of test_encode_cbr's
``_input`` (a zero frame, NaN, Inf, the 1e15 and the 3e12 sample) where the shape allows the injection (B >= 3, K >= 4), from
the ramped noise alone elsewhere; before any comparison the reference alone must show what a binding budget shows
(``_binding``).
"""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib
from conftest import ROOT

import fused_layouts as fl
from pack_reference import np_canon, np_pack, np_row_bits
from pack_rows_reference import marked_row, row_bytes
from test_encode_cbr import _input
from test_encode_quantized_fused import _pcm, _same, _where
from test_quantizer import np_inv, np_offsets, np_quantize, np_step
from test_rate_control import EX_OFF, EX_THR, EX_X
from transrate_reference import np_transrate, requant_brute, requant_fast, requantize_budget

gpu = pytest.mark.gpu
N0, M0 = 1024, 64
CAP = _lib.AC_PACK_ROWS_MAX_BITS
HEADER = os.path.join(ROOT, "include", "audiocodec_amd.h")
SHAPES = [(1, 1, 1), (2, 3, 2), (3, 5, 1), (2, 2, 3)]          # (B, K, C): 2, 16, 18 (tail waves in the last workgroup), 18 rows
LADDERS = [(2730, 1365), (2730, 682), (1365, 320), (1365, 1365)]   # (R, R'): 320 = 5M is the floor, the last passes through


# ---- CPU: the definition ----------------------------------------------------------------------------------------------
def test_identity_at_offset_zero_exhaustive():
    """clamp(rint(fp32(fp32(q step(s)) inv(s))), +-32767) == clamp(q, +-32767) for every int16 q and every s in [-127, 127]: a
    row that fits its new budget passes through with its fields unchanged."""
    q = np.arange(-32768, 32768, dtype=np.int32)
    want = np.clip(q, -32767, 32767)
    for s in range(-127, 128):
        x = (q.astype(np.float32) * np_step(s)).astype(np.float32)
        back = np.clip(np.rint((x * np_inv(s)).astype(np.float32)), -32767, 32767).astype(np.int32)
        assert np.array_equal(back, want), s


def test_worked_example():
    """Section 8c's example (M = 4): its 100-bit row requantised to 96 / 64 / 56 / 20 bits.  The brute-force search gives the
    table (it is section 8c's own: the requantiser lands where the quantiser would have), and both searches agree."""
    codes0, sf0 = np_quantize(EX_X, EX_THR, EX_OFF)
    assert np_row_bits(codes0, sf0, EX_OFF).ravel()[0] == 100
    table = {100: (0, 100, [0, -30, -22, -44], [54, -36, 45, -32, 2, 20, 0, -41]),
             96: (3, 94, [0, -27, -19, -41], [32, -21, 27, -19, 1, 12, 0, -24]),
             64: (20, 62, [0, -10, -2, -24], [2, -1, 1, -1, 0, 1, 0, -1]),
             56: (26, 32, [0, -4, 4, -18], [1, 0, 0, 0, 0, 0, 0, 0]),
             20: (28, 20, [0, -2, 6, -16], [0, 0, 0, 0, 0, 0, 0, 0])}
    for R, (k, bits, sf, codes) in table.items():
        brute = requant_brute(codes0, sf0, EX_OFF, R)
        fast = requant_fast(codes0, sf0, EX_OFF, R)
        for a, b in zip(brute, fast):
            np.testing.assert_array_equal(a, b)
        assert (int(brute[2].ravel()[0]), int(brute[3].ravel()[0])) == (k, bits), R
        assert brute[1].ravel().tolist() == sf and brute[0].ravel().tolist() == codes, R
    # at offset 0 the row is the input row
    np.testing.assert_array_equal(requantize_budget(codes0, sf0, EX_OFF, 100)[0], codes0)


def _random_rows(rng, off, B, F, C):
    """Canonical and non-canonical rows: random widths per band, scale factors over the whole range, -128 bands with junk
    codes, all-zero bands with a scale factor, and the code -32768."""
    N, M = int(off[-1]), len(off) - 1
    band = np.repeat(np.arange(M), np.diff(off))
    w = rng.integers(0, 17, (B, F, M, C))
    mag = (1 << w[:, :, band, :]) >> 1
    codes = (rng.integers(-32768, 32768, (B, F, N, C)) % np.maximum(mag, 1)) * rng.choice([-1, 1], (B, F, N, C))
    codes = np.where(mag == 0, 0, codes).astype(np.int16)
    sf = rng.integers(-127, 128, (B, F, M, C)).astype(np.int8)
    sf[rng.random(sf.shape) < 0.05] = -128
    codes[0, 0, :4, 0] = [-32768, 32767, -32767, 1]
    return codes, sf


def test_bits_do_not_grow_with_the_offset_and_searches_agree():
    rng = np.random.default_rng(5)
    for sr, N, M in [(44100, 256, 48), (48000, 128, 64)]:
        off = np_offsets(sr, N, M)
        codes, sf = _random_rows(rng, off, 2, 3, 2)
        natural = np_row_bits(*np_canon(codes, sf, off), off)
        R = np.maximum(5 * M, (natural * rng.uniform(0.0, 1.1, natural.shape)).astype(np.int64))
        brute = requant_brute(codes, sf, off, R)
        fast = requant_fast(codes, sf, off, R)
        for a, b in zip(brute, fast):
            np.testing.assert_array_equal(a, b)
        bits = brute[4]
        assert (np.diff(bits, axis=0) <= 0).all()
        assert len(np.unique(brute[2])) >= 3
        # bits(0) is the canonical input row's own length
        np.testing.assert_array_equal(bits[0], natural)


def test_a_saturated_row_never_fits():
    """Every scale factor 127 and codes +-32767: no offset brings it under a small budget -- offset 254, the marked row."""
    codes = np.full((1, 1, 8, 1), 32767, np.int16)
    codes[0, 0, 1::2] = -32767
    sf = np.full((1, 1, 4, 1), 127, np.int8)
    rc, rs, offset, bits = requantize_budget(codes, sf, EX_OFF, 20)
    assert rs.ravel().tolist() == [0, 127, 127, 127] and int(offset.ravel()[0]) == 254
    assert int(bits.ravel()[0]) == 20 + 3 * 8 + 16 * 8 > 8 * row_bytes(20)
    np.testing.assert_array_equal(rc, codes)
    data, index = np_pack(codes, sf, EX_OFF)
    out, _, fits, off2, _ = np_transrate(data, index, EX_OFF, 8, 20)
    assert not fits.any() and int(off2.ravel()[0]) == 254
    np.testing.assert_array_equal(out, marked_row(4, 20))


def test_a_marked_row_passes_through_and_fits():
    """fits reports only whether this call's row fitted.  Every band that holds bins keeps width 31; the example's band 0 is
    empty, and an empty band's scale factor is 0 at every offset (rule 1), so its width field comes out 0."""
    sf = np.full((1, 1, 4, 1), -128, np.int8)
    data, index = np_pack(np.zeros((1, 1, 8, 1), np.int16), sf, EX_OFF)
    np.testing.assert_array_equal(data, marked_row(4, 20))
    out, _, fits, offset, bits = np_transrate(data, index, EX_OFF, 8, 20)
    assert fits.all() and int(offset.ravel()[0]) == 0 and int(bits.ravel()[0]) == 20
    np.testing.assert_array_equal(out, [0xE0, 0xFF, 0x0F, 0x00])
    off = np_offsets(48000, N0, M0)                              # no empty band: the same bytes
    data, index = np_pack(np.zeros((1, 1, N0, 1), np.int16), np.full((1, 1, M0, 1), -128, np.int8), off)
    out, _, fits, _, _ = np_transrate(data, index, off, N0, 1365)
    assert fits.all()
    np.testing.assert_array_equal(out, marked_row(M0, 1365))


# ---- CPU: header, library, Python validation ------------------------------------------------------------------------------
def test_header_declares_the_flag_the_struct_and_the_launch_query():
    text = open(HEADER).read()
    assert re.search(r"\bAC_IN_PACKED\s*=\s*64\b", text)
    m = re.search(r"typedef\s+struct\s+ac_quantized_rows\s*\{(.*?)\}\s*ac_quantized_rows\s*;", text, flags=re.S)
    assert m, "ac_quantized_rows is not declared"
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["const int16_t* codes", "const int8_t* sf"], fields
    m = re.search(r"AC_API\s+int\s+ac_transrate_launches\s*\(([^;]*)\)\s*;", text)
    assert m and "stream" not in m.group(1), m and m.group(1)
    assert re.search(r"#define\s+AC_VERSION\s+171\b", text)


def test_library_exports_the_launch_query():
    lib = _lib.load()
    assert "ac_transrate_launches" in _lib.PROTOTYPES and callable(lib.ac_transrate_launches)
    assert lib.ac_transrate_launches(None, 2) == 0
    assert lib.ac_version() == 171
    assert _lib.AC_IN_PACKED == 64


def test_ctypes_mirror_has_the_headers_layout():
    Q = _lib.QuantizedRows
    assert [f[0] for f in Q._fields_] == ["codes", "sf"]
    assert (Q.codes.offset, Q.sf.offset) == (0, 8) and ctypes.sizeof(Q) == 16


def test_python_interface_validates_its_arguments():
    base = audiocodec_amd.AudioCodec(48000, N0)
    data, index = torch.zeros(64, dtype=torch.uint8), torch.zeros((1, 1, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"with_bitrate\(\)"):
        base.transrate_packed_rows(data, index)
    cbr = base.with_bitrate(64000)
    for bad in ((data.to(torch.int8), index), (data, index.to(torch.int32)), (data.view(8, 8), index), (data, index[0]),
                (data, index)):                               # the last: host tensors
        with pytest.raises(ValueError):
            cbr.transrate_packed_rows(*bad)
    with pytest.raises(TypeError):
        cbr.transrate_packed_rows(data.numpy(), index)
    with pytest.raises(NotImplementedError, match="float32"):
        f64 = audiocodec_amd.AudioCodec(48000, N0, compute_dtype=torch.float64)
        f64.transrate_packed_rows(data, index)
    codes, sf = torch.zeros((1, 1, N0, 2), dtype=torch.int16), torch.zeros((1, 1, M0, 2), dtype=torch.int8)
    for bad in ((codes.to(torch.int32), sf), (codes, sf.to(torch.int16)), (codes[:, :, :512], sf), (codes, sf[:, :, :32]),
                (codes[0], sf[0]), (codes, sf)):              # the last: host tensors
        with pytest.raises(ValueError):
            base.psy.requantize_to_budget(*bad, 1365)
    for bad in (-1, 255, -254):
        with pytest.raises(ValueError, match="min_offset"):
            base.psy.requantize_to_budget(codes, sf, 1365, bad)
    for bad in (1.0, True, None):
        with pytest.raises(TypeError):
            base.psy.requantize_to_budget(codes, sf, 1365, bad)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
class _nofuse:
    """AC_TRANSRATE_NOFUSE=1 (read per call) around a block."""

    def __enter__(self):
        os.environ["AC_TRANSRATE_NOFUSE"] = "1"

    def __exit__(self, *exc):
        del os.environ["AC_TRANSRATE_NOFUSE"]
        return False


def _composition(codec, data, index, return_offset=True):
    with _nofuse():
        assert codec.transrate_packed_rows_launches(index.shape[2]) == 3
        return codec.transrate_packed_rows(data, index, return_offset)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _x(B, K, C, seed, N=N0):
    """test_encode_cbr's input with its injections where the shape allows them (B >= 3, K >= 4: they include an all-zero
    frame); elsewhere the ramped noise, from two blocks on with block 0 of clip 0 zeroed, so that frame 0 there is an all-zero row."""
    inject = B >= 3 and K >= 4
    x = _input(C, B, K, seed, inject, N)
    if not inject and K >= 2:
        x[0, :N] = 0.0
    return x


def _check_requantize(psy, codes, sf, R, kmin=0):
    """requantize_to_budget against the numpy restatement, bit for bit; returns the reference."""
    off = psy.scale_band_offsets
    Rd = _dev(np.asarray(R, dtype=np.int32)) if isinstance(R, np.ndarray) else R
    got = psy.requantize_to_budget(_dev(codes), _dev(sf), Rd, kmin)
    ref = requantize_budget(codes, sf, off, R, kmin)
    B, F, N, C = codes.shape
    assert got[0].dtype == torch.int16 and got[1].dtype == torch.int8 and got[1].shape == sf.shape
    assert got[2].dtype == torch.int16 and got[2].shape == (B, F, C) and got[3].dtype == torch.int32
    for name, g, r in zip(("offset", "row_bits", "sf", "codes"), (got[2], got[3], got[1], got[0]), (ref[2], ref[3], ref[1], ref[0])):
        np.testing.assert_array_equal(g.cpu().numpy(), r, err_msg="%s at R = %s" % (name, R if np.isscalar(R) else "per row"))
    return ref


@gpu
@pytest.mark.parametrize("B,K,C", SHAPES)
def test_requantizer_against_numpy(B, K, C):
    base = audiocodec_amd.AudioCodec(48000, N0)
    codes, sf = (t.cpu().numpy() for t in base.encode_quantized(_x(B, K, C, C + 2 * B + K)))
    offs = []
    for R in (1365, 682, 320, 16 * N0 + 13 * M0):
        ref = _check_requantize(base.psy, codes, sf, R)
        offs.append(ref[2])
    assert int(offs[0].max()) > 0 and int(offs[3].max()) == 0           # a binding budget binds; an unlimited one does not
    np.testing.assert_array_equal(requantize_budget(codes, sf, base.psy.scale_band_offsets, 16 * N0 + 13 * M0)[0], codes)
    rng = np.random.default_rng(B + K + C)
    natural = np_row_bits(codes, sf, base.psy.scale_band_offsets)
    per_row = np.maximum(320, (natural * rng.uniform(0.1, 1.1, natural.shape))).astype(np.int32)
    ref = _check_requantize(base.psy, codes, sf, per_row)
    assert len(np.unique(ref[2])) >= 2 or ref[2].size < 16
    ref = _check_requantize(base.psy, codes, sf, 1365, kmin=7)
    assert int(ref[2].min()) >= 7


@gpu
@pytest.mark.parametrize("N", [2048, 960])
def test_requantizer_other_sizes(N):
    base = audiocodec_amd.AudioCodec(48000, N)
    codes, sf = (t.cpu().numpy() for t in base.encode_quantized(_x(3, 5, 2, 40 + N, N)))
    for R in (1365, 600):
        ref = _check_requantize(base.psy, codes, sf, R)
        assert int(ref[2].max()) > 0 and len(np.unique(ref[2])) >= 2


@gpu
@pytest.mark.parametrize("sr,N,M,C", [(48000, 1024, 64, 2), (44100, 256, 48, 3), (48000, 128, 64, 5)])
def test_requantizer_non_canonical_input(sr, N, M, C):
    """Junk codes under -128 bands, a scale factor on all-zero bands, -32768: the output is that of the canonical row."""
    psy = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M)
    off = psy.scale_band_offsets
    codes, sf = _random_rows(np.random.default_rng(N + C), off, 2, 3, C)
    cc, cs = np_canon(codes, sf, off)
    assert not np.array_equal(cc, codes) and not np.array_equal(cs, sf)
    natural = np_row_bits(cc, cs, off)
    for R in (int(natural.max()), int(np.median(natural)) // 2 + 5 * M, 5 * M):
        ref = _check_requantize(psy, codes, sf, R)
        same = psy.requantize_to_budget(_dev(cc), _dev(cs), R)
        for g, r in zip(same, ref):
            np.testing.assert_array_equal(g.cpu().numpy(), r)
    assert int(ref[2].max()) == 254                                       # saturated bands at sf 127 do not shrink


def _binding(R2, offset, bits, fits, unfit):
    """What the reference must show, so that a degenerate input cannot pass."""
    assert int((offset > 0).sum()) >= 1, "no row above offset 0"
    if R2 > 320 and offset.size >= 16:                         # (the two rows of one block have no all-zero frame)
        assert int(((offset == 0) & (bits < R2)).sum()) >= 1, "no row at offset 0 below its budget"
        flat = offset.ravel()
        assert int((flat[1:] != flat[:-1]).sum()) >= 1, "every row has its neighbour's offset"
    if unfit:
        assert int((~fits).sum()) >= 1, "no row that does not fit"


@gpu
@pytest.mark.parametrize("B,K,C", SHAPES)
def test_transrate_fused_composition_numpy(B, K, C):
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    x = _x(B, K, C, C + 2 * B + K)
    inject = B >= 3 and K >= 4
    for R, R2 in LADDERS:
        src, dst = base.with_row_budget(R), base.with_row_budget(R2)
        data, index, _ = src.encode_packed_rows(x)
        ref = np_transrate(data.cpu().numpy(), index.cpu().numpy(), off, N0, R2)
        print("%d -> %d: %d rows, offsets %s, %d unfit" % (R, R2, ref[3].size, np.unique(ref[3]).tolist(), int((~ref[2]).sum())))
        if R2 != R:
            # the 3e12 row fits the 2730-bit source alone, and no offset brings it under a smaller budget; at the 1365-bit
            # source it is a marked row already, and a marked row always fits
            _binding(R2, ref[3], ref[4], ref[2], unfit=inject and R == 2730)
        else:
            assert int(ref[3].max()) == 0                                 # the pass-through
        comp = _composition(dst, data, index)
        for name, g, r in zip(("data", "index", "fits", "offset"), comp, ref):
            np.testing.assert_array_equal(g.cpu().numpy(), r, err_msg="%s, %d -> %d" % (name, R, R2))
        assert dst.transrate_packed_rows_launches(C) == 1
        fused = dst.transrate_packed_rows(data, index, True)
        assert fused[0].dtype == torch.uint8 and fused[0].shape == (B * (K + 1) * C * dst.row_bytes,)
        assert fused[2].dtype == torch.bool and fused[3].dtype == torch.int16
        for name, g, r in zip(("data", "index", "fits", "offset"), fused, comp):
            assert torch.equal(g, r), (name, R, R2, _where(g, r))
        assert len(dst.transrate_packed_rows(data, index)) == 3
        if R2 == R:                                                       # every row that fitted keeps its bytes
            assert torch.equal(fused[0], data) and bool(fused[2].all())


def _upload(data, index):
    return _dev(np.asarray(data, dtype=np.uint8)), _dev(np.asarray(index, dtype=np.int64))


def _three_ways(dst, data, index, off):
    """numpy, the composition and the one launch on the same rows: returns the reference."""
    ref = np_transrate(data, index, off, N0, dst.row_bits)
    d, i = _upload(data, index)
    comp = _composition(dst, d, i)
    assert dst.transrate_packed_rows_launches(index.shape[2]) == 1
    fused = dst.transrate_packed_rows(d, i, True)
    for name, g, c, r in zip(("data", "index", "fits", "offset"), fused, comp, ref):
        np.testing.assert_array_equal(c.cpu().numpy(), r, err_msg=name)
        assert torch.equal(g, c), (name, _where(g, c))
    return ref


@gpu
def test_adversarial_rows():
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    band = np.repeat(np.arange(M0), np.diff(off))
    rng = np.random.default_rng(77)
    B, F, C = 1, 6, 2
    codes = rng.integers(-200, 201, (B, F, N0, C)).astype(np.int16)
    sf = rng.integers(-40, 0, (B, F, M0, C)).astype(np.int8)
    # row (0, 0): every band at width 16, +-32767 and -32768 -- 17216 bits, longer than the output cap
    codes[0, 0, :, 0] = np.where(np.arange(N0) % 3 == 0, -32768, np.where(np.arange(N0) % 3 == 1, 32767, -32767))
    # row (0, 1): scale factors at both ends of the range
    sf[0, 0, :, 1] = np.where(np.arange(M0) % 2 == 0, 127, -127)
    # row (1, 0): the saturating row no offset brings under a small budget
    codes[0, 1, :, 0] = np.where(np.arange(N0) % 2 == 0, 32767, -32767)
    sf[0, 1, :, 0] = 127
    # row (1, 1): -128 bands and all-zero bands between stored ones
    sf[0, 1, ::3, 1] = -128
    codes[0, 1, :, 1] = np.where((band % 3 == 1), 0, codes[0, 1, :, 1])
    data, index = np_pack(codes, sf, off)
    assert int(np_row_bits(codes, sf, off)[0, 0, 0]) == 16 * N0 + 13 * M0 > CAP
    for R2 in (1365, 320, CAP):
        ref = _three_ways(base.with_row_budget(R2), data, index, off)
        assert not ref[2][0, 1, 0] and int(ref[3][0, 1, 0]) == 254        # the saturating row: marked, at 254
        assert int(ref[3][0, 0, 0]) > 0
    dst = base.with_row_budget(1365)
    # widths 17 .. 30 read as 31: overwrite some width fields of row (2, 0)
    damaged = data.copy()
    bits = np.unpackbits(damaged, bitorder="little")
    start = int(index[0, 2, 0]) * 8
    for j, wv in ((3, 17), (10, 30), (40, 23)):
        bits[start + 5 * j:start + 5 * j + 5] = [(wv >> k) & 1 for k in range(5)]
    damaged = np.packbits(bits, bitorder="little")
    _three_ways(dst, damaged, index, off)
    # data truncated in the middle of its last row, and in the middle of a header
    for cut in (int(index[0, 5, 1]) + 100, int(index[0, 5, 1]) + 13, int(index[0, 3, 0]) + 2):
        _three_ways(dst, data[:cut], index, off)
    # row starts negative, past the end and off the 4-byte phase
    odd = index.copy()
    odd[0, 0, 0], odd[0, 1, 1], odd[0, 2, 0], odd[0, 3, 1], odd[0, 4, 0] = -7, len(data) + 1000, index[0, 2, 0] + 1, -(1 << 50), len(data) - 3
    odd[0, 5, 0] = (1 << 40)
    _three_ways(dst, data, odd, off)
    # a permuted index and a slice of frames
    perm = index.reshape(-1)[rng.permutation(index.size)].reshape(index.shape)
    ref = _three_ways(dst, data, perm, off)
    assert len(np.unique(ref[3])) >= 2
    _three_ways(dst, data, np.ascontiguousarray(index[:, 1:3]), off)
    d, i = _upload(data, index)
    got = dst.transrate_packed_rows(d, i[:, 1:3])                         # a strided view of the index tensor
    assert torch.equal(got[0], dst.transrate_packed_rows(d, i[:, 1:3].contiguous())[0])


@gpu
def test_dense_encode_packed_input():
    base = audiocodec_amd.AudioCodec(48000, N0)
    x = _x(3, 5, 2, 21)
    data, index = base.encode_packed(x)                                   # dense rows of the unbudgeted quantiser
    for R2 in (2730, 682):
        dst = base.with_row_budget(R2)
        comp = _composition(dst, data, index)
        fused = dst.transrate_packed_rows(data, index, True)
        for g, c in zip(fused, comp):
            assert torch.equal(g, c), _where(g, c)
        assert int(comp[3].max()) > 0
    ref = np_transrate(data.cpu().numpy(), index.cpu().numpy(), base.psy.scale_band_offsets, N0, 682)
    np.testing.assert_array_equal(comp[0].cpu().numpy(), ref[0])


@gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", fl.LAYOUTS, ids=fl.LAYOUT_IDS)
def test_band_layouts(layout, C):
    """One-bin bands, granules that straddle bands and empty bands (fused_layouts.LAYOUTS), on its ``tonal`` input."""
    sr, alpha = fl.resolve(layout)
    base = audiocodec_amd.AudioCodec(sr, N0, alpha=alpha)
    off = base.psy.scale_band_offsets
    x = torch.from_numpy(fl.tonal(C)).cuda()
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(x)
    for R2 in (1365, 400):
        dst = base.with_row_budget(R2)
        ref = np_transrate(data.cpu().numpy(), index.cpu().numpy(), off, N0, R2)
        assert int((ref[3] > 0).sum()) >= 1 and len(np.unique(ref[3])) >= 2
        comp = _composition(dst, data, index)
        assert dst.transrate_packed_rows_launches(C) == 1
        fused = dst.transrate_packed_rows(data, index, True)
        for name, g, c, r in zip(("data", "index", "fits", "offset"), fused, comp, ref):
            np.testing.assert_array_equal(c.cpu().numpy(), r, err_msg=name)
            assert torch.equal(g, c), (name, _where(g, c))


@gpu
def test_launch_table(monkeypatch):
    base = audiocodec_amd.AudioCodec(48000, N0)
    assert base.transrate_packed_rows_launches(2) == 0                    # no budget
    for C in (1, 2, 3, 7):
        for R in (320, 1365, CAP):
            assert base.with_row_budget(R).transrate_packed_rows_launches(C) == 1, (C, R)
    assert base.with_row_budget(CAP + 32).transrate_packed_rows_launches(2) == 3
    for N, M in ((2048, 64), (960, 64), (1024, 32)):
        assert audiocodec_amd.AudioCodec(48000, N, bark_bands_n=M).with_row_budget(1365).transrate_packed_rows_launches(2) == 3
    cbr = base.with_row_budget(1365)
    monkeypatch.setenv("AC_TRANSRATE_NOFUSE", "1")
    assert cbr.transrate_packed_rows_launches(2) == 3
    monkeypatch.delenv("AC_TRANSRATE_NOFUSE")
    assert cbr.transrate_packed_rows_launches(2) == 1


@gpu
def test_other_sizes_run_the_composition():
    """filters_n = 2048: three launches, the numpy restatement's bytes."""
    base = audiocodec_amd.AudioCodec(48000, 2048)
    x = _x(3, 5, 2, 9, 2048)
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(x)
    dst = base.with_row_budget(1365)
    assert dst.transrate_packed_rows_launches(2) == 3
    got = dst.transrate_packed_rows(data, index, True)
    ref = np_transrate(data.cpu().numpy(), index.cpu().numpy(), base.psy.scale_band_offsets, 2048, 1365)
    assert int(ref[3].max()) > 0
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g.cpu().numpy(), r)


@gpu
def test_chip_filling():
    """8224 rows -- 2056 workgroups of four waves -- of seeded noise at many levels, against the composition."""
    B, K, C = 16, 256, 2
    base = audiocodec_amd.AudioCodec(48000, N0)
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.rand((B, K * N0, C), generator=g, device="cuda") * 2 - 1
    x *= torch.logspace(-3, 0, B, device="cuda")[:, None, None] * torch.linspace(0.05, 1, K * N0, device="cuda")[None, :, None]
    x[0] = 0.0                                                            # 514 all-zero rows: offset 0
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(x)
    dst = base.with_row_budget(1365)
    assert index.numel() == 8224 and (index.numel() + 3) // 4 >= 2048 and dst.transrate_packed_rows_launches(C) == 1
    fused = dst.transrate_packed_rows(data, index, True)
    comp = _composition(dst, data, index)
    for name, a, b in zip(("data", "index", "fits", "offset"), fused, comp):
        assert torch.equal(a, b), (name, _where(a, b))
    off = comp[3]
    assert int((off > 0).sum()) >= 1000 and int((off == 0).sum()) >= 100 and bool(comp[2].all()) and int(fused[0].max()) > 0


def _transrate_abi(codec, data, index, out, fits, rb, flags=None, X=None, t=None, thr=None, offset=None, B=None, src=True,
                   dst=True):
    lib = _lib.load()
    dev = data.device
    rows = _lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr())
    po = _lib.PackedOut(out.data_ptr(), rb, fits.data_ptr())

    def p(v):
        return ctypes.c_void_p(v.data_ptr()) if v is not None else None
    st = lib.ac_encode_fused_ex(codec.mdct._plan(dev), codec.psy._plan(dev), ctypes.addressof(rows) if src else None, p(X), p(t),
                                p(thr), 0.0, (_lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED) if flags is None else flags,
                                ctypes.addressof(po) if dst else None, p(offset), 0, index.shape[0] if B is None else B,
                                index.shape[1] - 1, index.shape[2], None)
    torch.cuda.synchronize()
    return st


@gpu
def test_c_abi():
    lib = _lib.load()
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    data, index, _ = src.encode_packed_rows(_x(3, 5, 2, 17))
    rows, rb = index.numel(), dst.row_bytes
    out = torch.full((rows * rb,), 0xA5, dtype=torch.uint8, device="cuda")
    fits = torch.full((rows,), 7, dtype=torch.uint8, device="cuda")
    offset = torch.full((rows,), -3, dtype=torch.int16, device="cuda")
    spare = torch.zeros((3, 6, N0, 2), device="cuda")
    refused = (out.clone(), fits.clone(), offset.clone())
    IN, EMIT = _lib.AC_IN_PACKED, _lib.AC_EMIT_PACKED
    for flags in (IN, IN | _lib.AC_EMIT_CODES, IN | EMIT | _lib.AC_IN_PCM16, IN | EMIT | _lib.AC_EMIT_NOISY, IN | _lib.AC_IN_PCM16,
                  IN | EMIT | _lib.AC_EMIT_DB_NORM, IN | EMIT | 128):
        assert _transrate_abi(dst, data, index, out, fits, rb, flags=flags, offset=offset) == _lib.AC_EINVAL, flags
        assert lib.ac_last_error()
    for kw in ({"X": spare}, {"t": spare}, {"thr": spare}, {"src": False}, {"dst": False}):
        assert _transrate_abi(dst, data, index, out, fits, rb, offset=offset, **kw) == _lib.AC_EINVAL, kw
    assert _transrate_abi(dst, data, index, out, fits, rb + 4, offset=offset) == _lib.AC_EINVAL
    assert b"row_bytes" in lib.ac_last_error()
    assert _transrate_abi(base, data, index, out, fits, rb, offset=offset) == _lib.AC_EINVAL and b"row budget" in lib.ac_last_error()
    wide = audiocodec_amd.AudioCodec(48000, 2048).with_row_budget(1365)
    assert _transrate_abi(wide, data, index, out, fits, rb, offset=offset) == _lib.AC_EUNSUPPORTED
    assert b"composition" in lib.ac_last_error()
    with _nofuse():
        assert _transrate_abi(dst, data, index, out, fits, rb, offset=offset) == _lib.AC_EUNSUPPORTED
    other = audiocodec_amd.AudioCodec(48000, 2048)
    st = lib.ac_encode_fused_ex(other.mdct._plan(data.device), dst.psy._plan(data.device), None, None, None, None, 0.0, IN | EMIT,
                                None, None, 0, 3, 5, 2, None)
    assert st == _lib.AC_EINVAL and b"filters_n" in lib.ac_last_error()
    for got, want in zip((out, fits, offset), refused):                   # the refused calls wrote nothing
        assert torch.equal(got, want)
    assert _transrate_abi(dst, data, index, out, fits, rb, offset=offset, B=0) == _lib.AC_OK
    assert torch.equal(out, refused[0])
    assert _transrate_abi(dst, data, index, out, fits, rb, offset=offset) == _lib.AC_OK, lib.ac_last_error()
    ref = _composition(dst, data, index)
    assert torch.equal(out, ref[0]) and torch.equal(fits.view(3, 6, 2), ref[2].to(torch.uint8))
    assert torch.equal(offset.view(3, 6, 2), ref[3])
    out.fill_(0xA5)
    assert _transrate_abi(dst, data, index, out, fits, rb) == _lib.AC_OK  # out1 may be NULL
    assert torch.equal(out, ref[0])
    # the requantiser's form of ac_quantize_budget refuses a negative kmin
    codes, sf = base.psy.unpack(data, index)
    q = _lib.QuantizedRows(codes.data_ptr(), sf.data_ptr())
    oc, os_, oo = torch.empty_like(codes), torch.empty_like(sf), torch.empty((3, 6, 2), dtype=torch.int16, device="cuda")
    plan = base.psy._plan(data.device)

    def call(kmin):
        return lib.ac_quantize_budget(plan, ctypes.addressof(q), None, 1365, None, kmin, ctypes.c_void_p(oc.data_ptr()),
                                      ctypes.c_void_p(os_.data_ptr()), ctypes.c_void_p(oo.data_ptr()), None, 3, 6, 2, None)
    assert call(-1) == _lib.AC_EINVAL and b"kmin" in lib.ac_last_error()
    assert call(255) == _lib.AC_EINVAL
    assert call(0) == _lib.AC_OK
    torch.cuda.synchronize()
    assert torch.equal(oo, ref[3])


@pytest.fixture(scope="module")
def harness():
    from stream_order import Harness
    return Harness()


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
@pytest.mark.parametrize("check", ["delayed_producer", "busy_default"])
def test_stream_contract(harness, check, route):
    base = audiocodec_amd.AudioCodec(48000, N0)
    dst = base.with_row_budget(1365)
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(_pcm(N0, 2, 4, 20, seed=77, inject=False))
    torch.cuda.synchronize()
    assert dst.transrate_packed_rows_launches(2) == 1
    fn = (lambda d, i: dst.transrate_packed_rows(d, i, True)) if route == "fused" else (lambda d, i: _composition(dst, d, i))
    getattr(harness, check)("cbr.transrate_packed_rows[1024-2,%s]" % route, ([data, index], fn))


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
def test_graph_capture(route):
    """One eager call (plans, allocator), then a linear capture on one stream, replayed on new contents of the same data."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    call = (lambda d, i: dst.transrate_packed_rows(d, i, True)) if route == "fused" else (lambda d, i: _composition(dst, d, i))
    data, index, _ = src.encode_packed_rows(_x(3, 5, 2, 5))
    call(data, index)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(data, index)
    for seed in (6, 7):
        data.copy_(src.encode_packed_rows(_x(3, 5, 2, seed))[0])
        g.replay()
        torch.cuda.synchronize()
        ref = call(data.clone(), index)
        assert int((ref[3] > 0).sum()) >= 1 and int(ref[0].max()) > 0
        for got, want in zip(out, ref):
            assert torch.equal(got, want), (seed, _where(got, want))


@gpu
def test_an_empty_batch_gives_empty_results():
    dst = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    data = torch.zeros((64,), dtype=torch.uint8, device="cuda")
    for shape in ((0, 3, 2), (2, 0, 2)):
        index = torch.zeros(shape, dtype=torch.int64, device="cuda")
        got = dst.transrate_packed_rows(data, index, True)
        assert got[0].shape == (0,) and got[1].shape == shape and got[2].shape == shape and got[2].dtype == torch.bool
        assert got[3].shape == shape and got[3].dtype == torch.int16 and len(dst.transrate_packed_rows(data, index)) == 3
    codes = torch.zeros((0, 3, N0, 2), dtype=torch.int16, device="cuda")
    sf = torch.zeros((0, 3, M0, 2), dtype=torch.int8, device="cuda")
    assert dst.psy.requantize_to_budget(codes, sf, 1365)[2].shape == (0, 3, 2)


@gpu
def test_chunks_of_a_stream_transrate_to_the_one_shot_rows():
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    B, K, C = 3, 5, 2
    x = _x(B, K, C, 31)
    data, index, _ = src.encode_packed_rows(x)
    whole = dst.transrate_packed_rows(data, index, True)
    rb = dst.row_bytes
    rows = whole[0].view(B, K + 1, C, rb)
    st = src.stream(B, C)
    a = 0
    for k in (2, 1, 2):
        d, i, _ = st.encode_packed_rows_chunk(x[:, a * N0:(a + k) * N0].contiguous())
        got = dst.transrate_packed_rows(d, i, True)
        assert torch.equal(got[0].view(B, k, C, rb), rows[:, a:a + k]), (a, k)
        assert torch.equal(got[2], whole[2][:, a:a + k]) and torch.equal(got[3], whole[3][:, a:a + k])
        a += k
    assert int((whole[3] > 0).sum()) >= 1


@gpu
@pytest.mark.parametrize("pcm16", [False, True])
def test_end_to_end_decode(pcm16):
    """decode_packed of transrated rows == decode_quantized of the requantised codes, bit for bit."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_row_budget(2730), base.with_row_budget(682)
    x = _pcm(N0, 2, 3, 5, seed=32, inject=True)
    data, index, _ = src.encode_packed_rows(x)
    out, idx, fits, offset = dst.transrate_packed_rows(data, index, True)
    assert bool(fits.all()) and int((offset > 0).sum()) >= 1
    got = dst.decode_packed(out, idx, pcm16)
    rc, rs, ro, _ = dst.psy.requantize_to_budget(*dst.psy.unpack(data, index), 682)
    ref = dst.decode_quantized(rc, rs, pcm16)
    assert torch.equal(ro, offset)
    assert _same(got, ref), _where(got, ref)
