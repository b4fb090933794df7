"""Fixed-stride packed rows at a bitrate ("packed rows"): ``AudioCodec.encode_packed_rows``, the
``AC_EMIT_PACKED`` form of ``ac_encode_fused_ex`` behind it, and the one launch at filters_n = 1024 that packs the rows in
the wave that quantised them (k_fwd_fast_qp).

The reference of every GPU comparison is the composition -- ``encode_quantized_budget``, rows longer than their slot marked,
``ac_pack`` at the fixed row starts into zero-filled data -- which runs everywhere while ``AC_ENCODE_PACKED_NOFUSE=1`` is
set.  Every comparison is bit for bit.  The inputs are those of test_encode_cbr (``_input``: a zero frame, NaN, Inf, the 1e15
sample and the 3e12 sample whose row no offset brings under a small budget), at its seeds ``C + 2 B + K``; before any
comparison the composition alone must show what a binding budget shows (``_not_degenerate``).
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

import chip_scale_inputs as csi
from pack_reference import np_canon, np_pack, np_widths
from pack_rows_reference import marked_row, np_pack_rows, np_rows_from_codes, row_bytes
from rate_reference import quantize_budget
from test_encode_cbr import SMALL, UNLIMITED, _input
from test_encode_quantized_fused import _pcm, _same, _where
from test_rate_control import EX_OFF, EX_THR, EX_X

gpu = pytest.mark.gpu
N0 = 1024
CAP = _lib.AC_PACK_ROWS_MAX_BITS
HEADER = os.path.join(ROOT, "include", "audiocodec_amd.h")


# ---- CPU: header, library, Python validation, the numpy restatement -----------------------------------------------
def test_header_declares_the_flag_the_struct_and_the_launch_query():
    text = open(HEADER).read()
    assert re.search(r"\bAC_EMIT_PACKED\s*=\s*8\b", text)
    m = re.search(r"typedef\s+struct\s+ac_packed_out\s*\{(.*?)\}\s*ac_packed_out\s*;", text, flags=re.S)
    assert m, "ac_packed_out is not declared"
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["uint8_t* data", "int64_t row_bytes", "uint8_t* fits"], fields
    m = re.search(r"AC_API\s+int\s+ac_encode_packed_launches\s*\(([^;]*)\)\s*;", text)
    assert m and "stream" not in m.group(1), m and m.group(1)
    m = re.search(r"#define\s+AC_PACK_ROWS_MAX_BITS\s+(\d+)", text)
    assert m and int(m.group(1)) == _lib.AC_PACK_ROWS_MAX_BITS


def test_library_exports_the_launch_query():
    lib = _lib.load()
    assert "ac_encode_packed_launches" in _lib.PROTOTYPES
    assert lib.ac_encode_packed_launches(None, None, 2) == 0
    assert lib.ac_version() == 171
    assert _lib.AC_EMIT_PACKED == 8


def test_ctypes_mirror_has_the_headers_layout():
    P = _lib.PackedOut
    assert [f[0] for f in P._fields_] == ["data", "row_bytes", "fits"]
    assert (P.data.offset, P.row_bytes.offset, P.fits.offset) == (0, 8, 16) and ctypes.sizeof(P) == 24
    assert P.row_bytes.size == 8 and P.data.size == 8 and P.fits.size == 8


def test_the_cap_is_whole_words_and_serves_128_kbit():
    assert CAP % 32 == 0 and CAP >= 2730


def test_python_interface_validates_its_arguments():
    base = audiocodec_amd.AudioCodec(48000, N0)
    assert base.row_bytes is None
    with pytest.raises(ValueError, match=r"with_bitrate\(\)"):
        base.encode_packed_rows(torch.zeros(1, N0, 2))
    assert base.with_bitrate(64000).row_bytes == 172         # ceil(1365 / 32) * 4
    # ceil(320 / 32) * 4: the forty bytes of a row that stores no band (and of the marked row) fill the slot exactly.  A
    # slot of 44 bytes would contradict the layout's row_bytes = ceil(row_bits / 32) * 4, which the decoder's row starts,
    # the C ABI's check of row_bytes and the derived budget R* of test_small_shapes_bit_exact all rest on
    assert base.with_row_budget(320).row_bytes == 40
    assert base.with_row_budget(321).row_bytes == 44
    assert base.row_bytes is None


def test_reference_on_the_worked_example():
    """Section 8c's example (M = 4, off = [0, 0, 2, 5, 8]): every slot is np_pack's row and zero padding."""
    for R in (100, 96, 64, 56, 20):
        data, index, fits, offset, bits = np_pack_rows(EX_X, EX_THR, EX_OFF, R)
        codes, sf, _, rbits = quantize_budget(EX_X, EX_THR, EX_OFF, R)
        dense, _ = np_pack(codes, sf, EX_OFF)
        rb = row_bytes(R)
        assert rb == (R + 31) // 32 * 4 and data.shape == (rb,) and index.ravel().tolist() == [0]
        assert int(rbits.ravel()[0]) <= R and fits.all() and len(dense) <= rb
        np.testing.assert_array_equal(data[:len(dense)], dense)
        assert not data[len(dense):].any()


def test_reference_marks_a_row_that_does_not_fit():
    """A hand-made row with every scale factor at 127 and codes that saturate at every offset, at budget 20."""
    X = np.full((1, 1, 8, 1), 3e38, np.float32)
    X[0, 0, 1::2] = -3e38
    thr = np.full((1, 1, 8, 1), 1e30, np.float32)
    codes, sf, offset, bits = quantize_budget(X, thr, EX_OFF, 20)
    assert sf.ravel().tolist() == [0, 127, 127, 127] and int(offset.ravel()[0]) == 254
    assert int(bits.ravel()[0]) > 8 * row_bytes(20)          # longer than the slot: it may be used as the unfit case
    data, index, fits = np_rows_from_codes(codes, sf, bits, EX_OFF, 20)
    assert not fits.any() and data.shape == (4,)
    np.testing.assert_array_equal(data, [0xFF, 0xFF, 0x0F, 0x00])
    np.testing.assert_array_equal(data, marked_row(4, 20))
    np.testing.assert_array_equal(marked_row(64, 1365)[:41], [0xFF] * 40 + [0])
    w = np_widths(codes, np.full_like(sf, -128), EX_OFF)
    assert (w == 31).all()


# ---- GPU ---------------------------------------------------------------------------------------------------------
class _nofuse:
    """AC_ENCODE_PACKED_NOFUSE=1 (read per call) around a block."""

    def __enter__(self):
        os.environ["AC_ENCODE_PACKED_NOFUSE"] = "1"

    def __exit__(self, *exc):
        del os.environ["AC_ENCODE_PACKED_NOFUSE"]
        return False


def _composition(codec, x, drown=0.0):
    with _nofuse():
        assert codec.encode_packed_rows_launches(x.shape[2]) == codec.encode_launches(x.shape[2]) + 2
        return codec.encode_packed_rows(x, drown)


def _check_result(codec, x, out):
    data, index, fits = out
    B, C = x.shape[0], x.shape[2]
    F = x.shape[1] // codec.filters_n + 1
    rb = codec.row_bytes
    assert data.dtype == torch.uint8 and data.shape == (B * F * C * rb,)
    assert index.dtype == torch.int64 and index.shape == (B, F, C) and fits.dtype == torch.bool and fits.shape == (B, F, C)
    assert torch.equal(index.flatten().cpu(), torch.arange(B * F * C, dtype=torch.int64) * rb)


@gpu
def test_launch_table(monkeypatch):
    for C in (1, 2):
        for spreading in (None, "f32"):
            base = audiocodec_amd.AudioCodec(48000, N0, spreading=spreading)
            assert base.encode_packed_rows_launches(C) == 0                              # no budget
            for R in (320, 1365, 2730, CAP):
                assert base.with_row_budget(R).encode_packed_rows_launches(C) == 1, (C, spreading, R)
            over = base.with_row_budget(CAP + 32)
            assert over.encode_packed_rows_launches(C) == over.encode_launches(C) + 2 == 3
    for N, M, C in ((1024, 64, 3), (2048, 64, 2), (960, 64, 2), (1024, 32, 2)):
        cbr = audiocodec_amd.AudioCodec(48000, N, bark_bands_n=M).with_row_budget(1365)
        assert cbr.encode_packed_rows_launches(C) == cbr.encode_launches(C) + 2 >= 3, (N, M, C)
    cbr = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    monkeypatch.setenv("AC_ENCODE_PACKED_NOFUSE", "1")
    assert cbr.encode_packed_rows_launches(2) == 3 and cbr.encode_packed_rows_launches(1) == 3
    monkeypatch.delenv("AC_ENCODE_PACKED_NOFUSE")
    assert cbr.encode_packed_rows_launches(2) == 1


def _derived_budget(base, x, drown):
    """R* = 32 ceil(b / 32), b the unbudgeted length of one finite row (the median of them): at R* that row sits at offset 0
    and fills the last word of its slot."""
    _, sf, off, bits = base.encode_quantized_budget(x, UNLIMITED, 0, drown)
    assert int(off.abs().max()) == 0
    finite = (sf != -128).all(dim=2)
    b = int(bits[finite].flatten().sort().values[int(finite.sum()) // 2])
    return 32 * ((b + 31) // 32), b


def _not_degenerate(R, kmin, derived, fits, offset, bits, rb):
    """What the composition must show on the injected input, so that a degenerate input cannot pass."""
    padded = (bits.to(torch.int64) + 31) // 32 * 4
    if R in (1365, 320):
        assert int((~fits).sum()) >= 1, "no row that does not fit"
        assert int((fits & (offset > kmin)).sum()) >= 1, "no fitting row above min_offset"
    if derived:
        assert int((fits & (padded == rb)).sum()) >= 1, "no fitting row that fills its slot"
        assert int((fits & (padded <= rb - 4)).sum()) >= 1, "no fitting row shorter than its slot by a word"
        assert int((fits & (offset == kmin) & (padded == rb)).sum()) >= 1, "no row at offset 0 in the slot's last word"


@gpu
@pytest.mark.parametrize("C,spreading,B,K,drown,inject", SMALL)
def test_small_shapes_bit_exact(C, spreading, B, K, drown, inject):
    """Every budget on both edge frames of every clip, a half-empty mono pair (B = 3 mono), K = 5, 1 and 0, an all-zero frame,
    NaN, Inf, a row that does not fit (the 3e12 sample) and, at the derived budget, rows that fill the last word of their
    slot.  Seeds: test_encode_cbr's, C + 2 B + K."""
    base = audiocodec_amd.AudioCodec(48000, N0, spreading=spreading)
    x = _input(C, B, K, C + 2 * B + K, inject)
    off = base.psy.scale_band_offsets
    Rs, b = _derived_budget(base, x, drown)
    assert Rs <= CAP, (Rs, b)
    for R, kmin, derived in [(1365, 0, False), (2730, -8, False), (320, 0, False), (CAP, 0, False), (Rs, 0, True)]:
        cbr = base.with_row_budget(R, kmin)
        rb = cbr.row_bytes
        assert cbr.encode_packed_rows_launches(C) == 1
        rc, rs, ro, rbits = base.encode_quantized_budget(x, R, kmin, drown)
        comp = _composition(cbr, x, drown)
        _check_result(cbr, x, comp)
        assert torch.equal(comp[2], rbits <= 8 * rb)
        print("R=%d kmin=%d row_bytes=%d: %d rows, %d do not fit, %d fitting above kmin, longest %d bits"
              % (R, kmin, rb, ro.numel(), int((~comp[2]).sum()), int((comp[2] & (ro > kmin)).sum()), int(rbits.max())))
        if inject:
            _not_degenerate(R, kmin, derived, comp[2], ro, rbits, rb)
        fused = cbr.encode_packed_rows(x, drown)
        _check_result(cbr, x, fused)
        assert torch.equal(fused[2], comp[2]), (R, kmin, _where(fused[2], comp[2]))
        assert torch.equal(fused[0], comp[0]), (R, kmin, _where(fused[0], comp[0]))
        # the rows read back: the canonical codes and sf where the row fits, bands that could not be represented elsewhere
        uc, us = cbr.psy.unpack(fused[0], fused[1])
        cc, cs = np_canon(rc.cpu().numpy(), rs.cpu().numpy(), off)
        fit = fused[2].cpu().numpy()
        uc, us = uc.cpu().numpy(), us.cpu().numpy()
        np.testing.assert_array_equal(us[np.broadcast_to(fit[:, :, None, :], us.shape)],
                                      cs[np.broadcast_to(fit[:, :, None, :], cs.shape)])
        np.testing.assert_array_equal(uc[np.broadcast_to(fit[:, :, None, :], uc.shape)],
                                      cc[np.broadcast_to(fit[:, :, None, :], cc.shape)])
        assert (us[np.broadcast_to(~fit[:, :, None, :], us.shape)] == -128).all()
        assert not uc[np.broadcast_to(~fit[:, :, None, :], uc.shape)].any()
        if not fit.all():                                    # the marked row, byte for byte
            r = int(np.flatnonzero(~fit.ravel())[0])
            np.testing.assert_array_equal(fused[0][r * rb:(r + 1) * rb].cpu().numpy(), marked_row(64, R))


@gpu
def test_numpy_restatement():
    base = audiocodec_amd.AudioCodec(48000, N0)
    x = _input(2, 3, 5, 13, True)
    X, _, thr = base.encode(x)
    data, index, fits, offset, bits = np_pack_rows(X.cpu().numpy(), thr.cpu().numpy(), base.psy.scale_band_offsets, 1365, 0)
    assert (~fits).sum() >= 1 and (fits & (offset > 0)).sum() >= 1
    got = base.with_bitrate(64000).encode_packed_rows(x)
    np.testing.assert_array_equal(got[2].cpu().numpy(), fits)
    np.testing.assert_array_equal(got[1].cpu().numpy(), index)
    np.testing.assert_array_equal(got[0].cpu().numpy(), data)


@gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("pcm16", [False, True])
def test_round_trip(C, pcm16):
    base = audiocodec_amd.AudioCodec(48000, N0)
    cbr = base.with_bitrate(64000)
    x = _pcm(N0, C, 3, 5, seed=30 + C, inject=True)          # zero frame, NaN, Inf; none of the large samples
    data, index, fits = cbr.encode_packed_rows(x)
    assert cbr.encode_packed_rows_launches(C) == 1 and bool(fits.all())
    got = cbr.decode_packed(data, index, pcm16)
    ref = cbr.decode_quantized(*cbr.encode_quantized(x), pcm16)
    assert _same(got, ref), _where(got, ref)


@gpu
def test_rows_that_do_not_fit_decode_as_unrepresentable_bands():
    cbr = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(320)
    x = _input(2, 3, 5, 11, True)
    data, index, fits = cbr.encode_packed_rows(x)
    assert int((~fits).sum()) >= 1
    b, f, c = (int(i) for i in torch.nonzero(~fits)[0])
    pcm = cbr.decode_packed(data, index)
    assert bool(torch.isnan(pcm[b, f * N0:(f + 2) * N0, c]).all())
    assert int(cbr.decode_packed(data, index, pcm16=True)[b, f * N0:(f + 2) * N0, c].abs().max()) == 0


@gpu
@pytest.mark.parametrize("C", [2, 1])
def test_chip_filling(C):
    """>= 2048 workgroups of 4 waves x 4 frames (test_encode_cbr's shapes), against the composition in the same process."""
    cbr = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    K = csi.blocks_per_clip(N0)
    B = csi.clips_for(N0, C, tasks_per_workgroup=16)
    x = csi.structured(B, K, N0, C, seed=500 + C)
    assert cbr.encode_packed_rows_launches(C) == 1
    fused = cbr.encode_packed_rows(x)
    comp = _composition(cbr, x)
    assert torch.equal(fused[2], comp[2]) and torch.equal(fused[1], comp[1])
    assert torch.equal(fused[0], comp[0]), _where(fused[0], comp[0])
    assert int(fused[0].max()) > 0 and bool(fused[2].any())


@gpu
def test_an_empty_batch_gives_empty_results():
    cbr = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    data, index, fits = cbr.encode_packed_rows(torch.zeros((0, 2 * N0, 2), device="cuda"))
    assert data.shape == (0,) and index.shape == (0, 3, 2) and fits.shape == (0, 3, 2) and fits.dtype == torch.bool


def _emit_packed(codec, x, data, fits, rb, flags=None, X=None, t=None, thr=None, out1=None, B=None):
    lib = _lib.load()
    dev = x.device
    K = x.shape[1] // codec.filters_n
    out = _lib.PackedOut(data.data_ptr(), rb, fits.data_ptr())

    def p(v):
        return ctypes.c_void_p(v.data_ptr()) if v is not None else None
    st = lib.ac_encode_fused_ex(codec.mdct._plan(dev), codec.psy._plan(dev), p(x), p(X), p(t), p(thr), 0.0,
                                _lib.AC_EMIT_PACKED if flags is None else flags, ctypes.addressof(out), p(out1), 0,
                                x.shape[0] if B is None else B, K, x.shape[2], None)
    torch.cuda.synchronize()
    return st


@gpu
def test_c_abi():
    lib = _lib.load()
    base = audiocodec_amd.AudioCodec(48000, N0)
    cbr = base.with_row_budget(1365)
    x = _input(2, 3, 5, 17, True)
    rows, rb = 3 * 6 * 2, cbr.row_bytes
    data = torch.full((rows * rb,), 0xA5, dtype=torch.uint8, device=x.device)
    fits = torch.full((rows,), 7, dtype=torch.uint8, device=x.device)
    spare = torch.zeros((3, 6, N0, 2), device=x.device)
    assert _emit_packed(cbr, x, data, fits, rb) == _lib.AC_OK, lib.ac_last_error()
    ref = _composition(cbr, x)
    assert torch.equal(data, ref[0]) and torch.equal(fits.view(3, 6, 2), ref[2].to(torch.uint8))
    for kw in ({"X": spare}, {"t": spare}, {"thr": spare}, {"out1": spare}):
        assert _emit_packed(cbr, x, data, fits, rb, **kw) == _lib.AC_EINVAL, kw
    assert _emit_packed(cbr, x, data, fits, rb + 4) == _lib.AC_EINVAL and b"row_bytes" in lib.ac_last_error()
    assert _emit_packed(base, x, data, fits, rb) == _lib.AC_EINVAL and b"row budget" in lib.ac_last_error()
    for other in (_lib.AC_EMIT_NOISY, _lib.AC_EMIT_DB_NORM, _lib.AC_EMIT_CODES):
        assert _emit_packed(cbr, x, data, fits, rb, flags=_lib.AC_EMIT_PACKED | other) == _lib.AC_EINVAL
    assert _emit_packed(cbr, x, data, fits, rb, B=0) == _lib.AC_OK
    wide = audiocodec_amd.AudioCodec(48000, 2048).with_row_budget(1365)
    x2 = _pcm(2048, 2, 1, 1, seed=3, inject=False)
    d2 = torch.zeros((1 * 2 * 2 * rb,), dtype=torch.uint8, device=x.device)
    assert _emit_packed(wide, x2, d2, fits, rb) == _lib.AC_EUNSUPPORTED
    assert b"composition" in lib.ac_last_error()
    assert torch.equal(data, ref[0])                         # the refused calls wrote nothing


@pytest.fixture(scope="module")
def harness():
    from stream_order import Harness
    return Harness()


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
@pytest.mark.parametrize("check", ["delayed_producer", "busy_default"])
def test_stream_contract(harness, check, route):
    cbr = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    assert cbr.encode_packed_rows_launches(2) == 1
    x = _pcm(N0, 2, 4, 20, seed=77, inject=False)
    fn = (lambda x: cbr.encode_packed_rows(x)) if route == "fused" else (lambda x: _composition(cbr, x))
    getattr(harness, check)("cbr.encode_packed_rows[1024-2,%s]" % route, ([x], fn))


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
def test_graph_capture(route):
    """One eager call (plans, allocator), then a linear capture on one stream, replayed on new contents of the same x."""
    cbr = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    call = (lambda v: cbr.encode_packed_rows(v)) if route == "fused" else (lambda v: _composition(cbr, v))
    x = _input(2, 3, 5, 5, True)
    call(x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(x)
    for seed in (6, 7):
        x.copy_(_input(2, 3, 5, seed, True))
        g.replay()
        torch.cuda.synchronize()
        ref = call(x.clone())
        assert int((~ref[2]).sum()) >= 1 and int(ref[0].max()) > 0
        for got, want in zip(out, ref):
            assert torch.equal(got, want), (seed, _where(got, want))
