"""The argument checks that the C ABI states once and several entry points share: what each refuses, with which text, and
which message wins where two faults are present at once.

Every call here is refused before any launch, so a case costs a ctypes call.  The four readers of an ``ac_packed_rows``
-- ``ac_decode_quantized`` (sf == NULL), ``ac_encode_fused_ex`` under ``AC_IN_PACKED | AC_EMIT_PACKED``, and
``ac_stream_inverse_typed`` under ``AC_PACKED`` and under ``AC_PACKED | AC_CONCEAL`` -- report a negative ``nbytes``, then a
NULL tensor, then a NULL ``data``, then a misaligned address, in that order and in the same words.  Texts and order are those
the entry points had while each carried its own copy of these checks, so this file passes on a library from before they were
shared and on one after.
"""

import ctypes

import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib

gpu = pytest.mark.gpu
N0, KP, C0, BUDGET = 1024, 2, 2, 1365
NOFUSE = ("AC_DECODE_PACKED_NOFUSE", "AC_TRANSRATE_NOFUSE", "AC_ENCODE_PACKED_NOFUSE", "AC_ENCODE_QUANT_NOFUSE")
READERS = ("decode", "transrate", "stream", "stream_conceal")


class _Case:
    """One codec with a row budget at filters_n = 1024, 64 bands; B = 1, C = 2, K' = 2 rows per channel."""

    def __init__(self):
        self.lib = _lib.load()
        self.codec = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(BUDGET)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.mdct, self.psy = self.codec.mdct._plan(dev), self.codec.psy._plan(dev)
        self.stream = self.codec.stream(1, C0)
        rows, rb = KP * C0, self.codec.row_bytes
        self.data = torch.zeros((rows * rb + 16,), dtype=torch.uint8, device=dev)
        self.index = (torch.arange(rows, dtype=torch.int64, device=dev) * rb).view(1, KP, C0)
        self.lost = torch.zeros((1, KP, C0), dtype=torch.uint8, device=dev)
        self.x = torch.zeros((1, KP * N0, C0), device=dev)
        self.out = torch.zeros((rows * rb,), dtype=torch.uint8, device=dev)
        self.fits = torch.zeros((rows,), dtype=torch.uint8, device=dev)
        self.rb = rb

    def call(self, reader, data="ok", nbytes=None, index="ok", lost="ok", max_age=8, pcm16=0):
        """Status of one call of `reader` on rows (data, nbytes, index); "ok": the valid value."""
        data = self.data.data_ptr() if data == "ok" else data
        index = self.index.data_ptr() if index == "ok" else index
        lost = self.lost.data_ptr() if lost == "ok" else lost
        rows = _lib.PackedRows(data, self.data.numel() - 16 if nbytes is None else nbytes, index)
        x = ctypes.c_void_p(self.x.data_ptr())
        if reader == "decode":
            return self.lib.ac_decode_quantized(self.mdct, self.psy, ctypes.addressof(rows), None, x, None, None, 1, KP, C0, None)
        if reader == "transrate":
            po = _lib.PackedOut(self.out.data_ptr(), self.rb, self.fits.data_ptr())
            return self.lib.ac_encode_fused_ex(self.mdct, self.psy, ctypes.addressof(rows), None, None, None, 0.0,
                                               _lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED, ctypes.addressof(po), None, 0, 1, KP - 1,
                                               C0, None)
        pin = _lib.StreamPackedIn(rows, self.psy.value, pcm16)
        if reader == "stream":
            return self.lib.ac_stream_inverse_typed(self.stream._handle, ctypes.addressof(pin), x, _lib.AC_PACKED, KP, None)
        assert reader == "stream_conceal"
        lin = _lib.StreamPackedLostIn(pin, lost, max_age)
        return self.lib.ac_stream_inverse_typed(self.stream._handle, ctypes.addressof(lin), x, _lib.AC_PACKED | _lib.AC_CONCEAL,
                                                KP, None)

    def refused(self, status, text):
        got = self.lib.ac_last_error().decode()
        assert status == _lib.AC_EINVAL and got == text, (status, got, text)


@pytest.fixture(scope="module")
def case():
    return _Case()


@pytest.fixture(autouse=True)
def _fused(monkeypatch):
    for name in NOFUSE:   # (the hooks are read per call; with one set, a reader refuses every call as unsupported first)
        monkeypatch.delenv(name, raising=False)


def _unaligned(addr):
    return "tensor address 0x%x is not 16-byte aligned (pass the start of an allocation or an aligned view)" % addr


@gpu
@pytest.mark.parametrize("reader", READERS)
def test_the_readers_serve_this_configuration(case, reader):
    """The precondition of every case below: the reader has its one launch here, so none of them ends as AC_EUNSUPPORTED."""
    lib = case.lib
    got = {"decode": lib.ac_decode_packed_launches(case.mdct, case.psy, C0), "transrate": lib.ac_transrate_launches(case.psy, C0),
           "stream": lib.ac_stream_packed_launches(case.stream._handle, case.psy, 1),
           "stream_conceal": lib.ac_stream_packed_launches(case.stream._handle, case.psy, 2)}[reader]
    assert got == 1


@gpu
@pytest.mark.parametrize("reader", READERS)
def test_negative_nbytes(case, reader):
    case.refused(case.call(reader, nbytes=-1), "negative nbytes (-1)")


@gpu
@pytest.mark.parametrize("reader", READERS)
def test_null_index(case, reader):
    case.refused(case.call(reader, index=None), "NULL tensor pointer")


@gpu
@pytest.mark.parametrize("reader", READERS)
def test_null_data_with_bytes_to_read(case, reader):
    case.refused(case.call(reader, data=None), "data is NULL")


@gpu
@pytest.mark.parametrize("reader", READERS)
def test_misaligned_data(case, reader):
    addr = case.data.data_ptr() + 4
    case.refused(case.call(reader, data=addr), _unaligned(addr))


@gpu
@pytest.mark.parametrize("reader", READERS)
def test_negative_nbytes_wins_over_null_index(case, reader):
    case.refused(case.call(reader, nbytes=-1, index=None), "negative nbytes (-1)")


@gpu
def test_concealing_stream_max_age_wins_over_null_lost(case):
    case.refused(case.call("stream_conceal", lost=None, max_age=32), "ac_stream_packed_lost_in: max_age (32) outside [0, 31]")


@gpu
def test_concealing_stream_pcm16_wins_over_max_age(case):
    case.refused(case.call("stream_conceal", pcm16=2, max_age=32), "ac_stream_packed_in: pcm16 must be 0 or 1 (got 2)")


@gpu
def test_nothing_was_written(case):
    """The refused calls above launched nothing: the outputs are as they were made."""
    torch.cuda.synchronize()
    assert not case.x.any() and not case.out.any() and not case.fits.any()


@gpu
def test_mono_at_2048_takes_two_launches():
    """filters_n = 2048: mono input is two launches (the fused kernel would spill registers), stereo one."""
    codec = audiocodec_amd.AudioCodec(48000, 2048)
    assert codec.encode_launches(1) == 2 and codec.encode_launches(2) == 1
