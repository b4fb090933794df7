"""The argument checks that the C ABI states once and several entry points share: what each refuses, with which text, and
which message wins where two faults are present at once.

Every call here is refused before any launch, so a case costs a ctypes call.  The four readers of an ``ac_packed_rows``
-- ``ac_decode_quantized`` (sf == NULL), ``ac_encode_fused_ex`` under ``AC_IN_PACKED | AC_EMIT_PACKED``, and
``ac_stream_inverse_typed`` under ``AC_PACKED`` and under ``AC_PACKED | AC_CONCEAL`` -- report a negative ``nbytes``, then a
NULL tensor, then a NULL ``data``, then a misaligned address, in that order and in the same words.  Texts and order are those
the entry points had while each carried its own copy of these checks, so this file passes on a library from before they were
shared and on one after.

The same holds for the size refusals of the generic launchers at the end of the file: one launcher per kernel family serves every
dtype, and which text a dtype gets ("float64 kernel", "generic kernel", "backward kernel") is what these cases pin.
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


# ---- the size refusals of the generic launchers ---------------------------------------------------------------------------------
# Each kernel below the LDS-FFT tier keeps its working set in at most LDS_BOUND bytes of LDS, in the arithmetic type (8 bytes for
# float64 tensors, 4 for float32 and the 2-byte types): the O(N^2) analysis one frame of filters_n values, the synthesis two, the
# generic threshold filter_bands_n + 2 bark_bands_n values, its backward 2 filter_bands_n + 10 bark_bands_n.  Every size below is
# derived from that; a call is one clip, one block, one channel.
LDS_BOUND = 64 * 1024
PLAN_MAX_N, PLAN_MAX_M = 8192, 4096   # the largest filters_n / filter_bands_n and bark_bands_n a plan is made for
M_SMALL = 8                            # a band count the suite runs elsewhere (test_psy_alpha.py)


def _first_even_filters_n(bytes_per_filter):
    """The first even filters_n whose working set of bytes_per_filter * filters_n bytes is above LDS_BOUND."""
    n = LDS_BOUND // bytes_per_filter + 1
    return n + (n & 1)


def _smooth5(h):
    for r in (2, 3, 5):
        while h % r == 0:
            h //= r
    return h == 1


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _expect_einval(status, text):
    got = _lib.load().ac_last_error().decode()
    assert status == _lib.AC_EINVAL and got == text, (status, got, text)


def _float64_inverse(n):
    """Status of ac_mdct_inverse_typed on one float64 frame of n filters (ctypes: MDCTransformer.inverse_transform refuses
    float64 above 4096 itself, with a text of its own)."""
    mdct = audiocodec_amd.MDCTransformer(n, compute_dtype=torch.float64)
    X = torch.zeros((1, 1, n, 1), dtype=torch.float64, device=_device())
    x = torch.zeros((1, 2 * n, 1), dtype=torch.float64, device=_device())
    st = mdct._lib.ac_mdct_inverse_typed(mdct._plan(_device()), ctypes.c_void_p(X.data_ptr()), ctypes.c_void_p(x.data_ptr()),
                                         mdct._dtype_id, 1, 1, 1, None)
    torch.cuda.synchronize()
    return st


@gpu
def test_float64_synthesis_refuses_past_two_frames_of_lds():
    """launch_inv_T<double>: 16 bytes per filter.  4098 is refused in the float64 kernel's words, 4096 is served."""
    n = _first_even_filters_n(16)
    assert n == 4098
    _expect_einval(_float64_inverse(n), "filters_n = %d too large for the float64 kernel" % n)
    assert _float64_inverse(n - 2) == _lib.AC_OK


@gpu
@pytest.mark.parametrize("what, bytes_per_filter", [("float64 analysis", 8), ("float32 analysis", 4), ("float32 synthesis", 8)])
def test_plan_creation_refuses_first_what_these_launchers_would(what, bytes_per_filter):
    """Not cases of the launchers: the first even filters_n past the bound of the float64 analysis (8194) and of the float32
    synthesis (8194) and analysis (16386) -- halves not 5-smooth, so the O(N^2) kernels would be the ones reached -- are above the
    8192 that ac_mdct_plan_create admits, and it refuses with its own text.  "filters_n = %d too large for the float64 / generic
    kernel" cannot be reached through the C ABI for these three."""
    n = _first_even_filters_n(bytes_per_filter)
    assert n > PLAN_MAX_N and not _smooth5(n // 2)
    out = ctypes.c_void_p()
    st = _lib.load().ac_mdct_plan_create(n, _lib.window_id("vorbis"), torch.cuda.current_device(), ctypes.byref(out))
    _expect_einval(st, "filters_n = %d not supported (max %d)" % (n, PLAN_MAX_N))
    assert not out.value


@gpu
def test_float64_analysis_serves_the_largest_plan():
    """launch_fwd_T<double>: 8 bytes per filter, so filters_n = 8192 fills the bound exactly and is served."""
    assert 8 * PLAN_MAX_N == LDS_BOUND
    mdct = audiocodec_amd.MDCTransformer(PLAN_MAX_N, compute_dtype=torch.float64)
    X = mdct.transform(torch.zeros((1, PLAN_MAX_N, 1), dtype=torch.float64, device=_device()))
    torch.cuda.synchronize()
    assert tuple(X.shape) == (1, 2, PLAN_MAX_N, 1)


def _threshold(n, dtype, backward):
    """The generic threshold (or its backward) on one frame of n filters and M_SMALL bands through PsychoacousticModel."""
    model = audiocodec_amd.PsychoacousticModel(48000, n, M_SMALL, compute_dtype=dtype)
    X = torch.full((1, 1, n, 1), 0.5, dtype=dtype, device=_device())
    t = torch.full((1, 1, 1, 1), 0.5, dtype=dtype, device=_device())
    out = model._threshold_backward(X, t, 0.0, torch.ones_like(X)) if backward else model.global_masking_threshold(X, t)
    torch.cuda.synchronize()
    return out


@gpu
@pytest.mark.parametrize("dtype, backward, words, kernel", [
    (torch.float64, False, lambda n, m: n + 2 * m, "float64"),
    (torch.float64, True, lambda n, m: 2 * n + 10 * m, "backward"),
    (torch.float32, True, lambda n, m: 2 * n + 10 * m, "backward"),
], ids=["float64-forward", "float64-backward", "float32-backward"])
def test_generic_threshold_refuses_past_its_lds(dtype, backward, words, kernel):
    """launch_threshold_T<double> names the float64 kernel, launch_threshold_bwd_T the backward kernel in every dtype.  The
    largest even filter_bands_n whose working set fits the bound at 8 bands is served, the next even one refused (ValueError is
    what the package makes of AC_EINVAL)."""
    size = 8 if dtype == torch.float64 else 4
    n = max(n for n in range(2, PLAN_MAX_N + 1, 2) if words(n, M_SMALL) * size <= LDS_BOUND)
    assert n + 2 <= PLAN_MAX_N and words(n + 2, M_SMALL) * size > LDS_BOUND
    _threshold(n, dtype, backward)
    with pytest.raises(ValueError) as e:
        _threshold(n + 2, dtype, backward)
    assert str(e.value) == "filter_bands_n = %d / bark_bands_n = %d too large for the %s kernel" % (n + 2, M_SMALL, kernel)


@gpu
def test_plan_creation_refuses_first_what_the_float32_arithmetic_threshold_would():
    """Not a case of the launcher: float32 and bfloat16 tensors (float32 arithmetic) cross the bound at filter_bands_n +
    2 bark_bands_n > 16384, and the largest plan, 8192 filters and 4096 bands, has exactly 16384.  One band more is refused by
    ac_psy_plan_create with its own text; "... too large for the generic kernel" cannot be reached through the C ABI."""
    assert (PLAN_MAX_N + 2 * PLAN_MAX_M) * 4 == LDS_BOUND
    out = ctypes.c_void_p()
    st = _lib.load().ac_psy_plan_create(PLAN_MAX_N, PLAN_MAX_M + 1, 48000.0, 0.6, torch.cuda.current_device(), ctypes.byref(out))
    _expect_einval(st, "filter_bands_n = %d / bark_bands_n = %d not supported" % (PLAN_MAX_N, PLAN_MAX_M + 1))
    assert not out.value
