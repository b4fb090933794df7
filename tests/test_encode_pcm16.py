"""16-bit PCM straight into the quantising encodes at filters_n = 1024: k_fwd_fast_q16 / qb16 / qp16 / qps16 behind
``encode_quantized(int16)``, ``encode_packed_rows(int16)``, ``StreamingMDCT.encode_packed_rows_chunk(int16)``, the
``AC_IN_PCM16`` flag of ``ac_encode_fused_ex`` / ``ac_stream_encode_typed`` and the three ``*_launches_pcm16`` queries.

Definition: for int16 PCM p every path gives, bit for bit, what the float32 public path gives on ``p.float() / 32768`` (exact
in float32).  That float32 path is the reference of every GPU test here; its own tests hold it to the numpy restatements.
int16 cannot produce NaN, Inf or a marked row: the references assert that every ``fits`` is True, and the float tests keep
covering marked rows."""

import ctypes
import functools
import inspect
import itertools
import os
import re

import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib
from audiocodec_amd.codec import StreamingMDCT
from conftest import ROOT

import chip_scale_inputs as csi
from test_encode_packed_rows import CAP
from test_encode_quantized_fused import _pcm, _same, _where
from test_stream_packed import _bounds, _env, _hostless

gpu = pytest.mark.gpu
N0 = 1024
B0, K0 = 3, 7
HEADER = os.path.join(ROOT, "include", "audiocodec_amd.h")
Q_NOFUSE, P_NOFUSE = "AC_ENCODE_QUANT_NOFUSE", "AC_ENCODE_PACKED_NOFUSE"
CODE_BUDGETS = [None, (1365, 0), (2730, -8)]                     # (row_bits, min_offset)
ROW_BUDGETS = [(1365, 0), (2730, -8), (320, 0), (CAP, 0)]
CHUNKINGS = [(7,), (1,) * 7, (2, 3, 2)]
ELSEWHERE = [(960, 64, 2, 1365), (2048, 64, 2, 1365), (1024, 32, 2, 1365), (1024, 64, 3, 1365), (1024, 64, 2, CAP + 32)]
FAMILIES = {"q16": rb"14k_fwd_fast_q16", "qb16": rb"15k_fwd_fast_qb16", "qp16": rb"15k_fwd_fast_qp16",
            "qps16": rb"16k_fwd_fast_qps16"}
QUERIES = ("ac_encode_quantized_launches_pcm16", "ac_encode_packed_launches_pcm16", "ac_stream_packed_launches_pcm16")


# ---- CPU: header, library, Python validation -----------------------------------------------------------------------
def test_header_declares_the_flag_and_the_queries():
    text = open(HEADER).read()
    assert re.search(r"\bAC_IN_PCM16\s*=\s*32\b", text)
    want = {QUERIES[0]: "const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C",
            QUERIES[1]: "const ac_mdct_plan* mdct, const ac_psy_plan* psy, int C",
            QUERIES[2]: "const ac_stream* s, const ac_psy_plan* psy"}
    for name, params in want.items():
        m = re.search(r"AC_API\s+int\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, "%s is not declared" % name
        assert "stream" not in m.group(1).replace("ac_stream", ""), m.group(1)      # no void* stream: they launch nothing
        assert " ".join(m.group(1).split()) == params
    assert re.search(r"#define\s+AC_VERSION\s+171\b", text)


def test_library_exports_the_queries():
    lib = _lib.load()
    for name in QUERIES:
        assert name in _lib.PROTOTYPES
    assert lib.ac_encode_quantized_launches_pcm16(None, None, 2) == 0
    assert lib.ac_encode_packed_launches_pcm16(None, None, 2) == 0
    assert lib.ac_stream_packed_launches_pcm16(None, None) == 0
    assert lib.ac_version() == 171
    assert _lib.AC_IN_PCM16 == 32 and _lib.AC_PACKED | _lib.AC_IN_PCM16 == 48


def test_forty_eight_is_no_dtype_elsewhere():
    lib = _lib.load()
    assert lib.ac_mdct_forward_typed(None, None, None, 48, 1, 1, 1, None) == _lib.AC_EINVAL
    assert b"dtype = 48" in lib.ac_last_error()
    assert lib.ac_encode_fused_typed(None, None, None, None, None, None, 0.0, 48, 1, 1, 1, None) == _lib.AC_EINVAL
    assert lib.ac_stream_inverse_typed(None, None, None, 48, 1, None) == _lib.AC_EINVAL
    # the stream encode takes the value: it checks its own arguments
    assert lib.ac_stream_encode_typed(None, None, None, None, None, None, 0.0, 48, 1, None) == _lib.AC_EINVAL
    assert b"stream is NULL" in lib.ac_last_error()


def test_python_queries_take_the_keyword():
    for cls, name in ((audiocodec_amd.AudioCodec, "encode_quantized_launches"),
                      (audiocodec_amd.AudioCodec, "encode_packed_rows_launches"), (StreamingMDCT, "packed_chunk_launches")):
        p = inspect.signature(getattr(cls, name)).parameters
        assert "pcm16" in p and p["pcm16"].default is False and list(p)[-1] == "pcm16", name


def test_int16_passes_the_argument_checks():
    """As far as a machine without a device reaches: an int16 tensor gets past the dtype check to the device check; other
    integer types stop at the dtype check as before."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    cbr = base.with_row_budget(1365)
    p = torch.zeros((1, N0, 2), dtype=torch.int16)
    with pytest.raises(RuntimeError, match="lives on cpu"):
        cbr.encode_packed_rows(p)
    with pytest.raises(RuntimeError, match="lives on cpu"):
        _hostless(cbr).encode_packed_rows_chunk(p)
    for bad in (p.to(torch.int32), p.to(torch.uint8), p.double()):
        with pytest.raises(ValueError, match="dtype"):
            cbr.encode_packed_rows(bad)
        with pytest.raises(ValueError, match="dtype"):
            _hostless(cbr).encode_packed_rows_chunk(bad)
    with pytest.raises(ValueError, match=r"with_bitrate\(\)"):
        base.encode_packed_rows(p)
    f64 = audiocodec_amd.AudioCodec(48000, N0, compute_dtype=torch.float64)
    for call in (lambda: f64.encode_quantized(p), lambda: f64.encode_packed_rows(p),
                 lambda: _hostless(f64).encode_packed_rows_chunk(p)):
        with pytest.raises(NotImplementedError, match="float32"):
            call()


# ---- GPU: input and references (computed once, never modified) -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _p16(C, B=B0, K=K0, N=N0):
    """int16 PCM [B, K N, C]: the ramped noise of _pcm through round(x * 32767); with B >= 3 and K >= 4 two all-zero blocks in
    clip 1 and both rails at fixed samples of clips 0 and 2."""
    x = _pcm(N, C, B, K, seed=C + 2 * B + K, inject=False)
    p = torch.round(x * 32767).to(torch.int16)
    if B >= 3 and K >= 4:
        p[1, N:3 * N] = 0
        p[0, 2 * N + 17, 0] = -32768
        p[0, 2 * N + 18, C - 1] = 32767
        p[2, 3 * N + 5, C - 1] = 32767
        p[2, 3 * N + 6, 0] = -32768
    return p


def _f32(p):
    return p.to(torch.float32) / 32768


@functools.lru_cache(maxsize=None)
def _codec(spreading, budget, N=N0, M=64):
    c = audiocodec_amd.AudioCodec(48000, N, bark_bands_n=M, spreading=spreading)
    return c if budget is None else c.with_row_budget(*budget)


@functools.lru_cache(maxsize=None)
def _built(family):
    """(CMODE, SPREAD) of the instances of a new family in the library file (see test_stream_packed._built)."""
    with open(_lib.LIB_PATH, "rb") as f:
        names = re.findall(FAMILIES[family] + rb"ILi(\d)ELi(\d)E", f.read())
    return {(int(c), int(sp)) for c, sp in names}


def _instance(codec, C):
    return ((0 if C == 2 else 2), codec.psy.SPREADING[codec.psy.plan_spreading()])


@functools.lru_cache(maxsize=None)
def _ref_rows(C, spreading, budget, N=N0, M=64):
    """(rows uint8 [B, K+1, C, row_bytes], fits, data, index) of the float32 one-shot encode of _p16(C) / 32768."""
    cbr = _codec(spreading, budget, N, M)
    data, index, fits = cbr.encode_packed_rows(_f32(_p16(C, N=N)))
    assert bool(fits.all()), "int16 PCM gave a marked row: the float tests cover those"
    return data.view(B0, K0 + 1, C, cbr.row_bytes), fits, data, index


# ---- 1. codes ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("budget", CODE_BUDGETS)
@pytest.mark.parametrize("spreading", [None, "f32"])
@pytest.mark.parametrize("C", [1, 2])
def test_codes(C, spreading, budget):
    codec = _codec(spreading, budget)
    fam = "q16" if budget is None else "qb16"
    one = _instance(codec, C) in _built(fam)
    assert codec.encode_quantized_launches(C, pcm16=True) == (1 if one else 2)
    assert codec.encode_quantized_launches(C) == 1
    for B, K in ((B0, K0), (1, 1), (2, 0)):                      # B = 3 mono: a half-empty pair
        p = _p16(C, B, K)
        rc, rs = codec.encode_quantized(_f32(p))
        codes, sf = codec.encode_quantized(p)
        assert codes.dtype == torch.int16 and codes.shape == (B, K + 1, N0, C) and sf.shape == (B, K + 1, 64, C)
        assert torch.equal(sf, rs), (B, K, _where(sf, rs))
        assert torch.equal(codes, rc), (B, K, _where(codes, rc))
        assert not bool((rs == -128).any()), "int16 PCM gave a band the quantiser cannot represent"
        assert (int(rc.abs().max()) > 0) == (K > 0)              # K = 0: silence
    if budget is not None and budget[0] == 1365:                 # the budget binds, on the reference alone
        _, _, off, _ = codec.encode_quantized_budget(_f32(_p16(C)), *budget)
        assert int((off == budget[1]).sum()) >= 1, "no row at min_offset"
        assert int((off > budget[1]).sum()) >= 1, "no row above min_offset"


# ---- 2. rows ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("budget", ROW_BUDGETS)
@pytest.mark.parametrize("spreading", [None, "f32"])
@pytest.mark.parametrize("C", [1, 2])
def test_rows(C, spreading, budget):
    cbr = _codec(spreading, budget)
    one = _instance(cbr, C) in _built("qp16")
    assert cbr.encode_packed_rows_launches(C, pcm16=True) == (1 if one else cbr.encode_launches(C) + 2)
    ref_rows, ref_fits, ref_data, ref_index = _ref_rows(C, spreading, budget)
    data, index, fits = cbr.encode_packed_rows(_p16(C))
    assert data.dtype == torch.uint8 and fits.dtype == torch.bool and index.dtype == torch.int64
    assert torch.equal(index, ref_index) and torch.equal(fits, ref_fits)
    assert torch.equal(data, ref_data), _where(data, ref_data)
    assert int(data.max()) > 0 or budget[0] == 320
    # the round trip of the issue: rows of int16 PCM back to int16 PCM
    back = cbr.decode_packed(data, index, pcm16=True)
    assert back.dtype == torch.int16 and torch.equal(back, cbr.decode_packed(ref_data, ref_index, pcm16=True))


# ---- 3. chunks --------------------------------------------------------------------------------------------------------
def _encode_chunks(st, p, chunks):
    """The rows [B, K + 1, C, row_bytes] and fits of the chunks of p, then a flush chunk of one zero block."""
    C, rb = p.shape[2], st.row_bytes
    parts = [p[:, a * N0:b * N0] for a, b in _bounds(chunks)] + [torch.zeros_like(p[:, :N0])]
    rows, fits = [], []
    for part in parts:
        k = part.shape[1] // N0
        d, i, f = st.encode_packed_rows_chunk(part)
        assert d.dtype == torch.uint8 and d.shape == (B0 * k * C * rb,) and f.dtype == torch.bool and f.shape == (B0, k, C)
        assert torch.equal(i.flatten().cpu(), torch.arange(B0 * k * C, dtype=torch.int64) * rb)
        rows.append(d.view(B0, k, C, rb))
        fits.append(f)
    return torch.cat(rows, dim=1), torch.cat(fits, dim=1)


@gpu
@pytest.mark.parametrize("spreading", [None, "f32"])
@pytest.mark.parametrize("C", [1, 2])
def test_chunks(C, spreading):
    p = _p16(C)
    for budget in ROW_BUDGETS:
        cbr = _codec(spreading, budget)
        ref_rows, ref_fits, _, _ = _ref_rows(C, spreading, budget)
        one = _instance(cbr, C) in _built("qps16")
        for chunks in CHUNKINGS:
            for a, b in _bounds(chunks)[1:]:                     # the state matters at every boundary (not at 320 bits: a row
                if budget[0] > 5 * 64:                           # is its 64 width fields there, see test_stream_packed)
                    d, _, _ = cbr.stream(B0, C).encode_packed_rows_chunk(p[:, a * N0:b * N0])
                    assert not torch.equal(d.view(B0, b - a, C, -1)[:, 0], ref_rows[:, a]), (budget, chunks, a)
            st = cbr.stream(B0, C)
            assert st.packed_chunk_launches(pcm16=True) == (1 if one else cbr.encode_launches(C) + 2), (C, spreading, budget)
            rows, fits = _encode_chunks(st, p, chunks)
            assert torch.equal(fits, ref_fits), (budget, chunks, _where(fits, ref_fits))
            assert torch.equal(rows, ref_rows), (budget, chunks, _where(rows, ref_rows))


@gpu
@pytest.mark.parametrize("C", [1, 2])
def test_state_is_shared(C):
    """One stream alternates int16 chunks, float32 chunks of p / 32768, encode_chunk and reset(): the state an int16 chunk
    leaves is the float one's."""
    cbr = _codec(None, (1365, 0))
    p = _p16(C)
    x = _f32(p)
    ref_rows, ref_fits, _, _ = _ref_rows(C, None, (1365, 0))
    X, t, thr = cbr.encode(x)
    st = cbr.stream(B0, C)
    assert st.packed_chunk_launches(pcm16=True) == 1 and st.packed_chunk_launches() == 1

    def spectra(a, b):
        got = st.encode_chunk(x[:, a * N0:b * N0])
        for g, r in zip(got, (X, t, thr)):
            assert _same(g, r[:, a:b].contiguous()), (a, b, _where(g, r[:, a:b].contiguous()))

    def rows(src, a, b):
        d, _, f = st.encode_packed_rows_chunk(src[:, a * N0:b * N0])
        assert torch.equal(f, ref_fits[:, a:b]) and torch.equal(d.view(B0, b - a, C, -1), ref_rows[:, a:b]), (src.dtype, a, b)

    rows(p, 0, 2)
    rows(x, 2, 3)              # a float chunk on the state an int16 chunk left (block 1: all zero in clip 1)
    rows(p, 3, 5)              # ... and the other way round (block 2 holds the rails of clip 0)
    spectra(5, 6)
    rows(p, 6, 7)
    st.reset()                 # the zero state again
    rows(p, 0, 3)
    spectra(3, 4)
    rows(x, 4, 6)


# ---- 4. the C ABI -----------------------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _emit(codec, p, flags, want=("X", "t", "thr"), out0=None, out1=None):
    """ac_encode_fused_ex(flags) on int16 p with X / t / thr given where ``want`` names them: (status, X, t, thr)"""
    B, S, C = p.shape
    N = codec.filters_n
    K = S // N
    dev = p.device
    out = {"X": torch.full((B, K + 1, N, C), 7.0, device=dev) if "X" in want else None,
           "t": torch.full((B, K + 1, 1, C), 7.0, device=dev) if "t" in want else None,
           "thr": torch.full((B, K + 1, N, C), 7.0, device=dev) if "thr" in want else None}
    st = _lib.load().ac_encode_fused_ex(codec.mdct._plan(dev), codec.psy._plan(dev), _ptr(p), _ptr(out["X"]), _ptr(out["t"]),
                                        _ptr(out["thr"]), 0.0, flags, out0, out1, 0, B, K, C, None)
    torch.cuda.synchronize()
    return st, out["X"], out["t"], out["thr"]


@gpu
@pytest.mark.parametrize("C", [1, 2])
def test_c_abi_one_shot(C):
    lib = _lib.load()
    codec = _codec(None, None)
    p = _p16(C)
    F, M = K0 + 1, 64
    codes = torch.full((B0, F, N0, C), 77, dtype=torch.int16, device=p.device)
    sf = torch.full((B0, F, M, C), 77, dtype=torch.int8, device=p.device)
    # the flag alone, or with an element-wise epilogue
    for flags in (_lib.AC_IN_PCM16, _lib.AC_IN_PCM16 | _lib.AC_EMIT_NOISY, _lib.AC_IN_PCM16 | _lib.AC_EMIT_DB_NORM,
                  _lib.AC_IN_PCM16 | _lib.AC_EMIT_CODES | _lib.AC_EMIT_NOISY):
        assert _emit(codec, p, flags, out0=_ptr(codes), out1=_ptr(sf))[0] == _lib.AC_EINVAL, flags
        assert b"ac_encode_fused_pcm16" in lib.ac_last_error()
    assert int(codes.min()) == 77 == int(codes.max())
    # AC_EMIT_CODES | AC_IN_PCM16 with every subset of X / t / thr: each equals encode(p)'s
    X, t, thr = codec.encode(p)
    rc, rs = codec.encode_quantized(_f32(p))
    for k in range(4):
        for want in itertools.combinations(("X", "t", "thr"), k):
            codes.fill_(77)
            sf.fill_(77)
            st, gX, gt, gthr = _emit(codec, p, _lib.AC_EMIT_CODES | _lib.AC_IN_PCM16, want, _ptr(codes), _ptr(sf))
            assert st == _lib.AC_OK, (want, lib.ac_last_error())
            assert torch.equal(sf, rs) and torch.equal(codes, rc), want
            for name, got, ref in (("X", gX, X), ("t", gt, t), ("thr", gthr, thr)):
                assert (got is None) == (name not in want)
                assert got is None or _same(got, ref), (want, name, _where(got, ref))
    # AC_EMIT_PACKED | AC_IN_PCM16: the rows; at filters_n = 2048 unsupported, nothing written
    cbr = _codec(None, (1365, 0))
    ref_rows, ref_fits, ref_data, _ = _ref_rows(C, None, (1365, 0))
    data = torch.full_like(ref_data, 0xA5)
    fits = torch.full((B0 * F * C,), 7, dtype=torch.uint8, device=p.device)
    out = _lib.PackedOut(data.data_ptr(), cbr.row_bytes, fits.data_ptr())
    flags = _lib.AC_EMIT_PACKED | _lib.AC_IN_PCM16
    assert _emit(cbr, p, flags, (), ctypes.addressof(out))[0] == _lib.AC_OK, lib.ac_last_error()
    assert torch.equal(data, ref_data) and torch.equal(fits.view(B0, F, C), ref_fits.to(torch.uint8))
    assert _emit(cbr, p, flags, ("X",), ctypes.addressof(out))[0] == _lib.AC_EINVAL
    big = _codec(None, (1365, 0), 2048)
    data.fill_(0xA5)
    assert _emit(big, _p16(C, N=2048), flags, (), ctypes.addressof(out))[0] == _lib.AC_EUNSUPPORTED
    assert b"ac_encode_fused_pcm16" in lib.ac_last_error()
    assert int(data.min()) == 0xA5 == int(data.max())


def _c_chunk(st, psy, x, k, rb, dtype):
    data = torch.full((st.B * k * st.C * rb,), 0xA5, dtype=torch.uint8, device=st.device)
    fits = torch.full((st.B * k * st.C,), 7, dtype=torch.uint8, device=st.device)
    out = _lib.PackedOut(data.data_ptr(), rb, fits.data_ptr())
    status = _lib.load().ac_stream_encode_typed(st._handle, psy, _ptr(x), ctypes.addressof(out), None, None, 0.0, dtype, k, None)
    torch.cuda.synchronize()
    return status, data, fits


@gpu
@pytest.mark.parametrize("C", [1, 2])
def test_c_abi_stream(C):
    lib = _lib.load()
    P16 = _lib.AC_PACKED | _lib.AC_IN_PCM16
    p = _p16(C)
    x = _f32(p)
    # served: the rows, and the state the float chunk continues from
    cbr = _codec(None, (1365, 0))
    ref_rows, ref_fits, _, _ = _ref_rows(C, None, (1365, 0))
    psy, rb = cbr.psy._plan(p.device), cbr.row_bytes
    st = cbr.stream(B0, C)
    assert lib.ac_stream_packed_launches_pcm16(st._handle, psy) == 1
    status, d, f = _c_chunk(st, psy, p[:, :2 * N0].contiguous(), 2, rb, P16)
    assert status == _lib.AC_OK, lib.ac_last_error()
    assert torch.equal(d.view(B0, 2, C, rb), ref_rows[:, :2]) and torch.equal(f.view(B0, 2, C), ref_fits[:, :2].to(torch.uint8))
    assert _c_chunk(st, psy, p[:, :2 * N0].contiguous(), 2, rb + 4, P16)[0] == _lib.AC_EINVAL
    assert _c_chunk(st, psy, None, 0, rb, P16)[0] == _lib.AC_OK                  # k == 0
    status, d, _ = _c_chunk(st, psy, x[:, 2 * N0:5 * N0].contiguous(), 3, rb, _lib.AC_PACKED)
    assert status == _lib.AC_OK and torch.equal(d.view(B0, 3, C, rb), ref_rows[:, 2:5])
    assert lib.ac_stream_packed_launches_pcm16(st._handle, _codec(None, None).psy._plan(p.device)) == 0    # no budget
    # not served (the f32 spreading product: gated out): AC_EUNSUPPORTED, nothing written, the state untouched
    slow = _codec("f32", (1365, 0))
    assert _instance(slow, C) not in _built("qps16")
    ref_rows, _, _, _ = _ref_rows(C, "f32", (1365, 0))
    psy = slow.psy._plan(p.device)
    st = slow.stream(B0, C)
    assert lib.ac_stream_packed_launches_pcm16(st._handle, psy) == slow.encode_launches(C) + 2
    first, _, _ = st.encode_packed_rows_chunk(x[:, :2 * N0])
    status, d, f = _c_chunk(st, psy, p[:, 2 * N0:4 * N0].contiguous(), 2, rb, P16)
    assert status == _lib.AC_EUNSUPPORTED and b"composition" in lib.ac_last_error()
    assert int(d.min()) == 0xA5 == int(d.max()) and int(f.min()) == 7 == int(f.max())
    d, _, _ = st.encode_packed_rows_chunk(x[:, 2 * N0:4 * N0])
    assert torch.equal(first.view(B0, 2, C, rb), ref_rows[:, :2]) and torch.equal(d.view(B0, 2, C, rb), ref_rows[:, 2:4])


# ---- 5. the switches --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [1, 2])
def test_switches(C):
    p = _p16(C)
    for budget in (None, (1365, 0)):
        codec = _codec(None, budget)
        rc, rs = codec.encode_quantized(_f32(p))
        with _env(Q_NOFUSE):
            assert codec.encode_quantized_launches(C, pcm16=True) == 2
            codes, sf = codec.encode_quantized(p)
        assert codec.encode_quantized_launches(C, pcm16=True) == 1
        assert torch.equal(codes, rc) and torch.equal(sf, rs), budget
    cbr = _codec(None, (1365, 0))
    ref_rows, ref_fits, ref_data, _ = _ref_rows(C, None, (1365, 0))
    for name in (P_NOFUSE, Q_NOFUSE):                            # (the packing launch rides on the quantising one's switch too)
        with _env(name):
            assert cbr.encode_packed_rows_launches(C, pcm16=True) == cbr.encode_launches(C) + 2 == 3
            data, _, fits = cbr.encode_packed_rows(p)
            st = cbr.stream(B0, C)
            assert st.packed_chunk_launches(pcm16=True) == 3
            rows, cfits = _encode_chunks(st, p, (2, 3, 2))
        assert torch.equal(data, ref_data) and torch.equal(fits, ref_fits), name
        assert torch.equal(rows, ref_rows) and torch.equal(cfits, ref_fits), name
    assert cbr.encode_packed_rows_launches(C, pcm16=True) == 1 and cbr.stream(B0, C).packed_chunk_launches(pcm16=True) == 1


# ---- 6. elsewhere -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N,M,C,R", ELSEWHERE)
def test_elsewhere(N, M, C, R):
    cbr = _codec(None, (R, 0), N, M)
    p = _p16(C, N=N)
    x = _f32(p)
    assert cbr.encode_packed_rows_launches(C, pcm16=True) == cbr.encode_launches(C) + 2 > 1
    st = cbr.stream(B0, C)
    assert st.packed_chunk_launches(pcm16=True) == cbr.encode_launches(C) + 2
    if (N, M, C) != (1024, 64, 2):                               # (a budget beyond the cap leaves the quantising launch alone)
        assert cbr.encode_quantized_launches(C, pcm16=True) == 2
    rc, rs = cbr.encode_quantized(x)
    codes, sf = cbr.encode_quantized(p)
    assert torch.equal(sf, rs), _where(sf, rs)
    assert torch.equal(codes, rc), _where(codes, rc)
    ref_data, ref_index, ref_fits = cbr.encode_packed_rows(x)
    data, index, fits = cbr.encode_packed_rows(p)
    assert torch.equal(index, ref_index) and torch.equal(fits, ref_fits), _where(fits, ref_fits)
    assert torch.equal(data, ref_data), _where(data, ref_data)
    rows, cfits = [], []
    for part in [p[:, a * N:b * N] for a, b in _bounds((2, 3, 2))] + [torch.zeros_like(p[:, :N])]:
        d, _, f = st.encode_packed_rows_chunk(part)
        rows.append(d.view(B0, part.shape[1] // N, C, cbr.row_bytes))
        cfits.append(f)
    rows = torch.cat(rows, dim=1)
    assert torch.equal(torch.cat(cfits, dim=1), ref_fits)
    assert torch.equal(rows, ref_data.view(rows.shape)), _where(rows, ref_data.view(rows.shape))


# ---- 7. the gate ------------------------------------------------------------------------------------------------------
@gpu
def test_gate():
    """The queries say what the library holds, for every (C, spreading); the default spreading runs all four families in one
    launch, mono and stereo."""
    for fam in FAMILIES:
        assert _built(fam), "no k_fwd_fast_%s instance in the library" % fam
    for C, spreading in itertools.product((1, 2), (None, "f32")):
        plain, cbr = _codec(spreading, None), _codec(spreading, (1365, 0))
        inst = _instance(cbr, C)
        assert plain.encode_quantized_launches(C, pcm16=True) == (1 if inst in _built("q16") else 2), (C, spreading)
        assert cbr.encode_quantized_launches(C, pcm16=True) == (1 if inst in _built("qb16") else 2), (C, spreading)
        assert cbr.encode_packed_rows_launches(C, pcm16=True) == (1 if inst in _built("qp16") else 3), (C, spreading)
        assert cbr.stream(B0, C).packed_chunk_launches(pcm16=True) == (1 if inst in _built("qps16") else 3), (C, spreading)
        assert plain.encode_packed_rows_launches(C, pcm16=True) == 0 == plain.stream(B0, C).packed_chunk_launches(pcm16=True)
        if spreading is None:
            assert all(inst in _built(fam) for fam in FAMILIES), (C, inst)
    assert _codec("bf16_mfma", None).encode_quantized_launches(2, pcm16=True) == 2      # no fused instance of this product


# ---- 8. chip-filling launches -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("C", [2, 1])
def test_chip_filling(C, family):
    """>= 2048 workgroups of 4 waves x 4 frames (test_encode_quantized_fused's shapes), against the composition in the same
    process."""
    codec = _codec(None, None if family == "q16" else (1365, 0))
    K = csi.blocks_per_clip(N0)
    B = csi.clips_for(N0, C, tasks_per_workgroup=16, rows_per_clip=K if family == "qps16" else None)
    pairs = B if C == 2 else (B + 1) // 2
    assert pairs * (K if family == "qps16" else K + 1) >= 16 * csi.MIN_WORKGROUPS
    p = torch.round(csi.structured(B, K, N0, C, seed=600 + C) * 32767).to(torch.int16)
    assert _instance(codec, C) in _built(family)
    if family in ("q16", "qb16"):
        call, switch = (lambda: codec.encode_quantized(p)), Q_NOFUSE
        assert codec.encode_quantized_launches(C, pcm16=True) == 1
    elif family == "qp16":
        call, switch = (lambda: codec.encode_packed_rows(p)), P_NOFUSE
        assert codec.encode_packed_rows_launches(C, pcm16=True) == 1
    else:
        call, switch = (lambda: codec.stream(B, C).encode_packed_rows_chunk(p)), P_NOFUSE
        assert codec.stream(B, C).packed_chunk_launches(pcm16=True) == 1
    got = call()
    with _env(switch):
        ref = call()
    for g, r in zip(got, ref):
        assert torch.equal(g, r), (family, _where(g, r))
    assert int(got[0].max()) > 0


# ---- 9. the stream contract ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    from stream_order import Harness
    return Harness()


@gpu
@pytest.mark.parametrize("what", ["encode_quantized", "encode_packed_rows", "chunk"])
@pytest.mark.parametrize("check", ["delayed_producer", "busy_default"])
def test_stream_contract(harness, check, what):
    """The int16 calls only enqueue on the current stream, as their float32 forms do (their own test files)."""
    cbr = _codec(None, (1365, 0))
    p = torch.round(_pcm(N0, 2, 4, 20, seed=79, inject=False) * 32767).to(torch.int16)
    if what == "chunk":
        st = cbr.stream(4, 2)
        assert st.packed_chunk_launches(pcm16=True) == 1

        def fn(p):
            st.reset()                                           # (on the stream the case runs on)
            return st.encode_packed_rows_chunk(p)
    elif what == "encode_packed_rows":
        assert cbr.encode_packed_rows_launches(2, pcm16=True) == 1
        fn = cbr.encode_packed_rows
    else:
        assert cbr.encode_quantized_launches(2, pcm16=True) == 1
        fn = cbr.encode_quantized
    getattr(harness, check)("%s[int16-1024-2]" % what, ([p], fn))
