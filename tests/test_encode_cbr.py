"""A codec at a bitrate: plans that carry a row budget (``ac_psy_plan_with_row_budget``),
``PsychoacousticModel.with_row_budget`` and ``AudioCodec.with_row_budget`` / ``with_bitrate`` on top of them, and the fused
encode at filters_n = 1024 that meets the budget in its one launch (k_fwd_fast_qb).

The reference of every GPU comparison is the two launches of the base codec -- ``base.encode_quantized_budget(x, R, kmin)``:
``encode()`` into float32 tensors, then ``k_quantize_budget`` -- and every comparison is bit for bit (``torch.equal``; float
tensors that may hold NaN as their int32 patterns).  One case also holds the numpy restatement of ``rate_reference.py``
against them.

The input is ``_pcm(..., inject=True)`` -- a zero frame, a NaN and an Inf -- with ``x[1, 4N + 9, 0] = 1e15``, and one sample
more.  On the CPU oracle the 1e15 sample makes a row that no offset brings under a small budget (scale factors stop at
127).  The float32 masking model of the GPU kernels overflows on that frame (|X| = 7e11: tonality -inf, thresholds not
finite), so there the row stores nothing -- one more row with NaN bands, at its 320 bits.  The row at 254 comes from
``x[0, 4N + 9, 0] = 3e12`` (1e13 at filters_n = 2048), measured on the reference: the model stays finite up to 3e12 and has
overflowed at 1e13 (filters_n 960, 1024; 2048: finite at 1e13, overflowed at 3e13), and at 1e12 the row still fits.  Every
test that uses the input asserts on the reference what a binding budget must show (``_binding``).
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
from rate_reference import quantize_budget
from test_encode_quantized_fused import _emit_codes, _pcm, _same, _where

gpu = pytest.mark.gpu
N0 = 1024
UNLIMITED = 16 * N0 + 13 * 64                                        # 17216: no row is longer
BUDGETS = [(1365, 0), (2730, -8), (320, 0), (UNLIMITED, 0), (UNLIMITED, 4)]   # (row_bits, min_offset)


# ---- CPU: the interface (needs the built library) ----------------------------------------------------------------
def test_header_declares_the_plan_functions_without_a_stream():
    text = open(os.path.join(ROOT, "include", "audiocodec_amd.h")).read()
    for name in ("ac_psy_plan_with_row_budget", "ac_psy_plan_row_budget"):
        m = re.search(r"AC_API\s+int\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        assert "stream" not in m.group(1), (name, m.group(1))
    assert re.search(r"ac_psy_plan_with_row_budget\s*\(\s*const ac_psy_plan\s*\*\s*plan,\s*int row_bits,\s*int kmin,\s*"
                     r"ac_psy_plan\s*\*\*\s*out\)", text)


def test_library_exports_the_plan_functions():
    lib = _lib.load()
    for name in ("ac_psy_plan_with_row_budget", "ac_psy_plan_row_budget"):
        assert name in _lib.PROTOTYPES
        assert callable(getattr(lib, name))
    assert lib.ac_version() == 171
    out = ctypes.c_void_p()
    assert lib.ac_psy_plan_with_row_budget(None, 1365, 0, ctypes.byref(out)) == _lib.AC_EINVAL
    assert "plan" in lib.ac_last_error().decode() and not out.value
    r, k = ctypes.c_int(7), ctypes.c_int(7)
    assert lib.ac_psy_plan_row_budget(None, ctypes.byref(r), ctypes.byref(k)) == _lib.AC_EINVAL


def test_python_interface_validates_its_arguments():
    base = audiocodec_amd.AudioCodec(48000, N0)
    assert base.row_bits is None and base.psy.row_budget is None
    cbr = base.with_bitrate(64000.5)
    assert cbr.row_bits == 1365 == base.row_bits_for_bitrate(64000.5)
    assert cbr.psy.row_budget == (1365, 0) and cbr.mdct is base.mdct and cbr.psy is not base.psy
    assert base.row_bits is None and base.psy.row_budget is None             # the base codec is left as it was
    cbr2 = cbr.with_row_budget(2730, min_offset=-8)                          # deriving again replaces the budget
    assert cbr2.row_bits == 2730 and cbr2.psy.row_budget == (2730, -8) and cbr2.mdct is base.mdct
    m = base.psy.with_row_budget(np.int32(320), np.int64(254))
    assert m.row_budget == (320, 254) and m.W is base.psy.W and m.filter_bands_n == N0
    for obj in (base, base.psy):
        for bad in (319, 0, -1, 2 ** 31):
            with pytest.raises(ValueError):
                obj.with_row_budget(bad)
        for bad in (1365.0, True, "1365", None, torch.tensor(1365)):
            with pytest.raises(TypeError):
                obj.with_row_budget(bad)
        for bad in (255, -255):
            with pytest.raises(ValueError):
                obj.with_row_budget(1365, bad)
        for bad in (1.5, False, None):
            with pytest.raises(TypeError):
                obj.with_row_budget(1365, bad)
    with pytest.raises(ValueError):
        base.with_bitrate(0)
    with pytest.raises(TypeError):
        base.with_bitrate("128k")
    with pytest.raises(ValueError):
        base.with_bitrate(10000)                                             # 213 bits: below 5 * 64
    with pytest.raises(NotImplementedError):                                 # float32 only, as quantize_to_budget
        audiocodec_amd.AudioCodec(48000, N0, compute_dtype=torch.float64).with_row_budget(1365)


# ---- GPU ---------------------------------------------------------------------------------------------------------
def _input(C, B, K, seed, inject, N=N0):
    """``_pcm`` and, with ``inject``, the two large samples of the module docstring: 1e15 in clip 1, and in clip 0 the one whose
    frame stays finite on the GPU and cannot meet a small budget at any offset."""
    x = _pcm(N, C, B, K, seed=seed, inject=inject)
    if inject:
        x[1, 4 * N + 9, 0] = 1e15
        x[0, 4 * N + 9, 0] = 1e13 if N == 2048 else 3e12
    return x


def _binding(R, kmin, offset, row_bits):
    """What a reference must show at a binding budget, so that a degenerate input cannot pass."""
    assert int((offset == kmin).sum()) >= 1, "no row at min_offset"
    assert int(((offset > kmin) & (offset < 254)).sum()) >= 1, "no row strictly between min_offset and 254"
    assert int(((offset == 254) & (row_bits > R)).sum()) >= 1, "no row at 254 with its budget unmet"


SMALL = [  # C, spreading, B, K, drown, inject
    (1, None, 3, 5, 0.0, True), (2, None, 3, 5, 0.0, True), (1, "f32", 3, 5, 0.0, True), (2, "f32", 3, 5, 0.0, True),
    (2, None, 3, 5, 0.5, True), (1, None, 3, 5, 0.5, True), (2, "f32", 3, 5, 0.5, True), (1, "f32", 3, 5, 0.5, True),
    (2, None, 1, 1, 0.0, False), (1, None, 1, 1, 0.0, False), (2, "f32", 1, 1, 0.0, False), (1, "f32", 1, 1, 0.0, False),
    (2, None, 2, 0, 0.0, False), (1, "f32", 3, 0, 0.0, False)]


@gpu
@pytest.mark.parametrize("C,spreading,B,K,drown,inject", SMALL)
def test_small_shapes_bit_exact(C, spreading, B, K, drown, inject):
    """Every budget on both edge frames of every clip, a half-empty mono pair (B odd), an all-zero frame, NaN, Inf and a row
    that no offset brings under its budget."""
    base = audiocodec_amd.AudioCodec(48000, N0, spreading=spreading)
    x = _input(C, B, K, C + 2 * B + K, inject)
    plain = base.encode_quantized(x, drown)
    for R, kmin in BUDGETS:
        cbr = base.with_row_budget(R, kmin)
        assert cbr.encode_quantized_launches(C) == 1 and cbr.row_bits == R
        rc, rs, ro, rb = base.encode_quantized_budget(x, R, kmin, drown)
        if inject and R in (1365, 320):
            _binding(R, kmin, ro, rb)
        codes, sf = cbr.encode_quantized(x, drown)
        assert codes.dtype == torch.int16 and codes.shape == (B, K + 1, N0, C)
        assert sf.dtype == torch.int8 and sf.shape == (B, K + 1, 64, C)
        assert torch.equal(sf, rs), (R, kmin, _where(sf, rs))
        assert torch.equal(codes, rc), (R, kmin, _where(codes, rc))
        if (R, kmin) == (UNLIMITED, 0):                      # ... which is the base codec's unbudgeted encode
            assert torch.equal(codes, plain[0]) and torch.equal(sf, plain[1])
        if inject:
            assert bool((sf == -128).any()) and int(codes[1, 2].abs().max()) == 0 and int(codes.abs().max()) > 0


@gpu
def test_numpy_restatement():
    base = audiocodec_amd.AudioCodec(48000, N0)
    x = _input(2, 3, 5, 13, True)
    X, _, thr = base.encode(x)
    nc, ns, no, nb = quantize_budget(X.cpu().numpy(), thr.cpu().numpy(), base.psy.scale_band_offsets, 1365, 0)
    _binding(1365, 0, no, nb)
    codes, sf = base.with_row_budget(1365).encode_quantized(x)
    np.testing.assert_array_equal(sf.cpu().numpy(), ns)
    np.testing.assert_array_equal(codes.cpu().numpy(), nc)


@gpu
@pytest.mark.parametrize("C", [1, 2])
def test_optional_outputs(C):
    """X, t and thr under AC_EMIT_CODES with a derived plan: each equals encode()'s where given, any subset may be NULL."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    cbr = base.with_row_budget(1365)
    x = _input(C, 3, 5, 40 + C, True)
    X, t, thr = base.encode(x)
    rc, rs, ro, rb = base.encode_quantized_budget(x, 1365)
    _binding(1365, 0, ro, rb)
    for k in range(4):
        for want in itertools.combinations(("X", "t", "thr"), k):
            st, gX, gt, gthr, codes, sf = _emit_codes(cbr, x, want)
            assert st == _lib.AC_OK, (want, _lib.load().ac_last_error())
            assert torch.equal(sf, rs) and torch.equal(codes, rc), want
            for name, got, ref in (("X", gX, X), ("t", gt, t), ("thr", gthr, thr)):
                assert (got is None) == (name not in want)
                assert got is None or _same(got, ref), (want, name, _where(got, ref))


@gpu
def test_plan_carries_the_budget():
    lib = _lib.load()
    base = audiocodec_amd.AudioCodec(48000, N0, spreading="f32")
    dev = torch.device("cuda", torch.cuda.current_device())
    r, k = ctypes.c_int(7), ctypes.c_int(7)
    assert lib.ac_psy_plan_row_budget(base.psy._plan(dev), ctypes.byref(r), ctypes.byref(k)) == _lib.AC_OK
    assert (r.value, k.value) == (0, 0)
    cbr = base.with_row_budget(1365, 3).with_row_budget(2730, -8)
    plan = cbr.psy._plan(dev)
    assert plan.value != base.psy._plan(dev).value
    assert lib.ac_psy_plan_row_budget(plan, ctypes.byref(r), ctypes.byref(k)) == _lib.AC_OK
    assert (r.value, k.value) == (2730, -8)
    assert cbr.psy.plan_spreading() == "f32" and cbr.psy.is_fast() and cbr.psy.tier() == base.psy.tier()
    out = ctypes.c_void_p()
    for R, kmin in ((319, 0), (1365, 255), (1365, -255)):
        assert lib.ac_psy_plan_with_row_budget(plan, R, kmin, ctypes.byref(out)) == _lib.AC_EINVAL and not out.value
    # every entry point that does not quantise from sf0 treats the derived plan as the base plan
    x = _input(2, 3, 5, 3, True)
    for a, b in zip(cbr.encode(x), base.encode(x)):
        assert _same(a, b)


@gpu
@pytest.mark.parametrize("N,C", [(1024, 2), (960, 3)])
def test_quantize_on_a_derived_plan(N, C):
    base = audiocodec_amd.AudioCodec(48000, N)
    x = _input(C, 3, 5, N + C, True, N)
    X, _, thr = base.encode(x)
    for R, kmin in ((1365, 0), (2730, -8)):
        rc, rs, ro, rb = base.psy.quantize_to_budget(X, thr, R, kmin)
        if R == 1365:
            _binding(R, kmin, ro, rb)
        codes, sf = base.psy.with_row_budget(R, kmin).quantize(X, thr)
        assert torch.equal(codes, rc) and torch.equal(sf, rs), (R, kmin)
    pc, ps = base.psy.quantize(X, thr)                       # the base model is not budgeted by its derivations
    uc, us, _, _ = base.psy.quantize_to_budget(X, thr, 16 * N + 13 * 64, 0)
    assert torch.equal(pc, uc) and torch.equal(ps, us)


FALLBACK = [(960, 2, None), (1024, 3, None), (2048, 2, None), (1024, 2, "bf16_mfma")]


@gpu
@pytest.mark.parametrize("N,C,spreading", FALLBACK)
def test_fallback_is_the_composition(N, C, spreading):
    base = audiocodec_amd.AudioCodec(48000, N, spreading=spreading)
    cbr = base.with_row_budget(1365)
    assert cbr.encode_quantized_launches(C) == 2
    x = _input(C, 3, 5, N + C, True, N)
    X, t, thr = base.encode(x)
    rc, rs, ro, rb = base.encode_quantized_budget(x, 1365)
    _binding(1365, 0, ro, rb)
    codes, sf = cbr.encode_quantized(x)
    assert torch.equal(codes, rc) and torch.equal(sf, rs)
    st, gX, gt, gthr, codes, sf = _emit_codes(cbr, x, ("X", "t", "thr"))
    assert st == _lib.AC_OK, _lib.load().ac_last_error()
    assert torch.equal(codes, rc) and torch.equal(sf, rs) and _same(gX, X) and _same(gt, t) and _same(gthr, thr)
    for want in (("t", "thr"), ("X", "thr"), ("X", "t"), ()):
        assert _emit_codes(cbr, x, want)[0] == _lib.AC_EINVAL, want
        assert b"intermediates" in _lib.load().ac_last_error()


@gpu
def test_pcm16_input_takes_two_launches():
    base = audiocodec_amd.AudioCodec(48000, N0)
    x = _pcm(N0, 2, 3, 5, seed=9, inject=False)
    pcm = torch.round(x * 32767).to(torch.int16)
    rc, rs, ro, _ = base.encode_quantized_budget(pcm, 1365)
    assert int((ro > 0).sum()) >= 1
    codes, sf = base.with_row_budget(1365).encode_quantized(pcm)
    assert torch.equal(codes, rc) and torch.equal(sf, rs)


@gpu
def test_nofuse_hook(monkeypatch):
    base = audiocodec_amd.AudioCodec(48000, N0)
    cbr = base.with_row_budget(1365)
    x = _input(2, 3, 5, 21, True)
    fused = cbr.encode_quantized(x)
    assert cbr.encode_quantized_launches(2) == 1
    monkeypatch.setenv("AC_ENCODE_QUANT_NOFUSE", "1")
    assert cbr.encode_quantized_launches(2) == 2 and cbr.encode_quantized_launches(1) == 2
    two = cbr.encode_quantized(x)
    assert torch.equal(two[0], fused[0]) and torch.equal(two[1], fused[1])
    assert _emit_codes(cbr, x, ("t", "thr"))[0] == _lib.AC_EINVAL
    monkeypatch.delenv("AC_ENCODE_QUANT_NOFUSE")
    assert cbr.encode_quantized_launches(2) == 1
    rc, rs, ro, rb = base.encode_quantized_budget(x, 1365)
    _binding(1365, 0, ro, rb)
    assert torch.equal(fused[0], rc) and torch.equal(fused[1], rs)


@gpu
@pytest.mark.parametrize("C", [2, 1])
def test_packed(C):
    """A row that met its budget R takes at most ceil(R / 32) * 4 bytes of data; the stream decodes as the reference codes do."""
    R = 1365
    base = audiocodec_amd.AudioCodec(48000, N0)
    cbr = base.with_bitrate(64000)
    assert cbr.row_bits == R
    x = _input(C, 3, 5, 50 + C, True)
    rc, rs, ro, rb = base.encode_quantized_budget(x, R)
    _binding(R, 0, ro, rb)
    data, index = cbr.encode_packed(x)
    ends = torch.cat([index.flatten()[1:], torch.tensor([data.numel()], device=index.device)]).view_as(index)
    size = ends - index
    met = ro < 254
    assert int(met.sum()) >= 2 and int(size[met].max()) <= (R + 31) // 32 * 4
    got, ref = cbr.decode_packed(data, index), base.decode_quantized(rc, rs)
    assert _same(got, ref), _where(got, ref)


@gpu
def test_explicit_budget_methods_obey_their_arguments():
    base = audiocodec_amd.AudioCodec(48000, N0)
    cbr = base.with_row_budget(1365)
    x = _input(2, 3, 5, 61, True)
    for got, ref in zip(cbr.encode_quantized_budget(x, 2730, -8), base.encode_quantized_budget(x, 2730, -8)):
        assert torch.equal(got, ref)
    T = base.clip_bits_for_bitrate(96000, 6, 2)
    for got, ref in zip(cbr.encode_quantized_clip_budget(x, T), base.encode_quantized_clip_budget(x, T)):
        assert torch.equal(got, ref)


@gpu
@pytest.mark.parametrize("C", [2, 1])
def test_chip_filling(C, monkeypatch):
    """>= 2048 workgroups of 4 waves x 4 frames, against the two launches in the same process."""
    cbr = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    K = csi.blocks_per_clip(N0)
    B = csi.clips_for(N0, C, tasks_per_workgroup=16)
    pairs = B if C == 2 else (B + 1) // 2
    assert pairs * (K + 1) >= 16 * csi.MIN_WORKGROUPS
    x = csi.structured(B, K, N0, C, seed=400 + C)
    assert cbr.encode_quantized_launches(C) == 1
    codes, sf = cbr.encode_quantized(x)
    monkeypatch.setenv("AC_ENCODE_QUANT_NOFUSE", "1")
    assert cbr.encode_quantized_launches(C) == 2
    rc, rs = cbr.encode_quantized(x)
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
    """The contract ac_encode_fused_ex's row of test_stream_contract.py holds its flags to, on a plan with a row budget."""
    cbr = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    assert cbr.encode_quantized_launches(2) == 1
    x = _pcm(N0, 2, 4, 20, seed=77, inject=False)
    case = ([x], lambda x: cbr.encode_quantized(x))
    getattr(harness, check)("cbr.encode_quantized[1024-2]", case)
