"""The quantiser, the packer and rate control at the exact boundaries of their decisions (DESIGN.md sections 8a to 8e).

Every search of that family ends in a comparison -- ``bits <= budget`` (``row_offset``, ``transrate_row``, ``k_quantize_budget``,
``k_requantize_budget``), ``total <= T`` and the inclusive prefix sum of section 8d, ``bits <= 8 row_bytes`` (``fits``), ``fp32(step(s)
sqrt 3) <= min(thr)`` (``scale_factor_of``) -- and every code in a rounding (``qcode``: half to even, the clamp at +-32767).  The
other files choose layouts, launch sizes and channel counts; the values they feed land on an edge only by accident.  Here
``boundary_inputs.py`` chooses the values: budgets equal to a row's (a clip's) length at the first offset of that length, and one
bit to either side; band minima that are a criterion value, its predecessor and its successor, for all 255 scale factors;
bins whose product with the inverse step is k + 0.5, and the float on either side of such a bin.

The CPU tests build every input and assert, on the numpy restatements alone, that it shows its boundary.  The GPU tests
compare the kernels with those restatements (and the one-launch forms with their compositions) by exact equality; no
comparison in this file has a tolerance.

1. budgets that bind with equality: ``test_fused_*`` (the one-launch encoders at filters_n = 1024 and the compositions at 2048
   and 960), ``test_generic_*`` (a budget tensor with every row on its own edge), ``test_transrate_*``;
2. a clip's budget: ``test_clip_budget_edges``;
3. the scale-factor criterion: ``test_criterion_edges``;
4. ties, clamps and every scale factor downstream: ``test_ties_*``.

The file was run against one-character mutants of the library, each of which fails here: ``<`` for ``<=`` in ``row_offset``
(the ``test_fused_*`` cases at 1024), in ``transrate_row``'s search (``test_transrate_*``) and its ``fits``
(``test_transrate_slot_slack`` alone), in ``k_quantize_budget`` / ``k_requantize_budget`` (``test_generic_*``, every composition
of ``test_fused_*``, ``test_transrate_*``), in the clip search and in the fill's prefix sum (``test_clip_budget_edges``), in
``scale_factor_of`` (``test_criterion_edges``, ``test_ties_*``), and ``roundf`` for ``rint`` in ``qcode`` (``test_ties_*``).  Of the
older files, those of the fused encoders and ``test_clip_rate.py`` notice the strict comparison in ``row_offset`` and in the clip
search, through budgets equal to the floor of 5 M bits per row (320) and the floor of a clip, where every row ends on its
budget; ``test_quantizer.py``, ``test_rate_control.py`` and ``test_encode_quantized_fused.py`` pass with the strict comparison in
``scale_factor_of``.
"""

import functools

import numpy as np
import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib

import boundary_inputs as bi
from clip_rate_reference import ClipStats
from pack_reference import np_canon, np_pack, np_unpack
from pack_rows_reference import np_rows_from_codes
from rate_reference import K_MAX, fast_search, quantize_budget
from test_clip_rate import clip_unlimited, clips
from test_encode_cbr import _input
from test_encode_pcm16 import P_NOFUSE, Q_NOFUSE, _built as _built16, _instance
from test_encode_quantized_fused import _same, _where
from test_quantizer import np_dequantize, np_offsets, np_quantize
from test_rate_control import adversarial, unlimited
from test_stream_packed import _encode_chunks, _env, _gate_passed
from test_transrate import _random_rows, _three_ways
from transrate_reference import np_transrate, requant_fast, requantize_budget

gpu = pytest.mark.gpu
CAP = _lib.AC_PACK_ROWS_MAX_BITS
B1, K1 = 3, 5                                                # 36 rows at C = 2; three mono clips: a half-empty pair

GENERIC = [(48000, 1024, 64, 2), (48000, 960, 64, 3), (48000, 2048, 64, 1), (48000, 64, 64, 2)]
REQUANT = [(48000, 1024, 64, 2), (44100, 256, 48, 3)]
CLIP = [(48000, 1024, 64, 2), (48000, 960, 64, 6), (48000, 64, 64, 2)]
CRITERION = [(48000, 1024, 64, 2), (48000, 1024, 64, 1), (48000, 960, 64, 3), (48000, 2048, 64, 1), (44100, 256, 48, 2),
             (48000, 64, 64, 2)]
TIES = [(1024, 2), (960, 3)]
TIES_DECODE = [(1024, 1), (1024, 2), (2048, 1), (2048, 2)]


# ---- inputs and references: built once, never modified -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _generic_case(sr, N, M, C):
    """``test_rate_control.adversarial`` rows with one budget per row, each on a plateau start of its row: (X, thr, off, R, k,
    reference at R, reference at R - 1)."""
    off = np_offsets(sr, N, M)
    rng = np.random.default_rng(5 * N + C)
    X, thr = adversarial(rng, off, 2, 3, C)
    table = fast_search(X, thr, off, unlimited(N, M), 0)
    fallback = np.maximum(5 * M, table[3] * rng.uniform(0.1, 1.0, table[3].shape)).astype(np.int32)
    R, k = bi.per_row_budgets(table[4], rng, fallback)
    at, under = bi.check_per_row(lambda R, k0: quantize_budget(X, thr, off, R, k0), R, k)
    return X, thr, off, R, k, at, under


@functools.lru_cache(maxsize=None)
def _requant_case(sr, N, M, C):
    off = np_offsets(sr, N, M)
    rng = np.random.default_rng(3 * N + C)
    codes, sf = _random_rows(rng, off, 2, 3, C)
    table = requant_fast(codes, sf, off, unlimited(N, M), 0)
    R, k = bi.per_row_budgets(table[4], rng, np.full(table[3].shape, 5 * M, np.int32))
    at, under = bi.check_per_row(lambda R, k0: requantize_budget(codes, sf, off, R, k0), R, k)
    return codes, sf, off, R, k, at, under


@functools.lru_cache(maxsize=None)
def _slot_case():
    """Rows of constant length around R' = 1375 (43 words less one bit), dense as ``np_pack`` writes them."""
    off = np_offsets(48000, 1024, 64)
    R = 1375
    codes, sf, lengths = bi.slot_rows(off, R)
    data, index = np_pack(codes, sf, off)
    return off, R, codes, sf, lengths, data, index


@functools.lru_cache(maxsize=None)
def _clip_case(sr, N, M, C):
    off = np_offsets(sr, N, M)
    X, thr = clips(np.random.default_rng(N + C), off, 4, 6, C)
    st = ClipStats(X, thr, off)
    T = bi.clip_edges(st)
    return X, thr, off, st, T, bi.check_clip_edges(st, T, off)


@functools.lru_cache(maxsize=None)
def _criterion_case(sr, N, M, C):
    off = np_offsets(sr, N, M)
    X, thr, planted = bi.criterion_input(off, C, np.random.default_rng(N + C))
    codes, sf = bi.check_criterion_input(X, thr, planted, off)
    return X, thr, off, codes, sf


@functools.lru_cache(maxsize=None)
def _tie_case(N, C):
    off = np_offsets(48000, N, 64)
    X, thr = bi.tie_input(off, C)
    codes, sf = bi.check_tie_input(X, thr, off)
    return X, thr, off, codes, sf


# ---- CPU: every input shows its boundary, on the references alone --------------------------------------------------------
def test_row_budget_plan_on_the_reference():
    """The plan the fused encoders get from their own spectra, here on synthetic rows: three targets, five budgets each, every
    precondition asserted by ``edge_budgets``; a budget one bit short gives another offset, so a strict comparison shows."""
    off = np_offsets(48000, 1024, 64)
    rng = np.random.default_rng(12)
    X = (rng.standard_normal((2, 4, 1024, 2)) * 10.0 ** rng.uniform(-3, 0, (2, 4, 1, 2))).astype(np.float32)
    thr = (np.abs(X) * 0.02 + np.abs(rng.standard_normal(X.shape)) * 1e-4 + 1e-7).astype(np.float32)
    bits = fast_search(X, thr, off, unlimited(1024, 64), 0)[4]
    targets = bi.pick_three(bi.plateau_starts(bits, 0, hi=CAP))
    assert 1 <= targets[0].k <= 3 and targets[0].k <= targets[1].k <= targets[2].k < K_MAX
    plan = bi.edge_budgets(lambda R, k0: quantize_budget(X, thr, off, R, k0), targets)
    assert len(plan) == 15
    for t in targets:
        assert 321 <= t.R and t.R + 1 <= CAP
        by = {(R, k0): ref for R, k0, tt, ref in plan if tt is t}
        assert int(by[t.R, 0][2][t.row]) == t.k < int(by[t.R - 1, 0][2][t.row])
        assert not np.array_equal(by[t.R, 0][1], by[t.R - 1, 0][1])


@pytest.mark.parametrize("sr,N,M,C", GENERIC)
def test_per_row_budgets_on_the_reference(sr, N, M, C):
    X, thr, off, R, k, at, under = _generic_case(sr, N, M, C)
    has = k >= 0
    assert 2 * has.sum() >= has.size
    assert np.array_equal(at[3][has], R[has]) and np.all(under[2][has] > at[2][has])
    print("%d of %d rows at equality" % (has.sum(), has.size))


@pytest.mark.parametrize("sr,N,M,C", REQUANT)
def test_per_row_requantiser_budgets_on_the_reference(sr, N, M, C):
    codes, sf, off, R, k, at, under = _requant_case(sr, N, M, C)
    has = k >= 0
    assert 2 * has.sum() >= has.size and np.all(under[2][has] > at[2][has])


def test_slot_rows_on_the_reference():
    """The rows of constant length: R' met with equality at offset 0; one bit more is not met (offset 254) and fills the slot
    to its last bit (fits); two bits more is the marked row."""
    off, R, codes, sf, lengths, data, index = _slot_case()
    table = requant_fast(codes, sf, off, R, 0)[4]
    assert (table == np.array(lengths).reshape(1, 1, 4, 1)).all()              # the same length at every offset
    out, _, fits, offset, bits = np_transrate(data, index, off, 1024, R)
    assert 8 * (len(out) // 4) == R + 1
    assert fits.ravel().tolist() == [True, True, False, True]
    assert offset.ravel().tolist() == [0, K_MAX, K_MAX, 0] and bits.ravel().tolist() == lengths


@pytest.mark.parametrize("sr,N,M,C", CLIP)
def test_clip_edges_on_the_reference(sr, N, M, C):
    X, thr, off, st, T, ref = _clip_case(sr, N, M, C)
    assert set(T) == {"plateau", "plateau-1", "fill", "fill-1", "last", "last-1"}
    assert st.B == 4 and st.F == 6
    for a, b in (("plateau", "plateau-1"), ("fill", "fill-1")):                          # one bit changes every clip's rows
        assert np.all((ref[a][2] != ref[b][2]).any(axis=(1, 2)) | (ref[a][5] != ref[b][5])), a
    assert np.all((ref["fill"][2] != ref["fill-1"][2]).sum(axis=(1, 2)) >= 1)
    assert np.all(ref["last-1"][5] == ref["last"][5])                                      # unmet: the same rows, at 254


@pytest.mark.parametrize("sr,N,M,C", CRITERION)
def test_criterion_edges_on_the_reference(sr, N, M, C):
    X, thr, off, codes, sf = _criterion_case(sr, N, M, C)
    assert len(bi.criterion_values()) == 765 + 9
    assert X.shape[0] * X.shape[1] * C * int((np.diff(off) > 0).sum()) >= 765 + 9


@pytest.mark.parametrize("N,C", TIES + TIES_DECODE)
def test_ties_on_the_reference(N, C):
    X, thr, off, codes, sf = _tie_case(N, C)
    assert len(bi.TIE_K) == 31 and np.abs(codes).max() == 32767


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _eq(got, ref, what):
    np.testing.assert_array_equal(got.cpu().numpy(), ref, err_msg=str(what))


def _x(C, N=1024, pcm16=False):
    x = _input(C, B1, K1, 700 + C, not pcm16, N)
    return torch.round(x * 32767).to(torch.int16) if pcm16 else x


FUSED = [(1024, 2, None, False), (1024, 2, "f32", False), (1024, 1, None, False), (1024, 2, None, True), (1024, 1, None, True),
         (1024, 2, "f32", True), (2048, 2, None, False), (960, 2, None, False)]


@functools.lru_cache(maxsize=None)
def _fused_case(N, C, spreading, pcm16):
    """(base codec, x, off, plan): X and thr of the base codec's unfused ``encode()``, the table bits_r(k) of the reference, three
    target rows and the five budgets of each with the reference's result (``edge_budgets`` asserts the preconditions)."""
    base = audiocodec_amd.AudioCodec(48000, N, spreading=spreading)
    x = _x(C, N, pcm16)
    X, _, thr = base.encode(x)
    X, thr = X.cpu().numpy(), thr.cpu().numpy()
    off = base.psy.scale_band_offsets
    bits = fast_search(X, thr, off, unlimited(N, 64), 0)[4]
    targets = bi.pick_three(bi.plateau_starts(bits, 0, hi=CAP))
    plan = bi.edge_budgets(lambda R, k0: quantize_budget(X, thr, off, R, k0), targets)
    print("targets:", targets)
    return base, x, off, plan


def _one(base, C, pcm16, family):
    """Whether the plan method runs in one launch: filters_n = 1024, and for int16 PCM an instance that passed the register gate."""
    if base.filters_n != 1024:
        return False
    return _instance(base, C) in _built16(family) if pcm16 else True


@gpu
@pytest.mark.parametrize("N,C,spreading,pcm16", FUSED)
def test_fused_codes_at_equality(N, C, spreading, pcm16):
    """``with_row_budget(R, kmin).encode_quantized`` (k_fwd_fast_qb / qb16; two launches at 2048 and 960) against the numpy
    restatement and, where it is one launch, against its composition."""
    base, x, off, plan = _fused_case(N, C, spreading, pcm16)
    for R, kmin, t, ref in plan:
        cbr = base.with_row_budget(R, kmin)
        one = _one(base, C, pcm16, "qb16")
        assert cbr.encode_quantized_launches(C, pcm16=pcm16) == (1 if one else 2), (R, kmin)
        codes, sf = cbr.encode_quantized(x)
        _eq(sf, ref[1], (R, kmin, t))
        _eq(codes, ref[0], (R, kmin, t))
        if one:
            with _env(Q_NOFUSE):
                assert cbr.encode_quantized_launches(C, pcm16=pcm16) == 2
                two = cbr.encode_quantized(x)
            assert torch.equal(two[1], sf) and torch.equal(two[0], codes), (R, kmin, _where(two[0], codes))


@gpu
@pytest.mark.parametrize("N,C,spreading,pcm16", FUSED)
def test_fused_rows_at_equality(N, C, spreading, pcm16):
    """``.encode_packed_rows`` (k_fwd_fast_qp / qp16; the composition at 2048 and 960) against ``pack_rows_reference``."""
    base, x, off, plan = _fused_case(N, C, spreading, pcm16)
    for R, kmin, t, ref in plan:
        cbr = base.with_row_budget(R, kmin)
        data, index, fits = np_rows_from_codes(ref[0], ref[1], ref[3], off, R)
        assert fits[t.row]
        one = _one(base, C, pcm16, "qp16")
        assert cbr.encode_packed_rows_launches(C, pcm16=pcm16) == (1 if one else cbr.encode_launches(C) + 2), (R, kmin)
        got = cbr.encode_packed_rows(x)
        _eq(got[2], fits, (R, kmin, t))
        _eq(got[1], index, (R, kmin, t))
        _eq(got[0], data, (R, kmin, t))
        if one:
            with _env(P_NOFUSE):
                assert cbr.encode_packed_rows_launches(C, pcm16=pcm16) == cbr.encode_launches(C) + 2 == 3
                comp = cbr.encode_packed_rows(x)
            assert torch.equal(comp[2], got[2]) and torch.equal(comp[0], got[0]), (R, kmin, _where(comp[0], got[0]))


@gpu
@pytest.mark.parametrize("N,C,spreading,pcm16", FUSED)
def test_fused_chunks_at_equality(N, C, spreading, pcm16):
    """``.stream(...).encode_packed_rows_chunk`` in chunks of 2 + 1 + 2 blocks and the flush (k_fwd_fast_qps / qps16) against the
    one-shot rows of ``pack_rows_reference``."""
    base, x, off, plan = _fused_case(N, C, spreading, pcm16)
    for R, kmin, t, ref in plan:
        cbr = base.with_row_budget(R, kmin)
        data, _, fits = np_rows_from_codes(ref[0], ref[1], ref[3], off, R)
        rows_ref = data.reshape(B1, K1 + 1, C, cbr.row_bytes)
        st = cbr.stream(B1, C)
        one = st.packed_chunk_launches(pcm16=pcm16) == 1
        if base.filters_n == 1024:
            assert one == (_instance(base, C) in _built16("qps16") if pcm16 else _gate_passed(cbr, C))
        else:
            assert st.packed_chunk_launches(pcm16=pcm16) == cbr.encode_launches(C) + 2 and not one
        rows, got_fits = _encode_chunks(st, x, (2, 1, 2))
        _eq(got_fits, fits, (R, kmin, t))
        _eq(rows, rows_ref, (R, kmin, t))
        if one:
            with _env(P_NOFUSE):
                st = cbr.stream(B1, C)
                assert st.packed_chunk_launches(pcm16=pcm16) == cbr.encode_launches(C) + 2 == 3
                comp, comp_fits = _encode_chunks(st, x, (2, 1, 2))
            assert torch.equal(comp_fits, got_fits) and torch.equal(comp, rows), (R, kmin, _where(comp, rows))


def _held_to(got, ref, what):
    for name, g, r in zip(("offset", "row_bits", "sf", "codes"), (got[2], got[3], got[1], got[0]), (ref[2], ref[3], ref[1], ref[0])):
        _eq(g, r, (name, what))


@gpu
@pytest.mark.parametrize("sr,N,M,C", GENERIC)
def test_generic_quantize_to_budget_at_equality(sr, N, M, C):
    """k_quantize_budget (X in registers at N = 1024 and two channels, re-read elsewhere, empty bands at N = 64) with a budget
    tensor that puts every row on its own edge, then every budget one bit less."""
    X, thr, off, R, k, at, under = _generic_case(sr, N, M, C)
    psy = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M)
    Xd, td = _dev(X), _dev(thr)
    _held_to(psy.quantize_to_budget(Xd, td, _dev(R)), at, "R")
    _held_to(psy.quantize_to_budget(Xd, td, _dev(R - 1)), under, "R - 1")


@gpu
@pytest.mark.parametrize("sr,N,M,C", REQUANT)
def test_generic_requantize_to_budget_at_equality(sr, N, M, C):
    codes, sf, off, R, k, at, under = _requant_case(sr, N, M, C)
    psy = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M)
    cd, sd = _dev(codes), _dev(sf)
    _held_to(psy.requantize_to_budget(cd, sd, _dev(R)), at, "R")
    _held_to(psy.requantize_to_budget(cd, sd, _dev(R - 1)), under, "R - 1")


@gpu
def test_transrate_at_equality():
    """``transrate_packed_rows`` of rows encoded at 2730 bits to R' = bits_r(k) at a plateau start of ``requant_fast``'s table, and
    to R' - 1: numpy, the composition and the one launch (k_transrate_p)."""
    base = audiocodec_amd.AudioCodec(48000, 1024)
    off = base.psy.scale_band_offsets
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(_x(2))
    data, index = data.cpu().numpy(), index.cpu().numpy()
    codes, sf = np_unpack(data, index, off, 1024)
    bits = requant_fast(codes, sf, off, unlimited(1024, 64), 0)[4]
    targets = bi.pick_three(bi.plateau_starts(bits, 0, hi=2730))
    print("targets:", targets)
    for t in targets:
        at = _three_ways(base.with_row_budget(t.R), data, index, off)
        assert int(at[3][t.row]) == t.k and int(at[4][t.row]) == t.R and at[2][t.row]
        under = _three_ways(base.with_row_budget(t.R - 1), data, index, off)
        assert int(under[3][t.row]) > t.k and int(under[4][t.row]) < t.R


@gpu
def test_transrate_slot_slack():
    """The slack between a budget and its slot: a row longer than R' that ends on the slot's last bit is stored (offset 254,
    fits), the same row one bit longer is the marked row; a row of exactly R' bits stays at offset 0."""
    off, R, codes, sf, lengths, data, index = _slot_case()
    base = audiocodec_amd.AudioCodec(48000, 1024)
    ref = _three_ways(base.with_row_budget(R), data, index, off)
    assert ref[2].ravel().tolist() == [True, True, False, True] and ref[3].ravel().tolist() == [0, K_MAX, K_MAX, 0]


@gpu
@pytest.mark.parametrize("sr,N,M,C", CLIP)
def test_clip_budget_edges(sr, N, M, C):
    """``quantize_to_clip_budget`` with every clip's budget on an edge of section 8d's rules: the first offset of a total and one
    bit less (rule 2), a prefix sum met exactly and one bit less (rule 3), the total at offset 254 and one bit less."""
    X, thr, off, st, T, ref = _clip_case(sr, N, M, C)
    psy = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M)
    Xd, td = _dev(X), _dev(thr)
    for name, r in ref.items():
        codes, sf, offset, row_bits, clip_bits = psy.quantize_to_clip_budget(Xd, td, _dev(T[name]))
        _eq(offset, r[2], name)
        _eq(offset[:, -1, -1], r[4], name)                   # the clip's offset: the last row never steps back
        _eq(row_bits, r[3], name)
        _eq(clip_bits, r[5], name)
        _eq(sf, r[1], name)
        _eq(codes, r[0], name)


@gpu
@pytest.mark.parametrize("sr,N,M,C", CRITERION)
def test_criterion_edges(sr, N, M, C):
    """Every band minimum pred(CRIT[s]), CRIT[s], succ(CRIT[s]) and the specials through the three kernels that call
    ``scale_factor_of`` on thresholds they are given.  (The fused encoders compute thr from PCM, so these minima cannot be
    planted there: their ``FLAT`` form of the search is held by the tests of part 1 and 4 here and by the fused-against-
    composition tests of the other files.)"""
    X, thr, off, codes, sf = _criterion_case(sr, N, M, C)
    psy = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M)
    Xd, td = _dev(X), _dev(thr)
    got = psy.quantize(Xd, td)
    _eq(got[1], sf, "quantize")
    _eq(got[0], codes, "quantize")
    got = psy.quantize_to_budget(Xd, td, unlimited(N, M))
    _eq(got[1], sf, "quantize_to_budget")
    _eq(got[0], codes, "quantize_to_budget")
    assert not bool(got[2].any())
    got = psy.quantize_to_clip_budget(Xd, td, clip_unlimited(X.shape[1], C, N, M))
    _eq(got[1], sf, "quantize_to_clip_budget")
    _eq(got[0], codes, "quantize_to_clip_budget")
    assert not bool(got[2].any())


@gpu
@pytest.mark.parametrize("N,C", TIES)
def test_ties_quantize_pack_dequantize(N, C):
    """Products of exactly k + 0.5, their neighbours, +-32767.5 and +-FLT_MAX through ``quantize``; the codes and all 255 scale
    factors through ``pack`` and ``unpack``; ``dequantize``."""
    X, thr, off, codes, sf = _tie_case(N, C)
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=N, bark_bands_n=64)
    gc, gs = psy.quantize(_dev(X), _dev(thr))
    _eq(gs, sf, "sf")
    _eq(gc, codes, "codes")
    data, index = psy.pack(gc, gs)
    rd, ri = np_pack(codes, sf, off)
    _eq(index, ri, "index")
    _eq(data, rd, "data")
    uc, us = psy.unpack(data, index)
    cc, cs = np_canon(codes, sf, off)
    _eq(us, cs, "unpacked sf")
    _eq(uc, cc, "unpacked codes")
    Xh = psy.dequantize(gc, gs).cpu().numpy()
    np.testing.assert_array_equal(Xh.view(np.uint32), np_dequantize(codes, sf, off).view(np.uint32))


@gpu
@pytest.mark.parametrize("N,C", TIES_DECODE)
def test_ties_decode_quantized(N, C):
    """The fused synthesis from codes with every scale factor from -128 to 127 (one band of the last frame holds a NaN) against
    ``decode(dequantize(...))``, float32 and 16-bit PCM; the rows budgeted to 1365 bits through ``decode_packed``."""
    X, thr, off, _, _ = _tie_case(N, C)
    X = X.copy()
    X[-1, -1, off[40], C - 1] = np.nan
    codes, sf = np_quantize(X, thr, off)
    assert set(sf.ravel().tolist()) == set(range(-128, 128))
    codec = audiocodec_amd.AudioCodec(48000, N)
    assert codec.decode_quantized_launches(C) == 1
    gc, gs = codec.psy.quantize(_dev(X), _dev(thr))
    _eq(gs, sf, "sf")
    _eq(gc, codes, "codes")
    Xh = codec.psy.dequantize(gc, gs)
    bc, bs, offset, _ = codec.psy.quantize_to_budget(_dev(X), _dev(thr), 1365)
    assert int(offset.max()) > 0
    data, index = codec.psy.pack(bc, bs)
    for pcm16 in (False, True):
        got, ref = codec.decode_quantized(gc, gs, pcm16), codec.decode(Xh, pcm16)
        assert _same(got, ref), (pcm16, _where(got, ref))
        got, ref = codec.decode_packed(data, index, pcm16), codec.decode_quantized(bc, bs, pcm16)
        assert _same(got, ref), (pcm16, "packed", _where(got, ref))
