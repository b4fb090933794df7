"""The fused quantise, pack and decode kernels at filters_n = 1024 on scale-band layouts other than 48000 Hz's, at another alpha,
and on rows with wide code fields: k_fwd_fast_q / _qb / _qp / _qps, their 16-bit-PCM twins _q16 / _qb16 / _qp16 / _qps16 and
the packed-row decode k_inv_fast_p.  What they share (ac_fast_quant_dev.h, ac_fast_fwd_qp_dev.h, ac_fast_inv_p_dev.h) is
driven by the plan's band layout: runs of lanes per band, odd bins that go to their band on their own, empty bands, band
records with signed bases.  fused_layouts.py holds the layouts, why each is in the set, and the ``tonal`` input.

Every GPU comparison is bit for bit unless a bar is named.  A fused result is held to two references: the composition of the
generic kernels on ``encode()``'s X and thr, and the numpy restatements (test_quantizer, rate_reference, pack_reference,
pack_rows_reference) on those same tensors.  References are computed once per (layout, signal, C, spreading, input format),
shared by the tests and never modified.  Before a comparison the reference alone must show what keeps it from being vacuous:
``tonal``'s rows hold wide fields (fused_layouts.assert_wide), a budget binds (test_encode_cbr._binding,
test_encode_packed_rows._not_degenerate); the printed lines name the counts.
"""

import functools

import numpy as np
import pytest
import torch

import audiocodec_amd
from oracle.audiocodec_oracle import MDCTOracle, PsychoOracle

import fused_layouts as fl
from fused_layouts import B0, K0, LAYOUT_IDS, LAYOUTS, M0, N0
from pack_reference import np_canon, np_row_bits, np_widths
from pack_rows_reference import marked_row, np_rows_from_codes, row_bytes
from rate_reference import quantize_budget
from test_decode_packed_fused import NOFUSE as DEC_NOFUSE
from test_decode_packed_fused import _designed_rows, _hold_to_composition
from test_encode_cbr import _binding, _input
from test_encode_packed_rows import CAP, _check_result, _composition, _derived_budget, _not_degenerate
from test_encode_pcm16 import _p16
from test_encode_quantized_fused import _same, _where
from test_gpu_parity import LSB, TOL, rel_elem, rel_peak, tonality_err
from test_quantizer import decode_quantized_bit_equal, np_dequantize, np_offsets, np_quantize
from test_stream_packed import _decode_chunks, _encode_chunks

gpu = pytest.mark.gpu
BY_ID = {l[0]: l for l in LAYOUTS}
BY_ID["48000"] = ("48000", 48000, 0.6)                       # no case of this file: test_conceal_layouts.py takes _ref there
SIGNALS = ("noise", "tonal")
CHUNKS = (2, 1, 2)
FORMS = [(spreading, pcm16) for spreading in (None, "f32") for pcm16 in (False, True)]


# ---- CPU: the layouts, the EMPTY search on host offsets, the condition on ``tonal`` -----------------------------------
@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_layout_facts(layout):
    """The counts that say why the layout is in the set, from np_offsets; the library's host offsets are the same layout."""
    sr, _ = fl.resolve(BY_ID[layout])
    ref = np_offsets(sr, N0, M0)
    off = fl.host_offsets(sr)
    np.testing.assert_array_equal(off, ref)
    empty, one_bin, split = fl.layout_counts(ref)
    L = np.diff(ref)
    print("%s (%d Hz): %d empty bands, %d one-bin bands, %d granules in two bands, longest band %d, first lengths %s"
          % (layout, sr, empty, one_bin, split, int(L.max()), L[:6].tolist()))
    assert fl.layout_counts(off) == (empty, one_bin, split)
    if layout == fl.EMPTY:
        assert empty >= 1 and one_bin >= 11 and L[:6].min() == 0 and L[:6].max() == 1
        j = int(np.flatnonzero(L == 0)[0])
        assert 0 < j < M0 - 1 and L[j - 1] > 0 and L[j + 1] > 0   # (its neighbours hold bins: test_designed_rows' row)
    else:
        assert (empty, one_bin, int(L.max()), tuple(L[:6].tolist())) == fl.FACTS[sr]
    assert split >= 16                                           # odd bins that go to their band on their own, in every layout
    assert fl.layout_counts(np_offsets(48000, N0, M0))[:2] == (0, 1)   # ... and what the other tests' layout has of these


def test_every_candidate_rate_has_an_empty_band():
    for sr in fl.EMPTY_RATES:
        off = fl.host_offsets(sr)
        assert fl.has_empty_band(off), sr
        np.testing.assert_array_equal(off, np_offsets(sr, N0, M0))
    assert fl.empty_rate() in fl.EMPTY_RATES


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_tonal_holds_wide_fields_on_the_numpy_oracle(layout, C):
    """The condition on ``tonal`` through the float32 numpy oracle and np_quantize, for the float32 signal and its int16 PCM."""
    sr, alpha = fl.resolve(BY_ID[layout])
    off = fl.host_offsets(sr)
    x = fl.tonal(C)
    assert x.dtype == np.float32 and x.shape == (B0, K0 * N0, C) and float(np.abs(x).max()) <= 1.0
    for name, sig in (("float32", x), ("int16", fl.tonal16(C).astype(np.float32) / np.float32(32768))):
        codes, sf = fl.oracle_codes(sig, sr, alpha, off)
        hist = fl.assert_wide(codes, sf, off)
        bits = np_row_bits(codes, sf, off)
        print("%s C=%d %s: widths %s, rows of %d..%d bits" % (layout, C, name, hist, bits.min(), bits.max()))


# ---- GPU: references, computed once -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base(layout, spreading):
    sr, alpha = fl.resolve(BY_ID[layout])
    return audiocodec_amd.AudioCodec(sr, N0, alpha=alpha, spreading=spreading)


@functools.lru_cache(maxsize=None)
def _at_48000(spreading):
    return audiocodec_amd.AudioCodec(48000, N0, spreading=spreading)


@functools.lru_cache(maxsize=None)
def _signal(signal, C, pcm16):
    """noise: test_encode_cbr's ``_input`` (a zero frame, NaN, Inf, the 1e15 and the 3e12 samples), as int16 test_encode_pcm16's
    ``_p16`` (zero blocks, both rails); tonal: fused_layouts.tonal / tonal16."""
    if signal == "noise":
        return _p16(C, B0, K0) if pcm16 else _input(C, B0, K0, C + 2 * B0 + K0, True)
    return torch.from_numpy(fl.tonal16(C) if pcm16 else fl.tonal(C)).cuda()


class _Ref:
    """The references of one (layout, signal, C, spreading, input format): encode()'s X and thr, the composition's and numpy's
    plain codes, and per budget (on first use) the composition's and numpy's codes, offsets, lengths and rows."""

    def __init__(self, layout, signal, C, spreading, pcm16):
        self.key = (layout, signal, C, spreading, "int16" if pcm16 else "float32")
        self.base = _base(layout, spreading)
        self.off = self.base.psy.scale_band_offsets
        self.signal, self.C, self.pcm16, self.spreading = signal, C, pcm16, spreading
        self.x = _signal(signal, C, pcm16)
        self.X, _, self.thr = self.base.encode(self.x)
        self.Xn, self.tn = self.X.cpu().numpy(), self.thr.cpu().numpy()
        self.codes, self.sf = self.base.psy.quantize(self.X, self.thr)
        self.np_codes, self.np_sf = np_quantize(self.Xn, self.tn, self.off)
        self.hist = None
        if signal == "tonal":                                    # the condition on tonal, on the composition's codes
            self.hist = fl.assert_wide(self.codes.cpu().numpy(), self.sf.cpu().numpy(), self.off)
        self.Rs, self.median_bits = _derived_budget(self.base, self.x, 0.0)
        assert 2 * 5 * M0 <= self.Rs <= CAP, (self.Rs, self.median_bits)
        # (row_bits, min_offset): the minimum, the 32-bit-rounded median row, half of it, the packer's cap, one negative floor
        self.budgets = [(5 * M0, 0), (self.Rs, 0), (self.Rs // 2, 0), (CAP, 0), (self.Rs, -8)]
        self._budget = {}

    def budget(self, R, kmin):
        if (R, kmin) not in self._budget:
            rc, rs, ro, rbits = self.base.psy.quantize_to_budget(self.X, self.thr, R, kmin)
            nc, ns, no, nb = quantize_budget(self.Xn, self.tn, self.off, R, kmin)
            data, index, fits = np_rows_from_codes(nc, ns, nb, self.off, R)
            self._budget[(R, kmin)] = {"comp": (rc, rs, ro, rbits), "np": (nc, ns, no, nb), "np_rows": (data, index, fits)}
            self._preconditions(R, kmin)
        return self._budget[(R, kmin)]

    def _preconditions(self, R, kmin):
        """On the references alone (numpy's offsets and lengths, the composition's for _not_degenerate): the budget binds as
        far as the input allows.  Prints the counts that show it."""
        e = self._budget[(R, kmin)]
        rc, rs, ro, rbits = e["comp"]
        nc, ns, no, nb = e["np"]
        fits = e["np_rows"][2]
        rb = row_bytes(R)
        between = int(((no > kmin) & (no < 254)).sum())
        print("%s R=%d kmin=%d: %d rows, %d at min_offset, %d between, %d at 254, %d do not fit, offsets %d..%d, longest %d bits"
              % (self.key, R, kmin, no.size, int((no == kmin).sum()), between, int((no == 254).sum()), int((~fits).sum()),
                 no.min(), no.max(), nb.max()))
        derived = (R, kmin) == (self.Rs, 0)
        cfits = rbits <= 8 * rb
        if self.signal == "noise" and not self.pcm16:
            # _binding wants a row at 254 with its budget unmet.  On the GPU the 1e15 sample's rows store nothing, so that row is
            # the 3e12 sample's: |X| about 2e9 against the largest step 2^(127 / 4) = 3.6e9 leaves codes of -1, 0, 1, a row of
            # about 2.5 kbit -- over the minimum and over half the median everywhere, under the median row of the layouts with
            # long rows (8000, 44100).  At the median budget the row counts at and above min_offset are what must show
            if R in (5 * M0, self.Rs // 2):
                _binding(R, kmin, no, nb)
            elif R == self.Rs:
                assert int((no == kmin).sum()) >= 1 and between >= 1, "the median budget does not bind"
            _not_degenerate(R, kmin, derived, cfits, ro, rbits, rb)
        else:                                                    # no NaN, Inf or huge sample: every row fits
            assert fits.all()
            if derived:
                _not_degenerate(R, kmin, True, cfits, ro, rbits, rb)
            if R == self.Rs // 2:
                assert int((no > kmin).sum()) >= 1, "no row above min_offset"
            if R == self.Rs:
                assert int((no == kmin).sum()) >= 1, "no row at min_offset"


@functools.lru_cache(maxsize=None)
def _ref(layout, signal, C, spreading, pcm16):
    return _Ref(layout, signal, C, spreading, pcm16)


def _eq_np(got, want, what):
    np.testing.assert_array_equal(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want, err_msg=str(what))


@functools.lru_cache(maxsize=None)
def _at_48000_launches(spreading, C):
    return _launches(_at_48000(spreading), C)


def _tag(name, pcm16):
    return name + ("[pcm16]" if pcm16 else "")


CASES = [(layout, signal, C) for layout in LAYOUT_IDS for signal in SIGNALS for C in (1, 2)]


# ---- GPU: the search, the launch counts ---------------------------------------------------------------------------------
@gpu
def test_an_empty_band_layout_runs_in_one_launch():
    sr = fl.empty_rate()
    print("EMPTY: %s Hz" % sr)
    assert sr in fl.EMPTY_RATES
    assert fl.has_empty_band(fl.host_offsets(sr))
    codec = audiocodec_amd.AudioCodec(sr, N0)
    assert codec.encode_quantized_launches(1) == 1 and codec.encode_quantized_launches(2) == 1 and codec.psy.is_fast()


def _launches(codec, C):
    """Every launch query of the kernels under test on a codec and on its budgeted form, by name."""
    cbr = codec.with_row_budget(1365)
    st = cbr.stream(B0, C)
    out = {}
    for pcm16 in (False, True):
        tag = "[pcm16]" if pcm16 else ""
        out["encode_quantized" + tag] = codec.encode_quantized_launches(C, pcm16=pcm16)
        out["encode_quantized@budget" + tag] = cbr.encode_quantized_launches(C, pcm16=pcm16)
        out["encode_packed_rows" + tag] = cbr.encode_packed_rows_launches(C, pcm16=pcm16)
        out["packed_chunk" + tag] = st.packed_chunk_launches(pcm16=pcm16)
    out["decode_packed"] = codec.decode_packed_launches(C)
    out["packed_chunk[decode]"] = st.packed_chunk_launches(decode=True)
    return out


@gpu
@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_launch_counts(layout, monkeypatch):
    """One launch wherever 48000 Hz takes one: none of the tests below may fall back to the composition unnoticed."""
    for name in ("AC_ENCODE_QUANT_NOFUSE", "AC_ENCODE_PACKED_NOFUSE", DEC_NOFUSE):
        monkeypatch.delenv(name, raising=False)
    for spreading in (None, "f32"):
        for C in (1, 2):
            got, ref = _launches(_base(layout, spreading), C), _at_48000_launches(spreading, C)
            print("%s spreading=%s C=%d: %s" % (layout, spreading, C, got))
            for name, n in ref.items():
                assert got[name] == n, (layout, spreading, C, name, got[name], n)
            if spreading is None:                                # the default product runs every family in one launch
                assert set(got.values()) == {1}, got


# ---- 1. anchor: encode() at these layouts against the float64 oracle ------------------------------------------------------
# (X, thr) bars per layout.  A layout would get twice the unfused float32 calls' measured error if that exceeded TOL / 2
# against the oracle there.  Measured on the MI355X over all layouts (the printed lines): X 1.9e-7, tonality 0.11 of its bar,
# thresholds 5.4e-6 -- far below TOL / 2 = 5e-5, so every layout keeps TOL.
ANCHOR_BARS = {layout: (TOL, TOL) for layout in LAYOUT_IDS}


@gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_encode_against_the_oracle(layout, C):
    """test_gpu_parity.test_encode_fused_equals_unfused_and_oracle at the layout's sample rate and alpha: the spectra and
    thresholds every reference below starts from."""
    sr, alpha = fl.resolve(BY_ID[layout])
    xbar, thrbar = ANCHOR_BARS[layout]
    B, K = B0, K0
    rng = np.random.default_rng(11 + B)
    x = rng.uniform(-1, 1, (B, K * N0, C)).astype(np.float32)
    x[0, : 2 * N0, 0] *= 1e-3
    codec = _base(layout, None)
    xd = torch.from_numpy(x).cuda()
    assert codec.encode_launches(C) == 1
    X, t, thr = codec.encode(xd, drown=0.2)
    Xu = codec.mdct.transform(xd)
    tu = codec.psy.tonality(Xu)
    thru = codec.psy.global_masking_threshold(Xu, tu, 0.2)
    om = MDCTOracle(N0, "vorbis", np.float64)
    op = PsychoOracle(sr, N0, M0, alpha=alpha, compute_dtype=np.float64)
    Xo = om.transform(x.astype(np.float64))
    to = op.tonality(Xo)
    thro = op.global_masking_threshold(Xo, to, 0.2)
    host = lambda v: v.cpu().numpy()   # noqa: E731
    unfused = (rel_peak(host(Xu), Xo), tonality_err(host(tu), to), rel_elem(host(thru), thro))
    fused = (rel_peak(host(X), Xo), tonality_err(host(t), to), rel_elem(host(thr), thro))
    print("%s C=%d against the oracle: unfused X %.2e t %.2e thr %.2e; fused X %.2e t %.2e thr %.2e"
          % ((layout, C) + unfused + fused))
    assert float((X - Xu).abs().max()) <= 1e-6
    assert tonality_err(t, tu) <= 1.0
    assert float(((thr - thru).abs() / thru).max()) <= TOL
    assert fused[0] <= xbar
    assert fused[1] <= 1.0
    assert fused[2] <= thrbar
    xh = host(codec.decode(X))
    assert np.max(np.abs(xh[:, N0:-N0] - x)) <= LSB


# ---- 2. codes: k_fwd_fast_q / _qb / _q16 / _qb16 ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("layout,signal,C", CASES)
def test_codes(layout, signal, C, monkeypatch):
    monkeypatch.delenv("AC_ENCODE_QUANT_NOFUSE", raising=False)
    for spreading, pcm16 in FORMS:
        r = _ref(layout, signal, C, spreading, pcm16)
        expect = _at_48000_launches(spreading, C)
        assert r.base.encode_quantized_launches(C, pcm16=pcm16) == expect[_tag("encode_quantized", pcm16)], r.key
        if r.hist is not None:
            print("%s widths of the composition's codes: %s" % (r.key, r.hist))
        # the two references agree, then the fused launch equals both
        _eq_np(r.sf, r.np_sf, r.key)
        _eq_np(r.codes, r.np_codes, r.key)
        codes, sf = r.base.encode_quantized(r.x)
        assert codes.dtype == torch.int16 and codes.shape == (B0, K0 + 1, N0, C) and sf.shape == (B0, K0 + 1, M0, C)
        assert torch.equal(sf, r.sf), (r.key, _where(sf, r.sf))
        assert torch.equal(codes, r.codes), (r.key, _where(codes, r.codes))
        assert int(codes.abs().max()) > 0
        if signal == "noise" and not pcm16:
            assert bool((sf == -128).any()) and int(codes[1, 2].abs().max()) == 0
        for R, kmin in r.budgets:
            cbr = r.base.with_row_budget(R, kmin)
            assert cbr.encode_quantized_launches(C, pcm16=pcm16) == expect[_tag("encode_quantized@budget", pcm16)], (r.key, R)
            e = r.budget(R, kmin)
            for got, want, name in zip(e["comp"], e["np"], ("codes", "sf", "offset", "row_bits_out")):
                _eq_np(got, want, r.key + (R, kmin, name))
            codes, sf = cbr.encode_quantized(r.x)
            assert torch.equal(sf, e["comp"][1]), (r.key, R, kmin, _where(sf, e["comp"][1]))
            assert torch.equal(codes, e["comp"][0]), (r.key, R, kmin, _where(codes, e["comp"][0]))
            if (R, kmin) == (CAP, 0) and (signal == "tonal" or int(e["np"][2].max()) == 0):
                # longer than any row of tonal: every offset 0, the unbudgeted codes
                assert int(e["np"][2].max()) == 0 and torch.equal(codes, r.codes) and torch.equal(sf, r.sf)


# ---- 3. rows: k_fwd_fast_qp / _qp16 ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("layout,signal,C", CASES)
def test_rows(layout, signal, C, monkeypatch):
    monkeypatch.delenv("AC_ENCODE_PACKED_NOFUSE", raising=False)
    for spreading, pcm16 in FORMS:
        r = _ref(layout, signal, C, spreading, pcm16)
        for R, kmin in r.budgets:
            cbr = r.base.with_row_budget(R, kmin)
            rb = cbr.row_bytes
            assert cbr.encode_packed_rows_launches(C, pcm16=pcm16) == \
                _at_48000_launches(spreading, C)[_tag("encode_packed_rows", pcm16)], (r.key, R)
            e = r.budget(R, kmin)
            nc, ns, no, nb = e["np"]
            data, index, fits = e["np_rows"]
            comp = _composition(cbr, r.x)
            _check_result(cbr, r.x, comp)
            for got, want, name in zip(comp, (data, index, fits), ("data", "index", "fits")):
                _eq_np(got, want, r.key + (R, kmin, "composition", name))
            fused = cbr.encode_packed_rows(r.x)
            _check_result(cbr, r.x, fused)
            assert torch.equal(fused[2], comp[2]), (r.key, R, kmin, _where(fused[2], comp[2]))
            assert torch.equal(fused[1], comp[1])
            assert torch.equal(fused[0], comp[0]), (r.key, R, kmin, _where(fused[0], comp[0]))
            # the rows read back: the canonical reference codes where the row fits, the marked row where it does not
            uc, us = (v.cpu().numpy() for v in cbr.psy.unpack(fused[0], fused[1]))
            cc, cs = np_canon(nc, ns, r.off)
            fc, fs = np.broadcast_to(fits[:, :, None, :], uc.shape), np.broadcast_to(fits[:, :, None, :], us.shape)
            np.testing.assert_array_equal(us[fs], cs[fs])
            np.testing.assert_array_equal(uc[fc], cc[fc])
            assert (us[~fs] == -128).all() and not uc[~fc].any()
            got = fused[0].cpu().numpy().reshape(-1, rb)
            for row in np.flatnonzero(~fits.ravel()):
                np.testing.assert_array_equal(got[row], marked_row(M0, R))


# ---- 4. chunks: k_fwd_fast_qps / _qps16 ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("layout,signal,C", CASES)
def test_chunks(layout, signal, C, monkeypatch):
    """Chunks of (2, 1, 2) blocks and a flushing zero block against the one-shot rows.  Where the library holds no one-launch
    instance for a form (packed_chunk_launches says 3, as it does at 48000 Hz) the call is the composition, held to the same rows."""
    monkeypatch.delenv("AC_ENCODE_PACKED_NOFUSE", raising=False)
    for spreading, pcm16 in FORMS:
        r = _ref(layout, signal, C, spreading, pcm16)
        for R, kmin in r.budgets:
            cbr = r.base.with_row_budget(R, kmin)
            data, _, ref_fits = cbr.encode_packed_rows(r.x)
            ref_rows = data.view(B0, K0 + 1, C, cbr.row_bytes)
            _eq_np(data, r.budget(R, kmin)["np_rows"][0], r.key + (R, kmin, "one-shot"))
            st = cbr.stream(B0, C)
            n = st.packed_chunk_launches(pcm16=pcm16)
            assert n == _at_48000_launches(spreading, C)[_tag("packed_chunk", pcm16)], (r.key, R)
            assert n in (1, cbr.encode_launches(C) + 2)
            rows, fits = _encode_chunks(st, r.x, CHUNKS)
            assert torch.equal(fits, ref_fits), (r.key, R, kmin, n, _where(fits, ref_fits))
            assert torch.equal(rows, ref_rows), (r.key, R, kmin, n, _where(rows, ref_rows))


# ---- 5. decode: k_inv_fast_p ------------------------------------------------------------------------------------------------------
def _hold_to_the_oracle(codec, off, data, index, pcm, what):
    """float32 PCM of decode_packed against MDCTOracle(float64).inverse_transform(np_dequantize(the rows' codes)): the rows as
    psy.unpack reads them, held by _hold_codes_to_the_oracle."""
    codes, sf = (v.cpu().numpy() for v in codec.psy.unpack(data, index))
    return _hold_codes_to_the_oracle(codes, sf, off, pcm, what)


def _hold_codes_to_the_oracle(codes, sf, off, pcm, what):
    """float32 PCM decoded from codes int16 [B, F, N0, C] and sf int8 [B, F, M0, C] (numpy) against
    MDCTOracle(float64).inverse_transform(np_dequantize(codes, sf)).  The bar is the existing decode tests' for signals within
    full scale, one LSB of 16-bit PCM; the synthesis is linear, so for a block whose reference peaks above 1 (the 3e12 sample of
    ``noise``) the bar scales with that peak.  Blocks under a frame with a NaN band (a frame covers two blocks) are left out."""
    Xh = np_dequantize(codes, sf, off).astype(np.float64)
    bad = np.isnan(Xh).any(axis=2)                               # [B, F, C]
    ref = MDCTOracle(N0, "vorbis", np.float64).inverse_transform(np.where(np.isnan(Xh), 0.0, Xh))
    B, F, C = bad.shape
    nan_block = np.zeros((B, F + 1, C), dtype=bool)
    nan_block[:, :-1] |= bad
    nan_block[:, 1:] |= bad
    got = pcm.cpu().numpy().astype(np.float64).reshape(B, F + 1, N0, C)
    ref = ref.reshape(B, F + 1, N0, C)
    assert np.array_equal(np.isnan(got).any(axis=2), nan_block), what
    err = np.abs(got - ref).max(axis=2)
    bar = LSB * np.maximum(1.0, np.abs(ref).max(axis=2))
    keep = ~nan_block
    assert keep.sum() >= keep.size // 3, what
    worst = float((err[keep] / bar[keep]).max())
    assert worst <= 1.0, (what, worst)
    return worst


@gpu
@pytest.mark.parametrize("layout,signal,C", CASES)
def test_decode(layout, signal, C, monkeypatch):
    """decode_packed on the dense stream of the unbudgeted codes and on the fixed-stride rows of every budget: against
    unpack + decode_quantized (both PCM formats), in chunks of (2, 1, 2) frames against the one-shot blocks, and the float32 PCM
    against the float64 oracle on the numpy dequantiser's spectra."""
    monkeypatch.delenv(DEC_NOFUSE, raising=False)
    r = _ref(layout, signal, C, None, False)
    codec = r.base
    assert codec.decode_packed_launches(C) == 1
    streams = [("dense", codec) + tuple(codec.psy.pack(r.codes, r.sf))]
    for R, kmin in r.budgets:
        cbr = codec.with_row_budget(R, kmin)
        data, index, _ = cbr.encode_packed_rows(r.x)
        _eq_np(data, r.budget(R, kmin)["np_rows"][0], r.key + (R, kmin))
        streams.append(("R=%d kmin=%d" % (R, kmin), cbr, data, index))
    for name, c, data, index in streams:
        pcm = _hold_to_composition(c, data, index)
        worst = _hold_to_the_oracle(c, r.off, data, index, pcm, r.key + (name,))
        print("%s %s: float32 PCM within %.3f of its bar against the oracle" % (r.key, name, worst))
        part = index[:, :K0].contiguous()
        for pcm16 in (False, True):
            ref = c.decode_packed(data, part, pcm16)[:, :K0 * N0]
            st = c.stream(B0, C)
            assert st.packed_chunk_launches(decode=True) == 1
            got = _decode_chunks(st, data, part, CHUNKS, pcm16)
            assert _same(got, ref.contiguous()), (r.key, name, pcm16, _where(got, ref.contiguous()))


@gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_designed_rows(layout, C, monkeypatch):
    """test_decode_packed_fused.test_designed_rows' generator on the layout's offsets: every width 0..16 and 31 with the extreme
    codes, the shortest and the longest rows; at EMPTY also a row whose bands beside the empty one carry widths 16 and 1."""
    monkeypatch.delenv(DEC_NOFUSE, raising=False)
    sr, alpha = fl.resolve(BY_ID[layout])
    psy, off, codes, sf = _designed_rows(C, sr)
    L = np.diff(off)
    if layout == fl.EMPTY:
        j = int(np.flatnonzero(L == 0)[0])
        codes[0, 0, off[j - 1]:off[j], 0] = -32768
        codes[0, 0, off[j + 1]:off[j + 2], 0] = -1
        sf[0, 0, j - 1:j + 2, 0] = (7, 9, -3)
    w = np_widths(codes, sf, off)
    if layout == fl.EMPTY:
        assert w[0, 0, j - 1:j + 2, 0].tolist() == [16, 0, 1]
        assert (L == 0).any()
    assert set(np.unique(w[..., L > 0, :]).tolist()) == set(range(17)) | {31}
    assert (codes == -32768).any() and (codes == 32767).any() and (codes == -32767).any()
    bits = np_row_bits(codes, sf, off)
    assert bits.min() == 5 * M0 and bits.max() == 5 * M0 + 8 * int((L > 0).sum()) + 16 * N0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    codec = _base(layout, None)
    np.testing.assert_array_equal(codec.psy.scale_band_offsets, off)
    data, index = psy.pack(dev(codes), dev(sf))
    out = _hold_to_composition(codec, data, index)
    assert torch.isnan(out).any() and torch.isfinite(out).any()
    uc, us = (v.cpu().numpy() for v in codec.psy.unpack(data, index))
    cc, cs = np_canon(codes, sf, off)
    np.testing.assert_array_equal(us, cs)
    np.testing.assert_array_equal(uc, cc)


# ---- 6. decode_quantized at filters_n = 2048: its loads dequantise by band ----------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("sr", [44100, 96000])
def test_decode_quantized_at_2048(sr, C):
    """test_quantizer.test_decode_quantized_bit_equal's body at other sample rates, then against the numpy dequantiser: bit for
    bit through decode(), and within one LSB of the float64 oracle's synthesis."""
    codec, codes, sf = decode_quantized_bit_equal(2048, C, 1, sr=sr)
    off = codec.psy.scale_band_offsets
    np.testing.assert_array_equal(off, np_offsets(sr, 2048, M0))
    print("%d Hz at 2048: (empty, one-bin, split granules) = %s" % (sr, fl.layout_counts(off)))
    Xh = np_dequantize(codes.cpu().numpy(), sf.cpu().numpy(), off)
    assert np.isfinite(Xh).all() and np.abs(Xh).max() > 0
    got = codec.decode_quantized(codes, sf)
    assert torch.equal(got, codec.decode(torch.from_numpy(Xh).cuda()))
    ref = MDCTOracle(2048, "vorbis", np.float64).inverse_transform(Xh.astype(np.float64))
    assert np.max(np.abs(got.cpu().numpy() - ref)) <= LSB
