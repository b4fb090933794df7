"""Protected rows and the recovering decode (k_protect_p, k_inv_fast_plr) on copies that carry content,
on other band layouts, with the redundant budget above the row budget and at the packer's cap, and with the copy ending where
``data`` ends.

Why: the recovering tests of test_protect.py protect at R2 = 341 (``_slots``, the strip-crossing shapes, the ABI, graph,
stream-contract and chain tests; 400 on the composition only), and a 341-bit copy has 21 bits behind its 320-bit header: room
for one scale factor and 13 code bits.  test_a_341_bit_copy_stores_at_most_one_band holds that on the numpy oracle's codes; on
the noise ``_slots`` uses and on ``tonal`` at 48000 Hz no copy stores a band at all.  A recovered row there is 64 widths of 0 and
its frame is silence, whether the kernel read the copy, muted the row, read it a few words off or faded it.  What of a recovered
row's content test_protect.py does see, scratch build A below shows: the 8320 and 12513 rows of test_recover_across_strips --
64 and 96 frames of noise ramped up to full scale, where on the numpy oracle a few 341-bit copies in a hundred store their
one band -- and one odd ``redundant_at`` of test_recover_redundant_at_cases, which reads primary rows off the byte phase.  No
test there recovers from a copy with more than one band or with a code field across a word boundary, and none runs the
one-launch protect with R2 above R or compares its bytes at the cap.  Here the copies hold many bands, and numpy's reading of the bytes
must show so before a kernel result is looked at (protect_layouts.hold_conditions).

  1. (CPU) the fact above.
  2. Encoded ``tonal`` and ``noise`` at 8000, 44100, 96000, EMPTY and 48000 Hz, mono and stereo, B = 3, six frames, as the dense
     pack and as rows at 2730 bits: protected at R = 1365 with R2 = 1365 and 2730 (above R on purpose) -- the one launch, the
     composition and np_protect -- then recovered over test_protect's patterns at max_age 1 and 8 in both output formats: the
     kernel, the composition and decode_quantized of the numpy-planned rows, the plain decode on a substituted index wherever
     every lost row is recovered, and for ``tonal`` the float32 PCM against the float64 oracle at one LSB of 16-bit PCM times
     max(1, peak of the reference block).
  3. Designed rows (every width 0..16 and 31, the extreme codes, the shortest and longest rows, EMPTY's 16/0/1 row) as copies:
     np_protect at R = R2 = 17216 keeps every row's bytes (up to section 8e's clamp, below), and the base codec recovers
     from them.
  4. 48000 Hz, the copy in the last slot of ``data``: copies of 32 W .. 32 (W - 3) bits at W = 43 and 512 words and the 538-word
     row, ``data`` whole and trimmed by 4 and 3 bytes.  parse_strip_p gives a row plain loads where a + 4 (nw + 2) <= nbytes, so
     the last copy takes them exactly when it has at most 32 (W - 2) bits (trimmed: 32 (W - 3)); every case names its path.
  5. Protect at R2 = AC_PACK_ROWS_MAX_BITS: the redundant pack fills the whole staged slot.

Every GPU comparison between the kernel, the composition and numpy is bit for bit, float32 and 16-bit PCM.  The tests not
marked ``gpu`` hold the conditions on the numpy oracle's codes and on the designed bytes.

That the file bites (scratch builds of the library, each with one change that stays inside every buffer; this file and
test_protect.py run once against each on the MI355X):
  * parse_strip_p's ``recover`` branch no longer sets ``age = 0`` (a recovered row is faded as the concealed row it would have
    been): all 20 cases of test_protect_and_recover_encoded_signals, the 10 of test_designed_rows_as_copies and the 24 of
    test_the_copy_at_the_end_of_data fail, each at its first kernel-against-composition comparison; test_protect_at_the_cap
    and test_the_slots_of_test_protect_hold_empty_copies pass.  test_protect.py does not pass as a whole: the two cases of
    test_recover_across_strips and test_recover_redundant_at_cases (``redundant_at`` 6475) fail, its other 45 GPU tests pass --
    among them every case of test_recover_fused_composition_numpy, both chain cases, the ABI, graph and stream-contract tests.
  * protect_pack zeroes only ``row_bytes >> 2`` words of the staged slot before the second pack: the 20 cases of
    test_protect_and_recover_encoded_signals fail, each at R2 = 2730 in the bytes of ``data`` (kernel against composition),
    test_the_copy_at_the_end_of_data[512-1-middle] and [512-2-middle] (the protect at R2 = 16384 that makes their slots) and
    test_protect_at_the_cap[1365] and [320]; nothing at R2 <= R fails -- test_protect_at_the_cap[16384], W = 43 (R2 = 1376: 43
    words, as R has) -- and test_protect.py passes.
No kernel was found wrong: every comparison of this file holds on the library as it is.  Two statements about the reference
were put right on the way: requantising at offset 0 returns -32768 as -32767 and clears a -128 in an empty band (section 8e), so
a designed row's copy is its bytes only up to that (_designed_slots asserts the exact bytes), and the 538-word row of part 4
is written with -32767 in place of -32768.
"""

import functools

import numpy as np
import pytest
import torch

import audiocodec_amd

import boundary_inputs as bi
import fused_layouts as fl
import protect_layouts as pl
import test_conceal_layouts as tcl
import test_fused_layouts as tfl
from conceal_reference import np_conceal_plan, np_fade
from pack_reference import np_canon, np_code_fields, np_pack, np_row_bits, np_unpack, np_widths, unzz, zz
from pack_rows_reference import row_bytes
from protect_reference import np_protect, np_recover_plan, np_recover_src_index
from stream_order import same_bits
from test_protect import (CAP, NAMES, NOFUSE, _adversarial, _dev, _hold, _lost, _patterns, _protect3,
                          _slots, _substituted)
from transrate_reference import np_transrate

gpu = pytest.mark.gpu
N0, M0, B0, K0 = fl.N0, fl.M0, fl.B0, fl.K0
F0 = K0 + 1
LAYOUT_IDS = tcl.LAYOUT_IDS
R1 = 1365                                                        # the row budget of parts 2, 4 and 5
RB1 = row_bytes(R1)
REDS = (1365, 2730)
LONGEST = 5 * M0 + 8 * M0 + 16 * N0                              # 17216 bits, 538 words


def _pats(C, F=F0):
    return lambda max_age: _patterns(B0, F, C, max_age)


# ---- 1. CPU: the fact this file exists for ----------------------------------------------------------------------------------
@pytest.mark.parametrize("signal,C,Kp", [("noise", 1, 7), ("noise", 2, 7), ("noise", 2, 12), ("tonal", 1, F0), ("tonal", 2, F0)])
def test_a_341_bit_copy_stores_at_most_one_band(signal, C, Kp):
    """np_transrate at 341 bits -- the redundant part test_protect.py recovers from everywhere -- on the numpy oracle's codes
    of ``_slots``' noise and of ``tonal`` at 48000 Hz: no row keeps more than one stored band, and a row that keeps none is
    all zero bytes.  On the noise no row keeps one.  For test_protect.py this means that the PCM of a recovered frame is
    silence whatever the kernel did with the copy: read it, muted the row, read it some words off or faded it.  Its recovering
    tests hold the plan and the addresses, not what a copy with code fields decodes to; parts 2 to 4 of this file do."""
    off = fl.host_offsets(48000)
    x = pl.slots_noise(C, Kp) if signal == "noise" else fl.tonal(C)
    codes, sf = fl.oracle_codes(x, 48000, 0.6, off)
    assert codes.shape == (3, Kp, N0, C)
    data, index = np_pack(codes, sf, off)
    red, ridx, fits, offset, bits = np_transrate(data, index, off, N0, 341)
    w = np_widths(*np_unpack(red, ridx, off, N0), off)
    stored = pl.stored_bands(w)
    print("%s C=%d: %d rows, %d store a band, offsets %d..%d" % (signal, C, stored.size, int((stored > 0).sum()), offset.min(), offset.max()))
    assert fits.all() and not (w == 31).any()
    assert int(stored.max()) <= 1
    rows = red.reshape(3, Kp, C, row_bytes(341))
    assert not rows[stored == 0].any()
    if signal == "noise":
        assert int(stored.max()) == 0
    assert int(pl.stored_bands(np_widths(codes, sf, off)).min()) >= 8      # (the rows themselves hold many bands)


# ---- 2. CPU: tonal's copies at R2 = 1365 and 2730 carry content ---------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_tonal_copies_carry_content_on_the_numpy_oracle(layout, C):
    sr, alpha, off = tcl._offsets(layout)
    codes, sf = fl.oracle_codes(fl.tonal(C), sr, alpha, off)
    assert not (np_widths(codes, sf, off) == 31).any()
    data, index = np_pack(codes, sf, off)
    for R2 in REDS:
        ref = np_protect(data, index, off, N0, R1, R2)
        pl.hold_conditions(ref[0], ref[1], RB1, off, _pats(C), (layout, C, R2), red_offset=ref[5] if R2 == R1 else None)


# ---- 3. CPU: the designed rows as copies --------------------------------------------------------------------------------------
def _designed_lost(C):
    """Every second frame lost -- each recovered; and the same with a run of three in clip 1 (frames 4 .. 6: the last one
    recovered, the others concealed from frame 3, a longest row, at ages 1 and 2)."""
    every = _lost(tcl.F12, range(0, tcl.F12, 2), B0, C)
    run = every.copy()
    run[1, 5] = 1
    return {"every second": every, "and a run of three": run}


@functools.lru_cache(maxsize=None)
def _designed_slots(layout, C):
    """np_protect at R = R2 = 17216 of test_conceal_layouts._designed's rows, and the conditions on it: every row fits, so both
    parts are the input row's bytes as section 8e requantises them at offset 0, then zeros; the recovered rows take in the
    shortest and the longest row, the row with a
    width-31 band and, at EMPTY, the 16/0/1 row."""
    off, codes, sf, data, index, _, j = tcl._designed(layout, C)
    tcl._designed_conditions(layout, C)
    rb = row_bytes(LONGEST)
    ref = np_protect(data, index, off, N0, LONGEST, LONGEST)
    assert ref[2].all() and ref[3].all() and not ref[4].any() and not ref[5].any()
    slots = ref[0].reshape(B0, tcl.F12, C, 2 * rb)
    bits = np_row_bits(codes, sf, off)
    nb = (bits + 31) // 32 * 4
    # requantising at offset 0 is clamp(q, +-32767) (section 8e): the one code of these rows no quantiser writes, -32768, comes
    # back as -32767 at the same width, and an empty band's sf of -128 as 0 (rule 1: width 31 -> 0).  So a row's bytes are those
    # of its codes clamped and its empty bands cleared; a row with neither keeps its own
    sf1 = sf.copy()
    sf1[:, :, np.diff(off) == 0] = 0
    clamped, cidx = np_pack(np.maximum(codes, -32767), sf1, off)
    assert np.array_equal(cidx, index) and not np.array_equal(clamped, data)
    assert np.array_equal(np_row_bits(np.maximum(codes, -32767), sf1, off), bits)
    changed = (np_canon(codes, sf, off)[0] == -32768).any(axis=2) | ((sf == -128) & (sf1 == 0)).any(axis=2)    # [B, F, C]
    assert changed.any() and not changed.all()
    for b in range(B0):
        for f in range(tcl.F12):
            for c in range(C):
                row = clamped[index[b, f, c]:index[b, f, c] + nb[b, f, c]]
                assert np.array_equal(row, data[index[b, f, c]:index[b, f, c] + nb[b, f, c]]) != changed[b, f, c]
                assert np.array_equal(slots[b, f, c, :nb[b, f, c]], row) and not slots[b, f, c, nb[b, f, c]:rb].any()
                if f + 1 < tcl.F12:
                    copy = slots[b, f + 1, c, rb:]
                    assert np.array_equal(copy[:nb[b, f, c]], row) and not copy[nb[b, f, c]:].any(), (b, f, c)
    assert not slots[:, 0, :, rb:].any()
    lost = _designed_lost(C)
    rec = np_recover_plan(lost["every second"], 8)[2]
    assert rec.sum() == lost["every second"].sum() == B0 * 6 * C
    w = np_widths(codes, sf, off)
    assert (bits[rec] == LONGEST if layout != fl.EMPTY else bits[rec] == bits.max()).any() and (bits[rec] == 5 * M0).any()
    assert rec[2, 4].all() and (w[2, 4, M0 - 1] == 31).all() and rec[1, 0, 0]
    if layout == fl.EMPTY:
        assert w[1, 0, j - 1:j + 2, 0].tolist() == [16, 0, 1]
    src, age, rec = np_recover_plan(lost["and a run of three"], 8)
    assert rec[1, 6].all() and not rec[1, 4:6].any() and (src[1, 4:6] == 3).all() and age[1, 4:6, 0].tolist() == [1, 2]
    assert (bits[1, 3] == bits.max()).all()
    return off, ref, lost


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_designed_rows_are_their_own_copies(layout, C):
    _designed_slots(layout, C)


# ---- 4. CPU: the copy at the end of data ------------------------------------------------------------------------------------
WORDS = (43, 512, 538)
PLACEMENTS = (("middle", 0), ("last", 0), ("last", 4), ("last", 3))
PLACEMENT_IDS = ["middle", "last", "last-4", "last-3"]
FILL = 700                                                       # bits of the rows between the copies' rows


def _copy_bits(W):
    return (LONGEST,) if W == 538 else (32 * W, 32 * W - 1, 32 * (W - 1), 32 * (W - 2) + 1, 32 * (W - 2), 32 * (W - 3))


@functools.lru_cache(maxsize=None)
def _end_rows(W, C):
    """One clip of 2 n + 2 frames: frame 2 i + 1, i < n, is a row of _copy_bits(W)[i] bits -- boundary_inputs.constant_row, at
    W = 538 test_conceal_layouts._full_rows' every-band-at-16-bits row with _tail_codes -- and every other frame a 700-bit row;
    the slot of frame 2 i + 2 carries the copy.  Protected by numpy at R = 1365, R2 = 32 W: every copy is its input row's
    bytes, at offset 0."""
    off = fl.host_offsets(48000)
    lengths = _copy_bits(W)
    F = 2 * len(lengths) + 2
    codes, sf = np.zeros((1, F, N0, C), np.int16), np.zeros((1, F, M0, C), np.int8)
    filler = bi.constant_row(off, FILL)
    codes[0, :], sf[0, :] = filler[0][None, :, None], filler[1][None, :, None]
    for i, n in enumerate(lengths):
        for c in range(C):
            if W == 538:
                _, fc, fs, _, _, _, _ = tcl._full_rows("48000", C)
                # (-32768, which requantising returns as -32767, is written as -32767 here: still 16 bits, and the copy is the row)
                codes[0, 2 * i + 1, :, c], sf[0, 2 * i + 1, :, c] = np.maximum(fc[0, 1, :, c], -32767), fs[0, 1, :, c]
            else:
                codes[0, 2 * i + 1, :, c], sf[0, 2 * i + 1, :, c] = bi.constant_row(off, n)
            codes[0, 2 * i + 2, :, c], sf[0, 2 * i + 2, :, c] = filler
    bits = np_row_bits(codes, sf, off)
    assert bits[0, 1:F - 1:2, 0].tolist() == list(lengths) and (bits[0, 0::2] == FILL).all() and (bits[0, F - 1] == FILL).all()
    data, index = np_pack(codes, sf, off)
    R2 = 32 * W
    ref = np_protect(data, index, off, N0, R1, R2)
    sb = RB1 + 4 * W
    slots = ref[0].reshape(F, C, sb)
    for i, n in enumerate(lengths):
        for c in range(C):
            nb = (n + 31) // 32 * 4
            copy = slots[2 * i + 2, c, RB1:]
            assert ref[3][0, 2 * i + 2, c] and ref[5][0, 2 * i + 2, c] == 0
            assert np.array_equal(copy[:nb], data[index[0, 2 * i + 1, c]:index[0, 2 * i + 1, c] + nb]) and not copy[nb:].any()
            if n == R2:                                          # a full copy: its last word holds the last two bins' fields
                assert copy[-4:].view("<u4")[0] != 0
    return off, codes, sf, data, index, ref


def _end_case(W, C, i, where, trim):
    """The slots of _end_rows(W, C) with the slot that carries copy i of channel C - 1 placed in the middle of ``data`` or last,
    the index following, and ``data`` trimmed: (bytes, index, lost, plain) -- plain: the load path parse_strip_p's rule gives
    the copy; asserted against the table of the module docstring."""
    off, codes, sf, _, _, ref = _end_rows(W, C)
    F = codes.shape[1]
    sb = RB1 + 4 * W
    slots = ref[0].reshape(F * C, sb)
    t = (2 * i + 2) * C + (C - 1)
    others = [r for r in range(F * C) if r != t]
    order = others[:1] + [t] + others[1:] if where == "middle" else others + [t]
    index = np.empty(F * C, dtype=np.int64)
    index[order] = np.arange(F * C) * sb
    whole = slots[order].reshape(-1)
    n = len(whole) - trim
    lost = _lost(F, range(1, F - 1, 2), 1, C)                     # the rows before the carrying slots: every one recovered
    assert np_recover_plan(lost, 8)[2].sum() == lost.sum()
    assert (np_conceal_plan(lost, 8)[1][lost != 0] == 1).all()   # (concealment alone would read the row before, faded once)
    a = int(index[t]) + RB1
    nbits = _copy_bits(W)[i]
    nw = (nbits + 31) // 32
    plain = a % 4 == 0 and a + 4 * (nw + 2) <= n
    if where == "middle":
        assert trim == 0 and plain
    else:
        assert a + 4 * W == len(whole)                           # the redundant part ends where data ends
        assert plain == (nbits <= 32 * (W - 2 - (1 if trim else 0))), (W, nbits, trim)
    return whole[:n], index.reshape(1, F, C), lost, plain


def _end_reference(W, C, i, where, trim):
    """The rows numpy plans for _end_case, and the conditions on them alone: a recovered row is its input row; a full copy's
    last word holds the fields of the last two bins of its last stored band -- non-zero untrimmed, 0 with 4 bytes trimmed, the
    low byte's field with 3 bytes trimmed; a copy that is a word or more shorter than the redundant part loses nothing."""
    off, codes, sf, _, _, _ = _end_rows(W, C)
    data, index, lost, plain = _end_case(W, C, i, where, trim)
    src, age = np_recover_src_index(index, lost, len(data), 8, RB1)
    assert not age.any()
    uc, us = np_unpack(data, src, off, N0)
    cc, cs = np_canon(codes, sf, off)
    c, nbits = C - 1, _copy_bits(W)[i]
    for f in range(codes.shape[1]):
        for ch in range(C):
            if (f, ch) != (2 * i + 1, c):
                assert np.array_equal(uc[0, f, :, ch], cc[0, f, :, ch]) and np.array_equal(us[0, f, :, ch], cs[0, f, :, ch])
    got, want = uc[0, 2 * i + 1, :, c], cc[0, 2 * i + 1, :, c].copy()
    assert np.array_equal(us[0, 2 * i + 1, :, c], cs[0, 2 * i + 1, :, c])
    if nbits == 32 * W:
        w = np_widths(cc[:, 2 * i + 1:2 * i + 2, :, c:c + 1], cs[:, 2 * i + 1:2 * i + 2, :, c:c + 1], off)[0, 0, :, 0]
        pos, wb, keep = np_code_fields(w[None], off)
        last = int(np.flatnonzero(keep[0])[-1])
        assert wb[0, last] == 16 and wb[0, last - 1] == 16 and pos[0, last] + 16 == nbits and pos[0, last - 1] + 32 == nbits
        assert want[last - 1] != 0 and want[last] != 0
        if W == 538:
            assert last == N0 - 1 and want[N0 - 2:].tolist() == list(tcl._tail_codes(c))
        if where == "last" and trim == 4:
            want[last - 1:last + 1] = 0
        if where == "last" and trim == 3:
            want[last - 1:last + 1] = int(unzz(int(zz(want[last - 1])) & 0xFF)), 0
            assert want[last - 1] != 0
    elif nbits == 32 * W - 1 and trim:
        assert not np.array_equal(got, want) and np.array_equal(got[:off[1]], want[:off[1]])
        want = got
    assert np.array_equal(got, want), (W, C, nbits, where, trim)
    return uc, us, plain


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("W", WORDS)
def test_the_last_copy_reaches_the_reference_to_its_last_word(W, C):
    paths = {}
    for (where, trim), name in zip(PLACEMENTS, PLACEMENT_IDS):
        paths[name] = ["plain" if _end_reference(W, C, i, where, trim)[2] else "guarded" for i in range(len(_copy_bits(W)))]
    print("W=%d C=%d, copies of %s bits: %s" % (W, C, list(_copy_bits(W)), paths))
    if W != 538:
        assert paths == {"middle": ["plain"] * 6, "last": ["guarded"] * 4 + ["plain"] * 2, "last-4": ["guarded"] * 5 + ["plain"],
                         "last-3": ["guarded"] * 5 + ["plain"]}
    else:
        assert paths == {"middle": ["plain"], "last": ["guarded"], "last-4": ["guarded"], "last-3": ["guarded"]}


# ---- GPU --------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_slots_of_test_protect_hold_empty_copies():
    """Part 1 on the actual bytes: protect_layouts.slots_noise is ``_slots``' input, and no copy in ``_slots(2, 7)`` stores more
    than one band."""
    from test_encode_quantized_fused import _pcm
    want = _pcm(N0, 2, 3, 6, seed=37, inject=False)
    assert torch.equal(want.cpu(), torch.from_numpy(pl.slots_noise(2, 7)))
    codec, data, index = _slots(2, 7)
    _, _, w = pl.copies(data.cpu().numpy(), index.cpu().numpy(), codec.row_bytes, codec.psy.scale_band_offsets)
    assert int(pl.stored_bands(w).max()) <= 1 and not (w == 31).any()


def _recover_everything(dst, off, slots, idx, C, what, oracle):
    """_hold over test_protect's patterns at max_age 1 and 8 and both formats on numpy-made or numpy-checked slots; the plain
    decode on a substituted index where every lost row is recovered; with ``oracle`` the float32 PCM against the float64 oracle's
    synthesis of the numpy-planned, numpy-faded rows (a recovered row: np_unpack at index[b, f+1, c] + o, unfaded)."""
    data, index = _dev(slots), _dev(idx)
    o, worst, recovered = dst.row_bytes, 0.0, 0
    for max_age in pl.AGES:
        for name, lost in _pats(C, idx.shape[1])(max_age).items():
            out = _hold(dst, data, index, lost, max_age, o, "%s %s" % (what, name))
            rec = np_recover_plan(lost, max_age)[2]
            recovered += int(rec.sum())
            if rec.sum() == (lost != 0).sum():
                assert same_bits(out, dst.decode_packed(data, _substituted(index, _dev(lost), o))), (what, name, max_age)
            if oracle:
                src, age = np_recover_src_index(idx, lost, len(slots), max_age, o)
                codes, sf = np_unpack(slots, src, off, N0)
                assert not (sf == -128).any(), (what, name)                 # no width-31 band: no block is left out
                worst = max(worst, tfl._hold_codes_to_the_oracle(codes, np_fade(sf, age), off, out, (what, name, max_age)))
    assert recovered > 0
    return worst


@gpu
@pytest.mark.parametrize("layout,signal,C", tcl.CASES)
def test_protect_and_recover_encoded_signals(layout, signal, C, monkeypatch):
    """Part 2: the dense pack and the rows at 2730 bits, protected at R = 1365 with R2 = 1365 and 2730, then recovered."""
    monkeypatch.delenv(NOFUSE, raising=False)
    r = tfl._ref(layout, signal, C, None, False)
    dst = r.base.with_row_budget(R1)
    assert dst.row_bytes == RB1
    inputs = {"dense": r.base.psy.pack(r.codes, r.sf), "2730": r.base.with_row_budget(2730).encode_packed_rows(r.x)[:2]}
    for kind, (data, index) in inputs.items():
        assert tuple(index.shape) == (B0, F0, C)
        for R2 in REDS:
            what = (layout, signal, C, kind, R2)
            ref = _protect3(dst, data.cpu().numpy(), index.cpu().numpy(), R2, r.off)
            if R2 > R1 and kind == "2730":                         # the redundant part is longer than the primary one and holds more
                assert int((ref[5] < ref[4]).sum()) >= 1, what
            if signal == "tonal":                                  # numpy's reading of the bytes, before any decode
                pl.hold_conditions(ref[0], ref[1], RB1, r.off, _pats(C), what, red_offset=ref[5] if R2 == R1 else None)
            worst = _recover_everything(dst, r.off, ref[0], ref[1], C, what, signal == "tonal")
            if signal == "tonal":
                print("%s: recovered float32 PCM within %.3f of its bar against the oracle" % (what, worst))


@gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_designed_rows_as_copies(layout, C, monkeypatch):
    """Part 3: numpy-made slots at R = R2 = 17216, decoded by the base codec with redundant_at = row_bytes(R)."""
    monkeypatch.delenv(NOFUSE, raising=False)
    off, ref, patterns = _designed_slots(layout, C)
    sr, alpha, _ = tcl._offsets(layout)
    codec = audiocodec_amd.AudioCodec(sr, N0, alpha=alpha)
    np.testing.assert_array_equal(codec.psy.scale_band_offsets, off)
    data, index, o = _dev(ref[0]), _dev(ref[1]), row_bytes(LONGEST)
    for name, lost in patterns.items():
        out = _hold(codec, data, index, lost, 8, o, "%s C=%d designed, %s" % (layout, C, name))
        # NaN exactly in the blocks under a row that numpy reads with a width-31 band that holds bins
        src, _ = np_recover_src_index(ref[1], lost, len(ref[0]), 8, o)
        bad = (np_unpack(ref[0], src, off, N0)[1][:, :, np.diff(off) > 0] == -128).any(axis=2)
        nan_block = np.zeros((B0, tcl.F12 + 1, C), dtype=bool)
        nan_block[:, :-1] |= bad
        nan_block[:, 1:] |= bad
        blocks = out.view(B0, tcl.F12 + 1, N0, C)
        assert np.array_equal(torch.isnan(blocks).any(dim=2).cpu().numpy(), nan_block) and nan_block.any() and not nan_block.all()
        assert bool(torch.isnan(blocks[2, 4:6]).all())            # the recovered row with the width-31 band
        if name == "every second":
            assert same_bits(out, codec.decode_packed(data, _substituted(index, _dev(lost), o)))
            assert not same_bits(out, codec.decode_packed(data, index, lost=_dev(lost), max_age=8))


@gpu
@pytest.mark.parametrize("placement", PLACEMENTS, ids=PLACEMENT_IDS)
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("W", WORDS)
def test_the_copy_at_the_end_of_data(W, C, placement, monkeypatch):
    """Part 4.  The load path of the target copy per case is _end_case's ``plain`` (printed): in the middle plain dword loads;
    last, plain loads for copies of at most 32 (W - 2) bits, guarded loads above; trimmed by 4 or 3 bytes, plain loads for 32
    (W - 3) bits alone.  The bytes behind ``nbytes`` are 0xFF: a load past the end shows."""
    monkeypatch.delenv(NOFUSE, raising=False)
    where, trim = placement
    off, codes, sf, data, index, ref = _end_rows(W, C)
    base = audiocodec_amd.AudioCodec(48000, N0)
    dst = base.with_row_budget(R1)
    R2 = 32 * W
    if placement == PLACEMENTS[0]:                               # the slots themselves, once per (W, C)
        if R2 <= CAP:
            _protect3(dst, data, index, R2, off)
        else:                                                    # served by the composition: its bytes against numpy's
            assert dst.protect_packed_rows_launches(C, red_bits=R2) != 1
            for name, g, want in zip(NAMES, dst.protect_packed_rows(_dev(data), _dev(index), R2, True), ref):
                np.testing.assert_array_equal(g.cpu().numpy(), want, err_msg=name)
    for i in range(len(_copy_bits(W))):
        _end_reference(W, C, i, where, trim)                     # the conditions on the reference, before any kernel result
        bytes_, idx, lost, plain = _end_case(W, C, i, where, trim)
        n = len(bytes_)
        big = torch.full((n + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
        big[:n] = _dev(bytes_)
        what = "W=%d C=%d copy of %d bits, %s, %d trimmed: %s loads" % (W, C, _copy_bits(W)[i], where, trim, "plain" if plain else "guarded")
        print(what)
        out = _hold(dst, big[:n], _dev(idx), lost, 8, RB1, what)
        assert same_bits(out, dst.decode_packed(big[:n], _substituted(_dev(idx), _dev(lost), RB1))), what


@gpu
@pytest.mark.parametrize("R", [R1, CAP, 320])
def test_protect_at_the_cap(R):
    """Part 5: R2 = AC_PACK_ROWS_MAX_BITS, where the redundant pack fills all of the staged slot."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    dst = base.with_row_budget(R)
    off = base.psy.scale_band_offsets
    assert dst.protect_packed_rows_launches(2, red_bits=CAP) == 1
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(torch.from_numpy(fl.tonal(2)).cuda())
    ref = _protect3(dst, data.cpu().numpy(), index.cpu().numpy(), CAP)
    assert ref[3].all() and not ref[5].any()                      # every 2730-bit row fits the cap as it is
    np.testing.assert_array_equal(ref[0].reshape(B0, F0, 2, -1)[:, 1:, :, row_bytes(R):row_bytes(R) + row_bytes(2730)].reshape(-1),
                                  data.cpu().numpy().reshape(B0, F0, 2, -1)[:, :-1].reshape(-1))
    _, _, adv, adv_index, _ = _adversarial()
    ref = _protect3(dst, adv, adv_index, CAP)
    assert not ref[3][0, 2, 0] and int(ref[5][0, 2, 0]) == 254   # the saturating row's copy
    # test_protect_redundant_slot_slack at 16383: the copy of R2 + 1 bits ends on the staged slot's last bit, at word 511
    codes, sf, lengths = bi.slot_rows(off, CAP - 1)
    assert lengths[1] == CAP == 32 * 512
    codes, sf = np.concatenate([codes, codes[:, :1]], axis=1), np.concatenate([sf, sf[:, :1]], axis=1)
    data, index = np_pack(codes, sf, off)
    ref = _protect3(dst, data, index, CAP - 1)
    assert ref[3].ravel().tolist() == [True, True, True, False, True] and ref[5].ravel().tolist() == [0, 0, 254, 254, 0]
    sb = row_bytes(R) + row_bytes(CAP - 1)
    assert ref[0].reshape(5, sb)[2, -4:].view("<u4")[0] != 0
