"""The concealing decoders on other band layouts, on wide rows and on full-length rows: k_inv_fast_pl (``decode_packed(...,
lost=, max_age=)``) and k_inv_fast_pls (``decode_packed_chunk(..., lost=, max_age=)``, the carried row).  test_conceal.py and
test_stream_conceal.py run both families at 48000 Hz on rows of at most 346 words; here they run on the layouts of
fused_layouts.py (8000, 44100, 96000, EMPTY) and at 48000 Hz, mono and stereo, B = 3, on

  1. encoded signals -- ``noise`` (-128 bands, marked rows) and ``tonal`` (10- and 11-bit fields) -- as the dense pack of the
     unbudgeted codes and as the fixed-stride rows of a binding budget, twelve frames made of six through ``index`` (FRAMES: a
     source may lie before or after its reader in memory);
  2. designed rows: every width 0..16 and 31, the extreme codes, the shortest and the longest rows, at EMPTY the 16/0/1 row;
  3. the full-length row (538 words, every band at 16 bits) as the carried row of a stream: in the middle of ``data``, ending
     exactly at ``nbytes``, and with ``data`` trimmed by 4 and by 3 bytes -- the boundary of carry_state_p's plain copy at
     equality, one word short and off the word grid -- kept through a chunk in which nothing arrives;
  4. a chain: chunks encoded at 128 kbit/s, transrated to 64 kbit/s chunk by chunk, decoded with concealment.

Every GPU comparison between the kernel (one launch), the composition (``AC_DECODE_PACKED_NOFUSE=1``; three launches per chunk)
and ``decode_quantized`` of the numpy-concealed rows is bit for bit, float32 and 16-bit PCM.  The numpy side starts from the
bytes (``np_unpack``; ``psy.unpack`` must give the same arrays).  For ``tonal``'s dense rows the float32 PCM is also held to
the float64 oracle's synthesis of the numpy-concealed, numpy-dequantised rows at the bar of
test_fused_layouts._hold_codes_to_the_oracle, LSB * max(1, peak of the reference block); no band there has width 31, so no
block is left out.  Before a kernel result is looked at, the numpy plans must show what keeps a comparison from being vacuous
(_wide_sources, _read_at, the positions and the last word of part 3); the tests not marked ``gpu`` hold the same conditions
on the numpy oracle's codes and on the designed bytes.

Part 4's condition on the reference is that some row was requantised and fits (test_transrate._binding's first assertion).
All of _binding -- also a row left at offset 0, and neighbours at different offsets -- holds at 44100 and 48000 Hz and is
asserted there; at 96000 Hz and EMPTY 64 kbit/s (682 and 546 bits a row) leaves no row of ``tonal`` as it is.  At 8000 Hz
64 kbit/s is 8192 bits a row and ``tonal``'s longest row has 4551, so no row can be requantised at these bitrates: the test
asserts that fact (every offset 0, every row fits) and holds the same comparisons.

That the file bites (scratch builds of the library, each with one change that stays inside every buffer; this file and
test_stream_conceal.py run once against each on the MI355X):
  * copy_carried_row stores one word fewer (``< P_CARRY_WORDS - 1`` in the store guard only): the 32 cases of
    test_the_full_length_row_is_carried_to_its_last_word fail (every layout, C and placement) and the 10 of
    test_designed_rows_as_sources (their longest rows are carried too); nothing else, and test_stream_conceal.py passes.
  * the clamped branch of carry_state_p stops at ``P_CARRY_WORDS - 1``: the 8 cases "last, 3 bytes trimmed" of
    test_the_full_length_row_is_carried_to_its_last_word fail -- the one placement at which that branch has a non-zero last
    word to store ("last" takes the plain copy, and 4 bytes trimmed leave a word that reads as 0); nothing else, and
    test_stream_conceal.py passes.
No kernel was found wrong: every comparison of this file holds on the library as it is.
"""

import functools

import numpy as np
import pytest
import torch

import audiocodec_amd

import fused_layouts as fl
import test_fused_layouts as tfl
from conceal_reference import np_conceal, np_conceal_plan
from pack_reference import np_canon, np_code_fields, np_pack, np_row_bits, np_unpack, np_widths
from stream_conceal_reference import np_conceal_chunk, np_fresh_state, np_stream_plan
from stream_order import same_bits
from test_conceal import _patterns as _one_shot_patterns
from test_pack import designed
from test_stream_conceal import NOFUSE, _bounds, _chunks, _composed, _numpy_chunks, _patterns, _pcm_store
from test_transrate import _binding
from transrate_reference import np_transrate

gpu = pytest.mark.gpu
N0, M0, B0 = fl.N0, fl.M0, fl.B0
LAYOUTS = [l for l in fl.LAYOUTS if l[0] in ("8000", "44100", "96000", fl.EMPTY)] + [tfl.BY_ID["48000"]]
LAYOUT_IDS = [l[0] for l in LAYOUTS]
BY_ID = {l[0]: l for l in LAYOUTS}
FRAMES = (0, 1, 2, 3, 4, 5, 2, 4, 1, 5, 3, 0)                    # the twelve frames, of the six of a signal
F12 = len(FRAMES)
SPLITS = ((12,), (1,) * 12, (5, 7), (2, 3, 7))
SPLIT_IDS = ["12", "1x12", "5-7", "2-3-7"]
AGES = (1, 8)
KINDS = ("dense", "budget")
CARRY_WORDS = 538                                                # P_CARRY_WORDS: (5 * 64 + 8 * 64 + 16 * 1024) / 32
CASES = [(layout, signal, C) for layout in LAYOUT_IDS for signal in ("noise", "tonal") for C in (1, 2)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _offsets(layout):
    sr, alpha = fl.resolve(BY_ID[layout])
    return sr, alpha, fl.host_offsets(sr)


# ---- what the numpy plans must show ------------------------------------------------------------------------------------
def _wide_rows(codes, sf, off):
    """bool [B, F, C]: the row holds a stored width >= 10 and a code field of >= 9 bits across a 32-bit word boundary (rows
    start on word boundaries, so positions count from the row's start)."""
    w = np_widths(codes, sf, off)
    B, F, M, C = w.shape
    wr = np.moveaxis(w, 3, 2).reshape(B * F * C, M)
    pos, wb, keep = np_code_fields(wr, off)
    crossing = (keep & (wb >= 9) & ((pos % 32) + wb > 32)).any(axis=1)
    return (crossing & ((wr >= 10) & (wr <= 16)).any(axis=1)).reshape(B, F, C)


def _wide_sources(wide, lost, max_age, splits):
    """From the numpy plans alone: (reads at age >= 1 of a wide row, those of them the stream of `splits` reads as its carried
    row -- the source lies before the reader's chunk).  The stream's plan must be the one-shot plan."""
    src, age = np_conceal_plan(lost, max_age)
    s_src, s_age, _ = np_stream_plan(lost, splits, (max_age,) * len(splits))
    assert np.array_equal(s_src, src) and np.array_equal(s_age, age), (max_age, splits)
    b, _, c = np.meshgrid(*[np.arange(n) for n in src.shape], indexing="ij")
    hit = (age >= 1) & (src >= 0) & wide[b, np.maximum(src, 0), c]
    start = np.repeat([a for a, _ in _bounds(splits)], splits)   # first frame of every frame's chunk
    return int(hit.sum()), int((hit & (src < start[None, :, None])).sum())


def _assert_wide_sources(codes, sf, off, C, what):
    """Over the patterns of every split: a wide row is read at age >= 1 at each max_age, and the stream of every split of more
    than one chunk reads one as its carried row.  Prints the counts."""
    wide = _wide_rows(codes, sf, off)
    assert wide.any(), what
    for splits in SPLITS:
        carried = 0
        for max_age in AGES:
            got = [_wide_sources(wide, lost, max_age, splits) for lost in _patterns(B0, F12, C, max_age, splits).values()]
            hits = sum(g[0] for g in got)
            carried += sum(g[1] for g in got)
            print("%s max_age=%d splits=%s: %d reads of a wide row at age >= 1, %d as the carried row"
                  % (what, max_age, splits, hits, sum(g[1] for g in got)))
            assert hits >= 1, (what, max_age, splits)
        assert carried >= 1 or len(splits) == 1, (what, splits)


def _read_at(src, age, b, f, ages):
    """Row (b, f) is, in some channel, the source at each of `ages`."""
    return all(bool(((src[b] == f) & (age[b] == a)).any()) for a in ages)


# ---- part 1 on the CPU: tonal's dense rows on the numpy oracle -------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_tonal_rows_are_wide_sources_on_the_numpy_oracle(layout, C):
    sr, alpha, off = _offsets(layout)
    codes, sf = fl.oracle_codes(fl.tonal(C), sr, alpha, off)
    data, index = np_pack(codes, sf, off)
    index12 = index[:, list(FRAMES)]
    c12, s12 = np_unpack(data, index12, off, N0)
    cc, cs = np_canon(codes, sf, off)
    np.testing.assert_array_equal(c12, cc[:, list(FRAMES)])
    np.testing.assert_array_equal(s12, cs[:, list(FRAMES)])
    assert not (np_widths(c12, s12, off) == 31).any()            # every block is compared with the oracle
    fl.assert_wide(c12, s12, off)
    _assert_wide_sources(c12, s12, off, C, (layout, C))


# ---- part 2 on the CPU: the designed rows and the fixed pattern ---------------------------------------------------------------
DESIGNED_SPLITS = ((5, 7), (1,) * 12)
DESIGNED_AGE = 8


@functools.lru_cache(maxsize=None)
def _designed(layout, C):
    """test_pack.designed on the layout's offsets, shaped as test_decode_packed_fused._designed_rows but B = 3, F = 12: the
    shortest rows at frames 2 and 7, the longest at 3 and 8, a width-31 band in row (2, 4), at EMPTY the 16/0/1 row at (1, 0) in
    channel 0.  The pattern (max_age = 8):
      clip 0: frames 4 .. 8 lost -- the longest row (0, 3) at ages 1 .. 5 (age 5: more than four frames back);
      clip 1: frames 1 .. 3 lost -- row (1, 0) at ages 1 .. 3 (EMPTY: the 16/0/1 row); 8 .. 10 lost -- the shortest row (1, 7);
      clip 2: frames 5 .. 7 lost -- the row with the width-31 band, (2, 4), at ages 1 .. 3; 9 .. 11 lost -- the longest row
              (2, 8): in mono the clip of the pair that has no second signal."""
    _, _, off = _offsets(layout)
    L = np.diff(off)
    codes, sf = designed(np.random.default_rng(17 + C), off, B0, F12, C)
    codes[:, 2::5] = 0
    sf[:, 2::5] = 5
    codes[:, 3::5] = -32768
    sf[:, 3::5] = 3
    codes[0, 3, ::2] = 32767
    codes[0, 3, 1::4] = -32767
    sf[2, 4, M0 - 1] = -128
    j = None
    if layout == fl.EMPTY:
        j = int(np.flatnonzero(L == 0)[0])
        codes[1, 0, off[j - 1]:off[j], 0] = -32768
        codes[1, 0, off[j + 1]:off[j + 2], 0] = -1
        sf[1, 0, j - 1:j + 2, 0] = (7, 9, -3)
    lost = np.zeros((B0, F12, C), dtype=np.uint8)
    lost[0, 4:9] = 1
    lost[1, 1:4] = 1
    lost[1, 8:11] = 1
    lost[2, 5:8] = 1
    lost[2, 9:12] = 1
    data, index = np_pack(codes, sf, off)
    return off, codes, sf, data, index, lost, j


def _designed_conditions(layout, C):
    off, codes, sf, data, index, lost, j = _designed(layout, C)
    L = np.diff(off)
    w = np_widths(codes, sf, off)
    assert set(np.unique(w[..., L > 0, :]).tolist()) == set(range(17)) | {31}
    assert (codes == -32768).any() and (codes == 32767).any() and (codes == -32767).any()
    bits = np_row_bits(codes, sf, off)
    longest = 5 * M0 + 8 * int((L > 0).sum()) + 16 * N0
    assert bits.min() == 5 * M0 and bits.max() == longest
    assert (bits[0, 3] == longest).all() and (bits[2, 8] == longest).all() and (bits[1, 7] == 5 * M0).all()
    assert (w[2, 4, M0 - 1] == 31).all()
    if layout == fl.EMPTY:
        assert w[1, 0, j - 1:j + 2, 0].tolist() == [16, 0, 1] and L[j] == 0
    else:
        assert longest == 32 * CARRY_WORDS
    src, age = np_conceal_plan(lost, DESIGNED_AGE)
    assert _read_at(src, age, 0, 3, (1, 2, 3, 4, 5))             # a longest row; at age 5 from another strip
    assert _read_at(src, age, 1, 7, (1, 2, 3))                   # a shortest row
    assert _read_at(src, age, 2, 4, (1, 2, 3))                   # a row with a width-31 band
    assert _read_at(src, age, 1, 0, (1, 2, 3))                   # (EMPTY: the 16/0/1 row)
    assert _read_at(src, age, 2, 8, (1, 2, 3))                   # a longest row where, in mono, the pair is half empty
    assert (src[0, 8] == 3).all() and (age[0, 8] == 5).all()
    for splits in DESIGNED_SPLITS:   # ... as a carried row: the longest row across the boundary at 5, each of them in chunks of one
        s_src, s_age, _ = np_stream_plan(lost, splits, (DESIGNED_AGE,) * len(splits))
        assert np.array_equal(s_src, src) and np.array_equal(s_age, age)
        start = np.repeat([a for a, _ in _bounds(splits)], splits)[None, :, None]
        carried = (age >= 1) & (src < start)
        for b, f in ((0, 3), (1, 7), (2, 4), (1, 0), (2, 8)) if len(splits) == F12 else ((0, 3),):
            assert ((src[b] == f) & carried[b]).any(), (splits, b, f)
    uc, us = np_unpack(data, index, off, N0)
    cc, cs = np_canon(codes, sf, off)
    np.testing.assert_array_equal(uc, cc)
    np.testing.assert_array_equal(us, cs)
    return uc, us


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_designed_rows_are_sources_in_the_plan(layout, C):
    _designed_conditions(layout, C)


# ---- part 3 on the CPU: the full-length row, its positions and its last word ------------------------------------------------
FULL_LAYOUTS = [l for l in LAYOUT_IDS if l != fl.EMPTY]
PLACEMENTS = ("middle", "last", "last, 4 bytes trimmed", "last, 3 bytes trimmed")
FULL_SPLITS = (2, 3, 4)                                          # chunk 1; chunk 2, every row lost; chunk 3, its first two lost
FULL_AGE = 31


def _tail_codes(s):
    """Bins 1022 and 1023 of signal s's full-length row: the two 16-bit fields of the row's last word."""
    return 20000 + 1111 * s, -(9000 + 517 * s)


@functools.lru_cache(maxsize=None)
def _full_rows(layout, C):
    """Nine frames of B = 3 (stereo) or 6 (mono) clips: six signals.  Frame 1 of every signal is a longest row -- every band at 16
    bits, 17216 bits = 538 words -- that differs between the signals; the other rows hold codes in +-300."""
    _, _, off = _offsets(layout)
    B, F = (3 if C == 2 else 6), sum(FULL_SPLITS)
    rng = np.random.default_rng(538 + C)
    codes = rng.integers(-300, 301, (B, F, N0, C)).astype(np.int16)
    sf = rng.integers(-30, 10, (B, F, M0, C)).astype(np.int8)
    codes[:, 1] = rng.integers(-32768, 32768, (B, N0, C)).astype(np.int16)
    codes[:, 1, off[:-1]] = -32768                               # zigzag 65535: every band 16 bits wide
    sf[:, 1] = rng.integers(-40, -20, (B, M0, C)).astype(np.int8)
    for b in range(B):
        for c in range(C):
            codes[b, 1, N0 - 2:, c] = _tail_codes(b * C + c)
    bits = np_row_bits(codes, sf, off)
    assert (np.diff(off) > 0).all() and (bits[:, 1] == 32 * CARRY_WORDS).all() and bits[:, [0] + list(range(2, F))].max() < 32 * 350
    data, index = np_pack(codes, sf, off)
    lost = np.zeros((B, F, C), dtype=np.uint8)
    lost[:, 2:7] = 1
    return off, codes, sf, data, index, (bits + 31) // 32 * 4, lost


def _full_case(layout, C, target, placement):
    """The bytes with signal `target`'s full-length row placed: (data uint8 trimmed to nbytes, index [B, 9, C], lost, the
    untrimmed bytes).  Every other row keeps its bytes, at another start."""
    off, codes, sf, data, index, nb, lost = _full_rows(layout, C)
    B, F, _ = index.shape
    flat, nbf = index.reshape(-1), nb.reshape(-1)
    t = ((target // C) * F + 1) * C + target % C
    others = [r for r in range(flat.size) if r != t]
    order = others[:1] + [t] + others[1:] if placement == "middle" else others + [t]
    new = np.empty_like(flat)
    parts, at = [], 0
    for r in order:
        new[r] = at
        parts.append(data[flat[r]:flat[r] + nbf[r]])
        at += int(nbf[r])
    whole = np.concatenate(parts)
    trim = {"middle": 0, "last": 0, "last, 4 bytes trimmed": 4, "last, 3 bytes trimmed": 3}[placement]
    n = len(whole) - trim
    start = int(new[t])
    assert start % 4 == 0 and nbf[t] == 4 * CARRY_WORDS
    if placement == "middle":
        assert start + 4 * (CARRY_WORDS + 2) <= n                # plain loads in both kernels
    else:
        assert start + 4 * CARRY_WORDS == n + trim               # at equality, one word short, off the word grid
    return whole[:n], new.reshape(index.shape), lost, whole


def _full_reference(layout, C, target, placement):
    """The numpy state machine over the three chunks from the bytes, and the conditions on it alone: the bins the row's last
    word holds are read, non-zero and different in every signal, in every frame concealed from the carried row."""
    off, codes, sf, _, _, _, _ = _full_rows(layout, C)
    data, index, lost, whole = _full_case(layout, C, target, placement)
    B, F, _ = index.shape
    cc, cs = np_canon(codes, sf, off)
    state = np_fresh_state(B, N0, M0, C)
    out = []
    for i, (a, b) in enumerate(_bounds(FULL_SPLITS)):
        uc, us = np_unpack(data if i == 0 else whole, index[:, a:b], off, N0)
        c2, s2, state = np_conceal_chunk(uc, us, lost[:, a:b], state, FULL_AGE)
        out.append((c2, s2))
    c2 = np.concatenate([o[0] for o in out], axis=1)
    one = np_conceal(*np_unpack(data, index, off, N0), lost, FULL_AGE)
    np.testing.assert_array_equal(c2, one[0])                    # (the trimmed tail holds the target's row alone)
    last_band = slice(int(off[M0 - 1]), N0)
    seen = set()
    for b in range(B):
        for c in range(C):
            s = b * C + c
            want = list(_tail_codes(s))
            if s == target and placement == "last, 4 bytes trimmed":
                want = [0, 0]                                    # the word lies at nbytes: it reads as 0
            if s == target and placement == "last, 3 bytes trimmed":
                z = ((want[0] << 1) ^ (want[0] >> 15)) & 0xFF    # one byte of it is left: the low 8 bits of bin 1022's field
                want = [(z >> 1) ^ -(z & 1), 0]
            for f in (2, 3, 4, 5, 6):                            # frames 0 .. 2 of chunk 2, 0 .. 1 of chunk 3
                assert c2[b, f, N0 - 2:, c].tolist() == want, (s, f, placement)
                assert c2[b, f, last_band, c].any() and np.array_equal(c2[b, f, :N0 - 2, c], cc[b, 1, :N0 - 2, c])
            seen.add(tuple(want))
    assert len(seen) == B * C                                    # different in every signal
    return out


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", FULL_LAYOUTS)
def test_the_full_length_row_reaches_the_reference_to_its_last_word(layout, C):
    for target in range(6):
        for placement in PLACEMENTS:
            _full_reference(layout, C, target, placement)


# ---- GPU: inputs and references, computed once ----------------------------------------------------------------------------------
class _Rows:
    """One input: the codec that decodes it, data and index on the device, what np_unpack reads of the bytes (held once to
    psy.unpack) and the layout's offsets."""

    def __init__(self, key, codec, data, index, off):
        self.key, self.codec, self.data, self.index, self.off = key, codec, data, index.contiguous(), off
        self.codes, self.sf = np_unpack(data.cpu().numpy(), self.index.cpu().numpy(), off, N0)
        uc, us = codec.psy.unpack(data, self.index)
        np.testing.assert_array_equal(uc.cpu().numpy(), self.codes, err_msg=str(key))
        np.testing.assert_array_equal(us.cpu().numpy(), self.sf, err_msg=str(key))
        self.C = self.index.shape[2]
        self.oracle, self.worst = False, 0.0                     # hold the float32 PCM to the float64 oracle as well
        self.one = {}


@functools.lru_cache(maxsize=None)
def _encoded(layout, signal, C, kind):
    """The twelve frames of one (layout, signal, C): the dense pack of the unbudgeted codes, or the fixed-stride rows at half the
    median row (budgets[2] of test_fused_layouts._ref: it binds, and ``noise`` has a marked row there)."""
    r = tfl._ref(layout, signal, C, None, False)
    if kind == "dense":
        codec = r.base
        data, index = codec.psy.pack(r.codes, r.sf)
    else:
        R, kmin = r.budgets[2]
        assert (R, kmin) == (r.Rs // 2, 0)
        codec = r.base.with_row_budget(R, kmin)
        data, index, fits = codec.encode_packed_rows(r.x)
        ref = r.budget(R, kmin)["np_rows"]                       # (the budget's preconditions run here)
        np.testing.assert_array_equal(data.cpu().numpy(), ref[0])
        if signal == "noise":
            assert not bool(fits.all()) and not ref[2].all()
    rows = _Rows((layout, signal, C, kind), codec, data, index[:, list(FRAMES)], r.off)
    if signal == "noise":
        assert (rows.sf == -128).any()
    if signal == "tonal" and kind == "dense":
        assert not (np_widths(rows.codes, rows.sf, r.off) == 31).any()
        fl.assert_wide(rows.codes, rows.sf, r.off)
        _assert_wide_sources(rows.codes, rows.sf, r.off, C, rows.key)
        rows.oracle = True
    return rows


def _one_shot(rows, lost, max_age, pcm16):
    """Blocks [0, F) of the kernel's ``decode_packed(lost=)`` on the whole input, held once to the composition and to
    decode_quantized of the numpy-concealed rows; on ``tonal``'s dense rows the float32 PCM also to the float64 oracle."""
    k = (max_age, pcm16, lost.tobytes())
    if k not in rows.one:
        codec, C = rows.codec, rows.C
        assert codec.decode_packed_launches(C) == 1
        lost_d = _dev(lost)
        fused = codec.decode_packed(rows.data, rows.index, pcm16, lost=lost_d, max_age=max_age)
        with _composed():
            assert codec.decode_packed_launches(C) == 1 + codec.decode_quantized_launches(C)
            comp = codec.decode_packed(rows.data, rows.index, pcm16, lost=lost_d, max_age=max_age)
        c2, s2 = np_conceal(rows.codes, rows.sf, lost, max_age)
        ref = codec.decode_quantized(_dev(c2), _dev(s2), pcm16=pcm16)
        assert fused.dtype == (torch.int16 if pcm16 else torch.float32)
        assert same_bits(comp, ref), "composition != numpy: %s max_age=%d pcm16=%s" % (rows.key, max_age, pcm16)
        assert same_bits(fused, comp), "kernel != composition: %s max_age=%d pcm16=%s" % (rows.key, max_age, pcm16)
        if rows.oracle and not pcm16:
            assert not (s2 == -128).any()
            worst = tfl._hold_codes_to_the_oracle(c2, s2, rows.off, fused, rows.key + (max_age,))
            rows.worst = max(rows.worst, worst)
        rows.one[k] = fused[:, :rows.index.shape[1] * N0].contiguous()
    return rows.one[k]


def _hold_chunks(rows, lost, max_age, splits, fused, comp, what):
    """The chunks of `splits` on the stream objects `fused` (the kernel) and `comp` (the composition) against the one-shot
    blocks, both PCM formats."""
    lost_d = _dev(lost)
    for pcm16 in (False, True):
        ref = _one_shot(rows, lost, max_age, pcm16)
        fused.reset()
        got = torch.cat(_chunks(fused, rows.data, rows.index, lost_d, splits, max_age, pcm16), dim=1)
        assert same_bits(got, ref), "kernel != one-shot: %s %s max_age=%d pcm16=%s" % (rows.key, what, max_age, pcm16)
        comp.reset()
        with _composed():
            assert comp.packed_chunk_launches(decode=True, conceal=True) == 3
            other = torch.cat(_chunks(comp, rows.data, rows.index, lost_d, splits, max_age, pcm16), dim=1)
        assert same_bits(other, ref), "composition != one-shot: %s %s max_age=%d pcm16=%s" % (rows.key, what, max_age, pcm16)


def _streams(rows):
    B, C = rows.index.shape[0], rows.C
    fused, comp = rows.codec.stream(B, C), rows.codec.stream(B, C)
    assert fused.packed_chunk_launches(decode=True, conceal=True) == 1
    return fused, comp


# ---- 1. encoded signals as sources ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout,signal,C", CASES)
def test_encoded_signals_one_shot(layout, signal, C, kind, monkeypatch):
    """k_inv_fast_pl: test_conceal's patterns and those of every split of test_stream_conceal, max_age 1 and 8."""
    monkeypatch.delenv(NOFUSE, raising=False)
    rows = _encoded(layout, signal, C, kind)
    for max_age in AGES:
        named = [_one_shot_patterns(B0, F12, C, max_age)] + [_patterns(B0, F12, C, max_age, s) for s in SPLITS]
        for patterns in named:
            for lost in patterns.values():
                for pcm16 in (False, True):
                    _one_shot(rows, lost, max_age, pcm16)
    if rows.oracle:
        print("%s: concealed float32 PCM within %.3f of its bar against the oracle" % (rows.key, rows.worst))


@gpu
@pytest.mark.parametrize("splits", SPLITS, ids=SPLIT_IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout,signal,C", CASES)
def test_encoded_signals_in_chunks(layout, signal, C, kind, splits, monkeypatch):
    """k_inv_fast_pls: the chunks of a split against the one-shot blocks, and the composed stream against them."""
    monkeypatch.delenv(NOFUSE, raising=False)
    rows = _encoded(layout, signal, C, kind)
    fused, comp = _streams(rows)
    for max_age in AGES:
        for name, lost in _patterns(B0, F12, C, max_age, splits).items():
            _hold_chunks(rows, lost, max_age, splits, fused, comp, name)


# ---- 2. designed rows as sources ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_designed_rows_as_sources(layout, C, monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    uc, us = _designed_conditions(layout, C)                     # the plan, before any kernel result
    off, _, _, data, index, lost, _ = _designed(layout, C)
    sr, alpha, _ = _offsets(layout)
    codec = audiocodec_amd.AudioCodec(sr, N0, alpha=alpha)
    np.testing.assert_array_equal(codec.psy.scale_band_offsets, off)
    rows = _Rows((layout, "designed", C), codec, _dev(data), _dev(index), off)
    np.testing.assert_array_equal(rows.codes, uc)
    np.testing.assert_array_equal(rows.sf, us)
    out = _one_shot(rows, lost, DESIGNED_AGE, False)
    _one_shot(rows, lost, DESIGNED_AGE, True)
    blocks = out.view(B0, F12, N0, C)
    assert bool(torch.isnan(blocks[2, 4:9]).all()) and bool(torch.isfinite(blocks[1, 8:11]).all())   # width 31 / the shortest row
    fused, comp = _streams(rows)
    for splits in DESIGNED_SPLITS:
        _hold_chunks(rows, lost, DESIGNED_AGE, splits, fused, comp, "designed")


# ---- 3. the full-length row in the stream's state ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", FULL_LAYOUTS)
def test_the_full_length_row_is_carried_to_its_last_word(layout, C, placement, monkeypatch):
    """Chunk 1 ends with the 538-word row; chunk 2 (another data tensor) loses every row, so the state-to-state copy keeps it;
    chunk 3 starts with two lost rows.  The kernel, the composition and the numpy state machine, and the one-shot kernel on
    the same bytes with one index of nine frames."""
    monkeypatch.delenv(NOFUSE, raising=False)
    sr, alpha, off = _offsets(layout)
    codec = audiocodec_amd.AudioCodec(sr, N0, alpha=alpha)
    np.testing.assert_array_equal(codec.psy.scale_band_offsets, off)
    B = 3 if C == 2 else 6
    bounds = _bounds(FULL_SPLITS)
    for target in range(6):
        want = _full_reference(layout, C, target, placement)     # the conditions on the reference, before any kernel result
        data, index, lost, whole = _full_case(layout, C, target, placement)
        n = len(data)
        big = torch.full((n + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
        big[:n] = _dev(data)
        first, other = big[:n], _dev(whole)
        index_d, lost_d = _dev(index), _dev(lost)
        uc, us = (t.cpu().numpy() for t in codec.psy.unpack(first, index_d))
        nc, ns = np_unpack(data, index, off, N0)
        np.testing.assert_array_equal(uc, nc)
        np.testing.assert_array_equal(us, ns)
        what = "%s C=%d signal %d %s" % (layout, C, target, placement)
        for pcm16 in (False, True):
            fused, comp, plain = codec.stream(B, C), codec.stream(B, C), codec.stream(B, C)
            assert fused.packed_chunk_launches(decode=True, conceal=True) == 1
            calls = [(first if i == 0 else other, index_d[:, a:b].contiguous(), lost[:, a:b], FULL_AGE, pcm16)
                     for i, (a, b) in enumerate(bounds)]
            got = [fused.decode_packed_chunk(d, i, p, lost=_dev(l), max_age=m) for d, i, l, m, p in calls]
            with _composed():
                assert comp.packed_chunk_launches(decode=True, conceal=True) == 3
                composed = [comp.decode_packed_chunk(d, i, p, lost=_dev(l), max_age=m) for d, i, l, m, p in calls]
            ref, _ = _numpy_chunks(codec, plain, calls)
            plain.reset()                                        # ... and the rows _full_reference made of the bytes alone
            mine = [plain.inverse_chunk(codec.psy.dequantize(_dev(c2), _dev(s2))) for c2, s2 in want]
            for i in range(3):
                assert same_bits(ref[i], _pcm_store(mine[i]) if pcm16 else mine[i]), "numpy, psy.unpack != np_unpack: %s" % what
                assert same_bits(composed[i], ref[i]), "composition != numpy: %s chunk %d pcm16=%s" % (what, i + 1, pcm16)
                assert same_bits(got[i], ref[i]), "kernel != numpy: %s chunk %d pcm16=%s" % (what, i + 1, pcm16)
            # the one-shot kernel on the same bytes: its own plain / clamped decision for the same source row
            one = codec.decode_packed(first, index_d, pcm16, lost=lost_d, max_age=FULL_AGE)
            with _composed():
                comp1 = codec.decode_packed(first, index_d, pcm16, lost=lost_d, max_age=FULL_AGE)
            c2, s2 = np_conceal(nc, ns, lost, FULL_AGE)
            ref1 = codec.decode_quantized(_dev(c2), _dev(s2), pcm16=pcm16)
            assert same_bits(comp1, ref1), "one-shot composition != numpy: %s pcm16=%s" % (what, pcm16)
            assert same_bits(one, comp1), "one-shot kernel != composition: %s pcm16=%s" % (what, pcm16)
            assert same_bits(torch.cat(got, dim=1), one[:, :sum(FULL_SPLITS) * N0]), "chunks != one-shot: %s" % what


# ---- 4. a chain through a transrate ------------------------------------------------------------------------------------------------
CHAIN_SPLITS = (2, 1, 2, 1)                                      # blocks per chunk; the last one is the flushing zero block
CHAIN_KEEPS_A_ROW = ("44100", "48000")                           # 64 kbit/s leaves a row of tonal as it is: all of _binding holds


@gpu
@pytest.mark.parametrize("layout", LAYOUT_IDS)
def test_a_chain_through_a_transrate(layout, monkeypatch):
    """encode_packed_rows_chunk at 128 kbit/s, transrate_packed_rows at 64 kbit/s chunk by chunk, decode_packed_chunk with the
    "30 %" pattern at max_age = 8: against encode_packed_rows, transrate_packed_rows and decode_packed(lost=) on the whole signal,
    and against numpy from the transrated bytes."""
    monkeypatch.delenv(NOFUSE, raising=False)
    C = 2
    sr, alpha, off = _offsets(layout)
    base = audiocodec_amd.AudioCodec(sr, N0, alpha=alpha)
    hi, cbr = base.with_bitrate(128000), base.with_bitrate(64000)
    x = torch.from_numpy(fl.tonal(C)).cuda()
    xz = torch.cat((x, torch.zeros_like(x[:, :N0])), dim=1)
    F = fl.K0 + 1
    assert sum(CHAIN_SPLITS) == F
    lost = _patterns(B0, F, C, 8, CHAIN_SPLITS)["30 %"]
    assert lost.any() and not lost.all()
    # the one-shot route, and the condition on the reference: the transrate requantises
    d128, i128, _ = hi.encode_packed_rows(x)
    ref = np_transrate(d128.cpu().numpy(), i128.cpu().numpy(), off, N0, cbr.row_bits)
    longest = int(np_row_bits(*np_unpack(d128.cpu().numpy(), i128.cpu().numpy(), off, N0), off).max())
    print("%s: %d -> %d bits, offsets %s, rows of up to %d bits" % (layout, hi.row_bits, cbr.row_bits, np.unique(ref[3]).tolist(), longest))
    if layout == "8000":                                         # 8192 bits a row: longer than any row of tonal (module docstring)
        assert cbr.row_bits == 8192 and int(ref[3].max()) == 0 and ref[2].all()
    else:
        assert int(((ref[3] > 0) & ref[2]).sum()) >= 1, "no row was requantised"
        if layout in CHAIN_KEEPS_A_ROW:
            _binding(cbr.row_bits, ref[3], ref[4], ref[2], unfit=False)
    d64, i64, _ = cbr.transrate_packed_rows(d128, i128)
    np.testing.assert_array_equal(d64.cpu().numpy(), ref[0])
    rows = _Rows((layout, "chain", C), cbr, d64, i64, off)
    src, age = np_conceal_plan(lost, 8)
    assert (age >= 1).any()
    one = {p: _one_shot(rows, lost, 8, p) for p in (False, True)}
    # the chunked route
    for pcm16 in (False, True):
        enc, dec = hi.stream(B0, C), cbr.stream(B0, C)
        assert dec.packed_chunk_launches(decode=True, conceal=True) == 1
        outs, data = [], []
        for a, b in _bounds(CHAIN_SPLITS):
            d, i, _ = enc.encode_packed_rows_chunk(xz[:, a * N0:b * N0])
            d2, i2, _ = cbr.transrate_packed_rows(d, i)
            data.append(d2.view(B0, b - a, C, cbr.row_bytes))
            outs.append(dec.decode_packed_chunk(d2, i2, pcm16, lost=_dev(lost[:, a:b]), max_age=8))
        assert torch.equal(torch.cat(data, dim=1), d64.view(B0, F, C, cbr.row_bytes))
        assert same_bits(torch.cat(outs, dim=1), one[pcm16]), "chunked chain != one-shot: %s pcm16=%s" % (layout, pcm16)
