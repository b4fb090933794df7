"""Shared pieces of tests/test_protect_layouts.py: what numpy must read in the redundant copies of protected slots before a
recovering decode is compared with anything, and the inputs whose copy ends where ``data`` ends.  numpy only.

A recovered row (b, f, c) is read from ``index[b, f+1, c] + o``: the copy the next slot carries.  ``copies`` reads every such
start with ``np_unpack``; the conditions below are held on the copies of the rows that the loss patterns of
``test_protect._patterns`` recover, taken together.
"""

import numpy as np

from conceal_reference import np_conceal_plan, np_fade
from oracle.audiocodec_oracle import MDCTOracle
from pack_reference import np_code_fields, np_unpack, np_widths
from protect_reference import np_recover_plan, np_recover_src_index
from test_quantizer import np_dequantize

N0, M0 = 1024, 64
AGES = (1, 8)


def slots_noise(C, Kp, B=3):
    """The input of ``test_protect._slots(C, Kp)`` in numpy: ``_pcm``'s ramped noise at seed 30 + Kp, cut to Kp - 1 blocks."""
    K = max(Kp - 1, 1)
    rng = np.random.default_rng(30 + Kp)
    x = (rng.uniform(-1, 1, (B, K * N0, C)) * np.linspace(0.01, 1, K * N0)[None, :, None]).astype(np.float32)
    return np.ascontiguousarray(x[:, :(Kp - 1) * N0])


def recovered(patterns_of, ages=AGES):
    """bool [B, F, C]: the rows some pattern of ``patterns_of(max_age)`` recovers, over ``ages``."""
    rec = None
    for max_age in ages:
        for lost in patterns_of(max_age).values():
            r = np_recover_plan(lost, max_age)[2]
            rec = r if rec is None else rec | r
    return rec


def copies(data, index, o, off):
    """(codes [B, F, N, C], sf [B, F, M, C], widths [B, F, M, C]) of what lies at index[b, f+1, c] + o, for f < F - 1 (the last
    frame's entry is a row of silence, at len(data))."""
    index = np.asarray(index, dtype=np.int64)
    at = np.roll(index, -1, axis=1) + np.int64(o)
    at[:, -1] = len(data)
    codes, sf = np_unpack(data, at, off, N0)
    return codes, sf, np_widths(codes, sf, off)


def stored_bands(w):
    """[B, F, C]: bands of width 1 .. 16 per row, of widths [B, F, M, C]."""
    return ((w >= 1) & (w <= 16)).sum(axis=2)


def crossing_rows(w, off):
    """bool [B, F, C]: the row holds a code field of >= 9 bits across a 32-bit word boundary (a copy starts on a word
    boundary: positions count from its start), as fused_layouts.width_facts counts them."""
    B, F, M, C = w.shape
    wr = np.moveaxis(w, 3, 2).reshape(B * F * C, M)
    pos, wb, keep = np_code_fields(wr, off)
    return (keep & (wb >= 9) & ((pos % 32) + wb > 32)).any(axis=1).reshape(B, F, C)


def oracle_pcm(codes, sf, off):
    """float64 blocks [B, F + 1, N, C] of the float64 oracle's synthesis of np_dequantize(codes, sf)."""
    Xh = np_dequantize(codes, sf, off).astype(np.float64)
    assert np.isfinite(Xh).all()
    B, F, _, C = codes.shape
    return MDCTOracle(N0, "vorbis", np.float64).inverse_transform(Xh).reshape(B, F + 1, N0, C)


def fade_shows(data, index, o, off, lost, max_age, what):
    """On the reference alone: in the plan of (lost, max_age) some recovered row whose copy stores a band with sf > -127 would
    have been concealed at an age >= 1, and the float64 PCM of the two blocks it covers differs from the PCM with that row
    faded by 4 age -- a copy read as a concealed row is -- and from the PCM with the row muted.  Returns the row."""
    index = np.asarray(index, dtype=np.int64)
    src, age = np_recover_src_index(index, lost, len(data), max_age, o)
    rec = np_recover_plan(lost, max_age)[2]
    as_concealed = np_conceal_plan(lost, max_age)[1]
    codes, sf = np_unpack(data, src, off, N0)
    w = np_widths(codes, sf, off)
    loud = (((w >= 1) & (w <= 16)) & (sf > -127)).any(axis=2)
    rows = np.argwhere(rec & loud & (as_concealed >= 1))
    assert len(rows), "no recovered copy with a band above sf -127 that concealment would fade: %s" % (what,)
    b, f, c = (int(v) for v in rows[0])
    ref = oracle_pcm(codes, np_fade(sf, age), off)
    faded_age = age.astype(np.int64).copy()
    faded_age[b, f, c] = as_concealed[b, f, c]
    faded = oracle_pcm(codes, np_fade(sf, faded_age), off)
    silent = codes.copy()
    silent[b, f, :, c] = 0
    muted = oracle_pcm(silent, np_fade(sf, age), off)
    for other, name in ((faded, "faded"), (muted, "muted")):
        d = np.abs(ref[b, f:f + 2, :, c] - other[b, f:f + 2, :, c]).max()
        assert d > 4.0 / 32768.0, "the %s row is within %.2e of the recovered one: %s" % (name, d, what)
    return b, f, c


def hold_conditions(data, index, o, off, patterns_of, what, red_offset=None):
    """What keeps a recovering comparison on these slots from being vacuous, on numpy's reading of the bytes.  Over the copies
    of the rows the patterns recover: at most a quarter lack a non-zero code; one holds a code field of >= 9 bits across a word
    boundary; at least 6 distinct stored widths; the fade would show (fade_shows, on the "isolated" pattern at max_age 8).
    ``red_offset``, where given: some copy was requantised.  Returns the counts."""
    codes, sf, w = copies(data, index, o, off)
    rec = recovered(patterns_of)
    n = int(rec.sum())
    assert n >= 8, (what, n)
    assert not (w[np.broadcast_to(rec[:, :, None, :], w.shape)] == 31).any(), "a recovered copy holds a width-31 band: %s" % (what,)
    empty = int((~(codes != 0).any(axis=2))[rec].sum())
    crossing = int(crossing_rows(w, off)[rec].sum())
    wr = w[np.broadcast_to(rec[:, :, None, :], w.shape)]
    widths = sorted(set(wr[(wr >= 1) & (wr <= 16)].tolist()))
    most = int(stored_bands(w)[rec].max())
    print("%s: %d recovered copies, %d without a non-zero code, %d with a wide field across a word boundary, widths %s, "
          "up to %d stored bands" % (what, n, empty, crossing, widths, most))
    assert 4 * empty <= n, (what, empty, n)
    assert crossing >= 1, what
    assert len(widths) >= 6, (what, widths)
    if red_offset is not None:
        assert int(np.asarray(red_offset).max()) > 0, "no copy was requantised: %s" % (what,)
    fade_shows(data, index, o, off, patterns_of(8)["isolated"], 8, what)
    return n, empty, crossing, widths
