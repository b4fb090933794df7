"""numpy restatement of mixing packed rows, written from its rules on the helpers of ``rate_reference``
(section 8c), ``pack_reference`` / ``pack_rows_reference`` (section 8b), ``transrate_reference`` (section 8e) and
``test_quantizer`` (section 8a).

Sources i = 0 .. S-1 hold rows of the same shape; a row is one (b, f, c).  With (q_i, s_i) the canonical codes and scale
factors (``np_canon``) of source i's row, gains[i] in [-254, 254] and active[i] per row:

* band j of source i is *bad* if the row is active and s_ij = -128, *stored* if the row is active, the band is not bad and
  holds a non-zero code;
1. g_ij = clamp(s_ij + gains[i], -127, 127) in a stored band; X_i = fp32(q_i step(g_ij)), +0 in a band that is not stored,
   NaN in a bad band;
2. X^ = ((X_0 + X_1) + X_2) + ... in float32, in source order;
3. s0_j = -128 if band j is bad in any source, else the largest g_ij over the sources that store band j, else 0;
4. section 8c rules 1-3 on (X^, s0) with kmin = 0 and the budget R;
5. the slot is ``np_rows_from_codes``'s.

``mix_brute`` requantises every bin at every k, ``mix_fast`` takes a row's length from the band extremes of X^ as the kernel
does.  ``np_mix`` is the rows-to-rows form.
"""

import numpy as np

from pack_reference import np_canon, np_row_bits, np_unpack, np_widths
from pack_rows_reference import np_rows_from_codes
from rate_reference import _finish, _search, band_extremes, codes_at, fast_bits, sf_at
from test_quantizer import CRIT, np_step

F32 = np.float32


def _bands(off):
    off = np.asarray(off, dtype=np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def mix_spectrum(rows, off, gains=None, active=None):
    """Rules 1-3: rows = [(codes [B, F, N, C], sf [B, F, M, C]), ...] -> (X^ float32 [B, F, N, C], s0 int8 [B, F, M, C],
    g int32 [S, B, F, M, C] with -129 where source i does not store the band)."""
    S = len(rows)
    assert S >= 1
    gains = [0] * S if gains is None else [int(g) for g in gains]
    assert len(gains) == S and all(-254 <= g <= 254 for g in gains)
    band = _bands(off)
    Xh = bad = None
    gs = []
    for i, (codes, sf) in enumerate(rows):
        q, s = np_canon(codes, sf, off)
        B, F, N, C = q.shape
        on = np.ones((B, F, 1, C), dtype=bool) if active is None else (np.asarray(active)[i] != 0)[:, :, None, :]
        is_bad = on & (s == -128)
        w = np_widths(q, s, off)
        stored = on & ~is_bad & (w >= 1) & (w <= 16)
        g = np.clip(s.astype(np.int32) + gains[i], -127, 127)
        step = np.where(is_bad, F32(np.nan), np_step(np.where(stored, g, 0))).astype(F32)
        with np.errstate(invalid="ignore"):
            X = (np.where(stored[:, :, band, :], q, 0).astype(F32) * step[:, :, band, :]).astype(F32)
        X = np.where(stored[:, :, band, :] | is_bad[:, :, band, :], X, F32(0))          # +0 where nothing is stored
        with np.errstate(invalid="ignore"):
            Xh = X if Xh is None else (Xh + X).astype(F32)
        bad = is_bad if bad is None else bad | is_bad
        gs.append(np.where(stored, g, -129))
    gs = np.stack(gs)
    top = gs.max(axis=0)
    s0 = np.where(bad, -128, np.where(top == -129, 0, top)).astype(np.int8)
    return Xh, s0, gs


def mix_brute(rows, off, R, gains=None, active=None):
    """Rules 1-5 by requantising every bin at every k: (codes, sf, offset, row_bits_out, bits over k)."""
    Xh, s0, _ = mix_spectrum(rows, off, gains, active)

    def bits_of(k):
        sk = sf_at(s0, off, k)
        return np_row_bits(codes_at(Xh, sk, off), sk, off)

    offset, bits = _search(bits_of, R, 0)
    return _finish(Xh, s0, off, offset) + (bits,)


def mix_fast(rows, off, R, gains=None, active=None):
    """Rules 1-5 with bits_r(k) from the band extremes of X^: (codes, sf, offset, row_bits_out, bits over k)."""
    Xh, s0, _ = mix_spectrum(rows, off, gains, active)
    with np.errstate(invalid="ignore"):
        xmax, xmin = band_extremes(Xh, off)
    offset, bits = _search(lambda k: fast_bits(s0, xmax, xmin, off, k), R, 0)
    return _finish(Xh, s0, off, offset) + (bits,)


def mix_budget(rows, off, R, gains=None, active=None):
    """What mix_to_budget returns: (codes, sf, offset, row_bits_out)."""
    return mix_fast(rows, off, R, gains, active)[:4]


def threshold_of(s0, off):
    """Consequence (d): thr [B, F, N, C] = crit(s0 of the bin's band), 1.0 where s0 = -128."""
    s0 = np.asarray(s0, dtype=np.int32)
    t = np.where(s0 == -128, F32(1), CRIT[np.where(s0 == -128, 0, s0) + 127]).astype(F32)
    return t[:, :, _bands(off), :]


def np_mix(sources, off, N, R, gains=None, active=None):
    """What mix_packed_rows stores at the budget R: sources = [(data, index [B, F, C]), ...] -> (data', index', fits',
    offset, row_bits_out)."""
    rows = [np_unpack(data, index, off, N) for data, index in sources]
    rc, rs, offset, bits = mix_budget(rows, off, R, gains, active)
    return np_rows_from_codes(rc, rs, bits, off, R) + (offset, bits)
