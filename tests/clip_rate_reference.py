"""numpy restatement of rate control per clip, written from its rules 1-5 on top of section 8c
(``rate_reference``: ``sf_at``, ``codes_at`` and ``fast_bits``, a row's length from its band extremes).

A clip b has F*C rows in r = f*C + c order, a budget T_b (int64) and a lower bound kmin.

1. len_r(k) = 32 ceil(bits_r(k) / 32); total_b(k) = sum_r len_r(k) does not grow with k.
2. k_b = the smallest k in [kmin, 254] with total_b(k) <= T_b, else 254.
3. p_b = 0 where k_b = kmin or total_b(254) > T_b; otherwise, with d_r = len_r(k_b - 1) - len_r(k_b) >= 0, the number of rows
   whose inclusive prefix sum of d is at most T_b - total_b(k_b).
4. offset_r = k_b - 1 for r < p_b, else k_b.
5. codes and sf at offset_r, offset, row_bits_out = bits_r(offset_r), clip_offset = k_b, clip_bits_out = sum_r len_r(offset_r).

Two searches for rule 2: ``scan`` evaluates every k, ``bisect`` at most nine (rule 1: the total does not grow).
"""

import numpy as np

from pack_reference import np_row_bits
from rate_reference import K_MAX, band_extremes, codes_at, fast_bits, sf_at
from test_quantizer import np_quantize


def padded(bits):
    """Rule 1: a row's packed length with its padding to 32 bits."""
    return (np.asarray(bits, dtype=np.int64) + 31) // 32 * 32


def floor_bits(F, C, M):
    """The length of a clip that stores no band."""
    return F * C * 32 * ((5 * M + 31) // 32)


class ClipStats:
    """What the rules read of X and thr: sf0 and the band extremes.  ``bits(k)`` -> bits_r(k) [B, F*C] for a scalar k or
    one k per clip [B]; ``total(k)`` -> total_b(k) [B]."""

    def __init__(self, X, thr, off):
        self.X = np.asarray(X, dtype=np.float32)
        self.off = np.asarray(off)
        _, self.sf0 = np_quantize(self.X, thr, off)
        self.xmax, self.xmin = band_extremes(self.X, off)
        self.B, self.F, _, self.C = self.X.shape

    def bits(self, k):
        k = np.asarray(k, dtype=np.int32)
        if k.ndim:
            k = k.reshape(self.B, 1, 1, 1)
        return fast_bits(self.sf0, self.xmax, self.xmin, self.off, k).reshape(self.B, self.F * self.C)

    def total(self, k):
        return padded(self.bits(k)).sum(axis=1)


def _budgets(T, B):
    return np.broadcast_to(np.asarray(T, dtype=np.int64), (B,))


def search_scan(st, T, kmin):
    """Rule 2 by a scan of every k: (k_b [B], total_b over k [K, B])."""
    T = _budgets(T, st.B)
    ks = np.arange(kmin, K_MAX + 1)
    totals = np.stack([st.total(int(k)) for k in ks])
    met = totals <= T[None]
    return np.where(met.any(axis=0), ks[np.argmax(met, axis=0)], K_MAX), totals


def search_bisect(st, T, kmin):
    """Rule 2 by bisection: (k_b [B], the number of evaluations of total_b)."""
    T = _budgets(T, st.B)
    lo = np.full(st.B, kmin, dtype=np.int64)
    hi = np.full(st.B, K_MAX, dtype=np.int64)
    evaluations = 0
    while (lo < hi).any():
        act = lo < hi
        mid = lo + ((hi - lo) >> 1)
        fits = st.total(mid) <= T
        hi = np.where(act & fits, mid, hi)
        lo = np.where(act & ~fits, mid + 1, lo)
        evaluations += 1
    return lo, evaluations


def fill(st, T, kmin, kb):
    """Rules 3 and 4: (offset [B, F*C], p_b [B], d [B, F*C], total_b(k_b) [B])."""
    T = _budgets(T, st.B)
    at = padded(st.bits(kb))
    under = padded(st.bits(np.maximum(kb - 1, kmin)))
    d = under - at
    assert np.all(d >= 0)
    total = at.sum(axis=1)
    runs = (kb > kmin) & (total <= T)
    p = np.where(runs, (np.cumsum(d, axis=1) <= (T - total)[:, None]).sum(axis=1), 0)
    offset = np.where(np.arange(st.F * st.C)[None, :] < p[:, None], kb[:, None] - 1, kb[:, None])
    return offset, p, d, total


def quantize_clip_budget(X, thr, off, T, kmin=0, search=search_bisect, st=None):
    """What ac_quantize_clip_budget returns: (codes, sf, offset [B,F,C], row_bits_out [B,F,C], clip_offset [B],
    clip_bits_out [B]) and, for the tests, a dict with p_b, d, total_b(k_b) and the ClipStats (pass it back as ``st`` to
    search the same X and thr again)."""
    st = st if st is not None else ClipStats(X, thr, off)
    kb = search(st, T, kmin)[0]
    offset, p, d, total = fill(st, T, kmin, kb)
    offset = offset.reshape(st.B, st.F, st.C)
    s = sf_at(st.sf0, off, offset[:, :, None, :])
    codes = codes_at(st.X, s, off)
    row_bits = np_row_bits(codes, s, off).astype(np.int32)
    clip_bits = padded(row_bits).reshape(st.B, -1).sum(axis=1)
    return (codes, s, offset.astype(np.int16), row_bits, kb.astype(np.int16), clip_bits.astype(np.int64),
            {"p": p, "d": d, "total": total, "stats": st})
