"""numpy restatement of rate control, written from its rules 1-3.

A row is one (b, f, c).  sf0 and the codes of offset 0 are the quantiser of section 8a (``test_quantizer.np_quantize``);
a row's length is the packed length of section 8b before padding (``pack_reference.np_row_bits``).

1. s_j(k) = 0 in an empty band, -128 where sf0_j = -128, else clamp(sf0_j + k, -127, 127); the codes at k are section 8a
   rule 4 with s_j(k) in place of sf0_j.
2. bits_r(k) = np_row_bits(codes(k), s(k)) does not grow with k.
3. offset_r = the smallest k in [kmin, 254] with bits_r(k) <= R_r, else 254.

Two searches: ``brute_force`` requantises every bin at every k; ``band_extremes`` evaluates a row's length from each
band's largest and smallest X only (q is monotone in X for a fixed step), as the kernel does.
"""

import numpy as np

from pack_reference import bit_length, np_row_bits, zz
from test_quantizer import np_inv, np_quantize

K_MAX = 254


def sf_at(sf0, off, k):
    """Rule 1: the scale factors at offset k (a scalar or an array that broadcasts against sf0 [..., M, C])."""
    sf0 = np.asarray(sf0, dtype=np.int32)
    empty = (np.diff(np.asarray(off, dtype=np.int64)) == 0)[:, None]
    s = np.clip(sf0 + np.asarray(k, dtype=np.int32), -127, 127)
    return np.where(empty, 0, np.where(sf0 == -128, -128, s)).astype(np.int8)


def codes_at(X, s, off):
    """Section 8a rule 4 with the scale factors s [B, F, M, C]: codes int16 [B, F, N, C]."""
    X = np.asarray(X, dtype=np.float32)
    M = len(off) - 1
    band = np.repeat(np.arange(M), np.diff(np.asarray(off, dtype=np.int64)))
    sb = np.asarray(s, dtype=np.int32)[:, :, band, :]
    bad = sb == -128
    inv = np_inv(np.where(bad, 0, sb))
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.clip(np.rint((X * inv).astype(np.float32)), -32767, 32767)
    return np.where(bad, 0, q).astype(np.int16)


def _as_budget(R, shape):
    return np.broadcast_to(np.asarray(R, dtype=np.int64), shape)


def _finish(X, sf0, off, offset):
    s = sf_at(sf0, off, offset[:, :, None, :])
    codes = codes_at(X, s, off)
    return codes, s, offset.astype(np.int16), np_row_bits(codes, s, off).astype(np.int32)


def _search(bits_of, R, kmin):
    """Rule 3 by a scan of every k: bits_of(k) -> [B, F, C].  Also returns the bits at every k, [K, B, F, C]."""
    ks = np.arange(kmin, K_MAX + 1)
    bits = np.stack([bits_of(int(k)) for k in ks])
    met = bits <= _as_budget(R, bits.shape[1:])[None]
    offset = np.where(met.any(axis=0), ks[np.argmax(met, axis=0)], K_MAX)
    return offset, bits


def brute_force(X, thr, off, R, kmin=0):
    """Rules 1-3 by requantising every bin at every k in [kmin, 254]: (codes, sf, offset, row_bits, bits over k)."""
    X = np.asarray(X, dtype=np.float32)
    _, sf0 = np_quantize(X, thr, off)

    def bits_of(k):
        s = sf_at(sf0, off, k)
        return np_row_bits(codes_at(X, s, off), s, off)

    offset, bits = _search(bits_of, R, kmin)
    return _finish(X, sf0, off, offset) + (bits,)


def band_extremes(X, off):
    """Per band the largest and smallest X, [B, F, M, C] each (0 in an empty band)."""
    X = np.asarray(X, dtype=np.float32)
    B, F, N, C = X.shape
    M = len(off) - 1
    xmax = np.zeros((B, F, M, C), dtype=np.float32)
    xmin = np.zeros((B, F, M, C), dtype=np.float32)
    for j in range(M):
        if off[j + 1] > off[j]:
            xmax[:, :, j] = X[:, :, off[j]:off[j + 1]].max(axis=2)
            xmin[:, :, j] = X[:, :, off[j]:off[j + 1]].min(axis=2)
    return xmax, xmin


def fast_bits(sf0, xmax, xmin, off, k):
    """bits_r(k) [B, F, C] from the band extremes alone: the widest zz of a band is that of q(xmax) or q(xmin)."""
    s = sf_at(sf0, off, k).astype(np.int32)
    bad = s == -128
    inv = np_inv(np.where(bad, 0, s))
    with np.errstate(invalid="ignore", over="ignore"):
        qa = np.clip(np.rint((xmax * inv).astype(np.float32)), -32767, 32767)
        qb = np.clip(np.rint((xmin * inv).astype(np.float32)), -32767, 32767)
    qa, qb = (np.where(bad, 0, q).astype(np.int32) for q in (qa, qb))
    w = bit_length(np.maximum(zz(qa), zz(qb)))
    L = np.diff(np.asarray(off, dtype=np.int64))[:, None]
    cost = np.where(~bad & (w >= 1) & (L > 0), 8 + w * L, 0)
    return 5 * (len(off) - 1) + cost.sum(axis=-2)


def fast_search(X, thr, off, R, kmin=0):
    """Rules 1-3 with bits_r(k) from the band extremes: (codes, sf, offset, row_bits, bits over k)."""
    X = np.asarray(X, dtype=np.float32)
    _, sf0 = np_quantize(X, thr, off)
    xmax, xmin = band_extremes(X, off)
    offset, bits = _search(lambda k: fast_bits(sf0, xmax, xmin, off, k), R, kmin)
    return _finish(X, sf0, off, offset) + (bits,)


def quantize_budget(X, thr, off, R, kmin=0):
    """What quantize_to_budget returns: (codes, sf, offset, row_bits_out)."""
    return fast_search(X, thr, off, R, kmin)[:4]
