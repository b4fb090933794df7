"""numpy restatement of requantising and transrating, written from its rules on the helpers of
``rate_reference`` (section 8c), ``pack_reference`` (section 8b) and ``test_quantizer`` (section 8a).

A row is one (b, f, c).  Its canonical codes q and scale factors s are ``np_canon``'s (what ``np_unpack`` returns for a row
``np_pack`` wrote; for a damaged row, what ``np_unpack`` returns is taken as it is).  X^ = np_dequantize(q, s), and with a
budget R' and kmin in [0, 254]:

1. s_j(k) = 0 in an empty band, -128 where s_j = -128, else clamp(s_j + k, -127, 127) (``sf_at`` with sf0 := s);
2. the codes at k are section 8a rule 4 on X^ with s_j(k) (``codes_at``);
3. offset_r = the smallest k in [kmin, 254] with bits_r(k) <= R', else 254; row_bits_out = bits_r(offset_r).

Two searches, as in ``rate_reference``: ``requant_brute`` requantises every bin at every k; ``requant_fast`` evaluates a
row's length from each band's largest and smallest X^ only.  ``np_transrate`` is the rows-to-rows form: ``np_unpack``, the
requantiser at kmin 0, ``np_rows_from_codes``.
"""

import numpy as np

from pack_reference import np_canon, np_row_bits, np_unpack
from pack_rows_reference import np_rows_from_codes
from rate_reference import _finish, _search, band_extremes, codes_at, fast_bits, sf_at
from test_quantizer import np_dequantize


def _spectrum(codes, sf, off):
    q, s = np_canon(codes, sf, off)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(np_dequantize(q, s, off), dtype=np.float32), s


def requant_brute(codes, sf, off, R, kmin=0):
    """Rules 1-3 by requantising every bin at every k: (codes, sf, offset, row_bits_out, bits over k)."""
    Xh, s = _spectrum(codes, sf, off)

    def bits_of(k):
        sk = sf_at(s, off, k)
        return np_row_bits(codes_at(Xh, sk, off), sk, off)

    offset, bits = _search(bits_of, R, kmin)
    return _finish(Xh, s, off, offset) + (bits,)


def requant_fast(codes, sf, off, R, kmin=0):
    """Rules 1-3 with bits_r(k) from the band extremes of X^: (codes, sf, offset, row_bits_out, bits over k)."""
    Xh, s = _spectrum(codes, sf, off)
    with np.errstate(invalid="ignore"):
        xmax, xmin = band_extremes(Xh, off)
    offset, bits = _search(lambda k: fast_bits(s, xmax, xmin, off, k), R, kmin)
    return _finish(Xh, s, off, offset) + (bits,)


def requantize_budget(codes, sf, off, R, kmin=0):
    """What requantize_to_budget returns: (codes, sf, offset, row_bits_out)."""
    return requant_fast(codes, sf, off, R, kmin)[:4]


def np_transrate(data, index, off, N, R):
    """What transrate_packed_rows stores at the budget R: (data', index', fits', offset, row_bits_out)."""
    codes, sf = np_unpack(data, index, off, N)
    rc, rs, offset, bits = requantize_budget(codes, sf, off, R, 0)
    return np_rows_from_codes(rc, rs, bits, off, R) + (offset, bits)
