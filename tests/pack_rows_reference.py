"""numpy restatement of the fixed-stride packed rows of DESIGN.md section 8b ("packed rows"), written from its rules on
``pack_reference.np_pack`` and ``rate_reference.quantize_budget``.

For a row budget R: row_bytes = ceil(R / 32) * 4, and row r = (b F + f) C + c takes bytes [r row_bytes, (r + 1) row_bytes).
A row whose codes and scale factors of ``quantize_budget(X, thr, off, R, kmin)`` pack into at most 8 row_bytes bits holds
``np_pack``'s bytes for them, then zero bytes (fits = 1); any other row holds the marked row -- every width field 31, then
zero bits (fits = 0).
"""

import numpy as np

from pack_reference import np_pack
from rate_reference import quantize_budget


def row_bytes(R):
    return (int(R) + 31) // 32 * 4


def marked_row(M, R):
    """The bytes of a slot that holds a row that does not fit: M width fields of 31, then zeros."""
    bits = np.zeros(8 * row_bytes(R), dtype=np.uint8)
    bits[:5 * M] = 1
    return np.packbits(bits, bitorder="little")


def np_rows_from_codes(codes, sf, row_bits_out, off, R):
    """codes [B, F, N, C], sf [B, F, M, C] and their packed lengths [B, F, C] -> (data uint8 [B F C row_bytes], index int64
    [B, F, C], fits bool [B, F, C])."""
    codes, sf = np.asarray(codes, dtype=np.int16), np.asarray(sf, dtype=np.int8)
    B, F, N, C = codes.shape
    rb = row_bytes(R)
    fits = np.asarray(row_bits_out, dtype=np.int64) <= 8 * rb
    marked = np.where(fits[:, :, None, :], sf, np.int8(-128)).astype(np.int8)   # width 31 follows whatever the codes are
    dense, start = np_pack(codes, marked, off)
    start = start.ravel()
    end = np.append(start[1:], len(dense))
    rows = B * F * C
    data = np.zeros(rows * rb, dtype=np.uint8)
    for r in range(rows):
        seg = dense[start[r]:end[r]]
        assert len(seg) <= rb, (r, len(seg), rb)
        data[r * rb:r * rb + len(seg)] = seg
    index = (np.arange(rows, dtype=np.int64) * rb).reshape(B, F, C)
    return data, index, fits


def np_pack_rows(X, thr, off, R, kmin=0):
    """What encode_packed_rows stores for spectra X and thresholds thr: (data, index, fits, offset, row_bits_out)."""
    codes, sf, offset, bits = quantize_budget(X, thr, off, R, kmin)
    return np_rows_from_codes(codes, sf, bits, off, R) + (offset, bits)
