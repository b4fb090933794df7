"""numpy restatement of the packed bitstream of quantised spectra, written from the format's rules.

A row is one (b, f, c) of codes int16 [B, F, N, C] and sf int8 [B, F, M, C].  Bit p of a row is bit p % 8 of its byte
p // 8 (the same as bit p % 32 of its little-endian word p // 32).  Fields, LSB first: M widths of 5 bits; the 8-bit sf of
every band with width 1..16; the zigzag codes of those bands at their width; zero padding to 32 bits.
"""

import numpy as np

W_NONFINITE = 31


def zz(q):
    """(q << 1) ^ (q >> 15) on the int16 code taken as 16 bits."""
    q = np.asarray(q).astype(np.int32)
    return ((q << 1) & 0xFFFF) ^ ((q >> 15) & 0xFFFF)


def unzz(z):
    z = np.asarray(z).astype(np.int32)
    return ((z >> 1) ^ -(z & 1)).astype(np.int16)


def bit_length(m):
    m = np.asarray(m).astype(np.int64)
    w = np.zeros(m.shape, dtype=np.int64)
    for k in range(32):
        w += (m >> k) > 0
    return w


def _rows(codes, sf):
    """[B, F, N, C], [B, F, M, C] -> [R, N], [R, M] in (b, f, c) order."""
    B, F, N, C = codes.shape
    M = sf.shape[2]
    return (np.moveaxis(codes, 3, 2).reshape(B * F * C, N), np.moveaxis(sf, 3, 2).reshape(B * F * C, M))


def _unrows(a, B, F, C):
    return np.moveaxis(a.reshape(B, F, C, a.shape[-1]), 2, 3)


def np_widths(codes, sf, off):
    """Width fields [..., M, C]: 31 where sf = -128, else the bit length of the band's largest zz (0 for an empty band)."""
    z = zz(codes)
    M = len(off) - 1
    mx = np.zeros(sf.shape, dtype=np.int64)
    for j in range(M):
        if off[j + 1] > off[j]:
            mx[..., j, :] = z[..., off[j]:off[j + 1], :].max(axis=-2)
    w = bit_length(mx)
    return np.where(np.asarray(sf) == -128, W_NONFINITE, w)


def _stored(w):
    return (w >= 1) & (w <= 16)


def np_row_bits(codes, sf, off):
    """Bits of every row before padding, [B, F, C]: 5M + sum over bands of width 1..16 of (8 + w (o_{j+1} - o_j))."""
    w = np_widths(codes, sf, off)
    L = np.diff(np.asarray(off, dtype=np.int64))
    M = len(off) - 1
    cost = np.where(_stored(w), 8 + w * L[:, None], 0)
    return 5 * M + cost.sum(axis=-2)


def _put(bits, pos, val, width):
    """Writes val's low `width` bits LSB first at bit positions pos (flattened arrays of equal shape)."""
    pos, val, width = (np.asarray(a, dtype=np.int64).ravel() for a in (pos, val, width))
    for k in range(int(width.max(initial=0))):
        m = width > k
        bits[pos[m] + k] = (val[m] >> k) & 1


def np_code_fields(w, off):
    """Where a row's code fields lie: widths w [R, M] -> (pos [R, N]: first bit of bin i's field, counted from the row's
    start; width [R, N]; keep [R, N]: the bin's band is stored)."""
    off = np.asarray(off, dtype=np.int64)
    M = len(off) - 1
    L = np.diff(off)
    st = _stored(w)
    cb = np.where(st, w * L, 0)
    boff = np.cumsum(cb, axis=1) - cb
    base = 5 * M + 8 * st.sum(axis=1, keepdims=True)
    band = np.repeat(np.arange(M), L)
    i = np.arange(int(off[-1]))
    return base + boff[:, band] + w[:, band] * (i - off[band]), w[:, band], st[:, band]


def np_pack(codes, sf, off):
    """codes int16 [B, F, N, C], sf int8 [B, F, M, C] -> (data uint8 [nbytes], index int64 [B, F, C])."""
    codes, sf = np.asarray(codes, dtype=np.int16), np.asarray(sf, dtype=np.int8)
    B, F, N, C = codes.shape
    off = np.asarray(off, dtype=np.int64)
    M = len(off) - 1
    L = np.diff(off)
    cr, sr = _rows(codes, sf)
    w = np_widths(cr[:, :, None], sr[:, :, None], off)[:, :, 0]          # [R, M]
    st = _stored(w)
    rowbits = 5 * M + np.where(st, 8 + w * L, 0).sum(axis=1)
    rowbytes = (rowbits + 31) // 32 * 4
    index = np.concatenate([[0], np.cumsum(rowbytes)[:-1]]).astype(np.int64) if len(rowbytes) else np.zeros(0, np.int64)
    total = int(rowbytes.sum())
    bits = np.zeros(total * 8, dtype=np.uint8)
    start = index[:, None] * 8
    # 1. widths
    _put(bits, start + 5 * np.arange(M), w, np.full(w.shape, 5))
    # 2. scale factors of the stored bands
    cnt = np.cumsum(st, axis=1) - st
    _put(bits, (start + 5 * M + 8 * cnt)[st], (sr.astype(np.int64) & 0xFF)[st], np.full(int(st.sum()), 8))
    # 3. codes of the stored bands
    pos, wb, keep = np_code_fields(w, off)
    pos = start + pos
    _put(bits, pos[keep], zz(cr)[keep], wb[keep])
    data = np.packbits(bits, bitorder="little")
    return data, index.reshape(B, F, C)


def _get(data, pos, width):
    """The `width`-bit fields at absolute bit positions pos; bits outside data read as 0."""
    nbits = 8 * len(data)
    pos = np.asarray(pos, dtype=np.int64)
    width = np.broadcast_to(np.asarray(width, dtype=np.int64), pos.shape)
    out = np.zeros(pos.shape, dtype=np.int64)
    for k in range(int(width.max(initial=0))):
        p = pos + k
        inside = (p >= 0) & (p < nbits) & (width > k)
        pc = np.where(inside, p, 0)
        b = (data[pc >> 3].astype(np.int64) >> (pc & 7)) & 1 if len(data) else np.zeros(p.shape, np.int64)
        out |= np.where(inside, b, 0) << k
    return out


def np_unpack(data, index, off, N):
    """data uint8 [nbytes], index int64 [B, F, C] -> canonical (codes int16 [B, F, N, C], sf int8 [B, F, M, C]).  A width
    of 17..30 reads as 31 (a non-finite band); bits at or beyond len(data) read as 0."""
    data = np.asarray(data, dtype=np.uint8)
    index = np.asarray(index, dtype=np.int64)
    B, F, C = index.shape
    off = np.asarray(off, dtype=np.int64)
    M = len(off) - 1
    L = np.diff(off)
    start = index.reshape(-1)[:, None] * 8
    w = _get(data, start + 5 * np.arange(M), 5)
    w = np.where(w > 16, W_NONFINITE, w)
    st = _stored(w)
    cnt = np.cumsum(st, axis=1) - st
    sv = _get(data, start + 5 * M + 8 * cnt, 8)
    sv = np.where(sv >= 128, sv - 256, sv)
    sf = np.where(w == W_NONFINITE, -128, np.where(st, sv, 0)).astype(np.int8)
    cb = np.where(st, w * L, 0)
    boff = np.cumsum(cb, axis=1) - cb
    base = start + 5 * M + 8 * st.sum(axis=1, keepdims=True)
    band = np.repeat(np.arange(M), L)
    i = np.arange(N)
    pos = base + boff[:, band] + w[:, band] * (i - off[band])
    keep = st[:, band]
    z = _get(data, np.where(keep, pos, 0), np.where(keep, w[:, band], 0))
    codes = np.where(keep, unzz(z), 0).astype(np.int16)
    return _unrows(codes, B, F, C), _unrows(sf, B, F, C)


def np_canon(codes, sf, off):
    """What unpack(pack(codes, sf)) returns: codes 0 where sf = -128; sf 0 in a band of width 0; the rest unchanged."""
    codes, sf = np.array(codes, dtype=np.int16), np.array(sf, dtype=np.int8)
    w = np_widths(codes, sf, off)
    M = len(off) - 1
    band = np.repeat(np.arange(M), np.diff(np.asarray(off, dtype=np.int64)))
    codes[(sf == -128)[..., band, :]] = 0
    sf[w == 0] = 0
    return codes, sf
