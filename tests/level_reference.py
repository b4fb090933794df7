"""numpy restatement of the level of packed rows and of the selector, written from its rules on the
helpers of ``pack_reference`` (section 8b) and ``test_quantizer`` (section 8a).

The level of a row (b, f, c), with (q, s) the codes and scale factors ``np_unpack`` returns and bands [o_j, o_{j+1}):

1. band j is *bad* if s_j = -128;
2. Q_j = the sum of q_n^2 over band j as an exact integer, 0 in a bad or empty band;
3. w(s) = fp32(step(s) step(s));
4. e_j = fp32(fp32(Q_j) w(s_j)), the conversion rounding to nearest even; +0 in a bad band;
5. E = the fold tree over v[0 .. P), P the smallest power of two >= M, v[j] = e_j and +0 beyond M: for d = P/2 ... 1,
   v[i] = fp32(v[i] + v[i + d]) for i < d;
6. bad = 1 if any band of the row is bad.

The selector, on energy and valid [S, B, F, C]:

1. E[s,b,f] = ((E'_0 + E'_1) + ...) in float32, E'_c the energy where valid is non-zero and the energy > 0, else +0;
2. d = fp32(P[s,b,f-1] release); P[s,b,f] = d where d > E[s,b,f], else E[s,b,f]; P[s,b,-1] = state[s,b];
3. s is selected at (b, f) if P[s,b,f] > gate and fewer than n sources t have P_t > P_s or (P_t == P_s and t < s);
4. active = selected and valid != 0; state = P[:, :, F-1].
"""

import numpy as np

from pack_reference import np_unpack
from test_quantizer import np_step

F32 = np.float32


def band_squares(codes, sf, off):
    """Rules 1-2: codes [B, F, N, C], sf [B, F, M, C] -> (Q uint64 [B, F, M, C], bad bool [B, F, M, C])."""
    codes = np.asarray(codes).astype(np.int64)
    sf = np.asarray(sf).astype(np.int32)
    off = np.asarray(off, dtype=np.int64)
    M = len(off) - 1
    bad = sf == -128
    Q = np.zeros(sf.shape, dtype=np.uint64)
    for j in range(M):
        if off[j + 1] > off[j]:
            Q[:, :, j, :] = (codes[:, :, off[j]:off[j + 1], :] ** 2).sum(axis=2).astype(np.uint64)
    Q[bad] = 0
    return Q, bad


def weight(s):
    """Rule 3 for s in [-127, 127]."""
    st = np_step(s)
    return (st * st).astype(F32)


def band_energy(Q, sf, bad):
    """Rules 3-4: e float32 [B, F, M, C]."""
    s = np.where(bad, 0, np.asarray(sf).astype(np.int32))
    e = (Q.astype(F32) * weight(s)).astype(F32)              # (numpy converts uint64 to float32 to nearest even)
    return np.where(bad, F32(0), e).astype(F32)


def fold(e):
    """Rule 5 along axis 2: [B, F, M, C] -> [B, F, C]."""
    M = e.shape[2]
    P = 1
    while P < M:
        P *= 2
    v = np.zeros(e.shape[:2] + (P,) + e.shape[3:], dtype=F32)
    v[:, :, :M] = e
    while P > 1:
        P //= 2
        v = (v[:, :, :P] + v[:, :, P:2 * P]).astype(F32)
    return v[:, :, 0]


def in_band_order(e):
    """What rule 5 is not: ((e_0 + e_1) + e_2) + ... in float32."""
    t = e[:, :, 0].astype(F32)
    for j in range(1, e.shape[2]):
        t = (t + e[:, :, j]).astype(F32)
    return t


def level_of_codes(codes, sf, off):
    """Rules 1-6 on unpacked rows: (energy float32 [B, F, C], bad uint8 [B, F, C])."""
    Q, bad = band_squares(codes, sf, off)
    return fold(band_energy(Q, sf, bad)), bad.any(axis=2).astype(np.uint8)


def np_level(data, index, off, N):
    """What packed_rows_level returns: data uint8 [nbytes], index int64 [B, F, C] -> (energy, bad)."""
    return level_of_codes(*np_unpack(data, index, off, N), off)


def exact_energy(codes, sf, off):
    """Consequence (a)'s yardstick: the float64 sum of fp32(q step(s))^2 over the good bands, [B, F, C]."""
    off = np.asarray(off, dtype=np.int64)
    band = np.repeat(np.arange(len(off) - 1), np.diff(off))
    s = np.asarray(sf).astype(np.int32)[:, :, band, :]
    good = s != -128
    X = (np.asarray(codes).astype(F32) * np_step(np.where(good, s, 0))).astype(F32)
    return np.where(good, X.astype(np.float64) ** 2, 0.0).sum(axis=2)


def np_peaks(energy, valid, release, state):
    """Rules 1-2: P float32 [S, B, F]."""
    energy = np.asarray(energy, dtype=F32)
    S, B, F, C = energy.shape
    ok = energy > 0
    if valid is not None:
        ok &= np.asarray(valid) != 0
    lev = np.where(ok, energy, F32(0)).astype(F32)
    tot = np.zeros((S, B, F), dtype=F32)
    if C:
        tot = lev[..., 0]
        for c in range(1, C):
            tot = (tot + lev[..., c]).astype(F32)
    P = np.zeros((S, B, F), dtype=F32)
    prev = np.zeros((S, B), dtype=F32) if state is None else np.asarray(state, dtype=F32)
    for f in range(F):
        with np.errstate(invalid="ignore"):
            d = (prev * F32(release)).astype(F32)
            prev = np.where(d > tot[:, :, f], d, tot[:, :, f]).astype(F32)
        P[:, :, f] = prev
    return P


def np_select(energy, n, valid=None, release=0.5, gate=0.0, state=None):
    """Rules 1-4: (active uint8 [S, B, F, C], state' float32 [S, B], selected bool [S, B, F], P float32 [S, B, F])."""
    energy = np.asarray(energy, dtype=F32)
    S, B, F, C = energy.shape
    P = np_peaks(energy, valid, release, state)
    t = np.arange(S)
    before = (t[None, :] < t[:, None])[:, :, None, None]                     # [s, t]: t comes before s
    above = ((P[None] > P[:, None]) | ((P[None] == P[:, None]) & before)).sum(axis=1)
    selected = (P > F32(gate)) & (above < n)
    v = np.ones(energy.shape, dtype=bool) if valid is None else np.asarray(valid) != 0
    active = (selected[..., None] & v).astype(np.uint8)
    last = P[:, :, -1] if F else (np.zeros((S, B), dtype=F32) if state is None else np.asarray(state, dtype=F32))
    return active, last.copy(), selected, P
