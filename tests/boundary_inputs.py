"""Inputs and budgets that sit exactly on the decisions of the quantiser, the packer and rate control (DESIGN.md sections
8a to 8e), for ``test_decision_boundaries.py``.  numpy only.

Every decision in that code is a comparison (``bits <= budget``, ``total <= T``, ``crit(s) <= min(thr)``, ``bits <= 8
row_bytes``) or a rounding (``rint``, the clamp at +-32767).  The builders here choose values at which the two sides are
equal, and one unit to either side.  They hold no rule of their own: every table and every expected value comes from the
restatements the suite already has (``np_quantize``, ``rate_reference``, ``clip_rate_reference``, ``transrate_reference``,
``pack_reference``), and every builder asserts, on those references alone, that its input shows the boundary it was built
for -- a budget that no longer binds with equality fails here, before any kernel is asked.
"""

import collections

import numpy as np

from clip_rate_reference import fill, quantize_clip_budget, search_scan
from pack_reference import bit_length, np_row_bits, zz
from rate_reference import K_MAX
from test_quantizer import CRIT, S_ALL, np_inv, np_quantize, np_step

F32 = np.float32
FLT_MAX = np.finfo(F32).max
FLT_MIN = np.finfo(F32).tiny
SUB_MIN = np.nextafter(F32(0), F32(1))
SUB_MAX = np.nextafter(FLT_MIN, F32(0))
INF = F32(np.inf)


# ---- 1. budgets that bind with equality ------------------------------------------------------------------------------
Target = collections.namedtuple("Target", "row k R")     # row (b, f, c); a plateau start k; R = bits_row(k)


def plateau_starts(bits, kmin=0, lo=321, hi=None):
    """bits [K, B, F, C] over k = kmin .. 254 -> every Target with kmin < k < 254, bits(k) < bits(k - 1) -- k is the first
    offset of its length -- whose budgets R - 1, R and R + 1 separate k from k - 1 (bits(k - 1) >= R + 2) and lie in
    [lo - 1, hi]."""
    bits = np.asarray(bits, dtype=np.int64)
    assert bits.shape[0] == K_MAX - kmin + 1
    start = np.zeros(bits.shape, dtype=bool)
    start[1:-1] = bits[:-2] >= bits[1:-1] + 2
    start &= bits >= lo
    if hi is not None:
        start &= bits + 1 <= hi
    return [Target((int(b), int(f), int(c)), int(i) + kmin, int(bits[i, b, f, c])) for i, b, f, c in np.argwhere(start)]


def pick_three(targets, kmin=0):
    """A small one (k - kmin in 1 .. 3), the median one and the largest below 254, by k; three different rows where the
    targets allow it."""
    assert targets, "no row has a plateau start"
    by_k = sorted(targets, key=lambda t: (t.k, t.row))
    small = [t for t in by_k if 1 <= t.k - kmin <= 3]
    assert small, "no plateau start at an offset of 1 .. 3 above min_offset"
    out = [small[0], by_k[-1]]
    rest = [t for t in by_k if t.row not in (out[0].row, out[1].row)] or by_k
    out.insert(1, rest[len(rest) // 2])
    return out


def edge_budgets(search, targets, kmin=0):
    """The budget plan of one input: for every target the budgets R - 1, R and R + 1 from kmin, then R from min_offset = k
    and from k + 1.  ``search(R, kmin)`` -> the reference's (codes, sf, offset, row_bits_out).  Returns a list of
    (R, kmin, target, reference) after asserting on the reference what each budget was chosen for."""
    plan = []
    for t in targets:
        assert kmin < t.k < K_MAX
        for R, k0 in ((t.R - 1, kmin), (t.R, kmin), (t.R + 1, kmin), (t.R, t.k), (t.R, t.k + 1)):
            ref = search(R, k0)
            offset, bits = int(ref[2][t.row]), int(ref[3][t.row])
            if k0 == t.k + 1:
                assert offset == t.k + 1 and bits <= t.R, (t, R, k0, offset, bits)
            elif R == t.R - 1:
                assert offset > t.k and bits < t.R, (t, R, k0, offset, bits)      # one bit less: the next plateau
            else:
                assert offset == t.k and bits == t.R, (t, R, k0, offset, bits)    # equality, and one bit of slack
            plan.append((R, k0, t, ref))
    return plan


def per_row_budgets(bits, rng, fallback, kmin=0):
    """One budget per row, each on its own edge: R_r = bits_r(k_r) at a plateau start k_r of the row drawn by ``rng``; a
    row without one keeps ``fallback``'s entry.  bits [K, B, F, C] over k = kmin .. 254.  Returns (R int32 [B, F, C],
    k [B, F, C] with -1 where the row has no plateau start)."""
    bits = np.asarray(bits, dtype=np.int64)
    drop = np.zeros(bits.shape, dtype=bool)
    drop[1:] = bits[1:] < bits[:-1]
    R = np.array(fallback, dtype=np.int64)
    k = np.full(R.shape, -1, dtype=np.int64)
    for b, f, c in np.ndindex(R.shape):
        ks = np.flatnonzero(drop[:, b, f, c])
        if len(ks):
            i = int(rng.choice(ks))
            R[b, f, c], k[b, f, c] = bits[i, b, f, c], i + kmin
    return R.astype(np.int32), k


def check_per_row(search, R, k, kmin=0):
    """The precondition of the per-row plan, on the reference: at least half the rows sit at equality -- at R the row's
    offset is k_r with row_bits_out == R_r, at R - 1 it is greater.  Returns the two references."""
    at, under = search(R, kmin), search(R - 1, kmin)
    has = k >= 0
    assert has.mean() >= 0.5, "%d of %d rows have a plateau start" % (has.sum(), has.size)
    assert np.array_equal(at[2][has], k[has]) and np.array_equal(at[3][has], R[has])
    assert np.all(under[2][has] > k[has])
    return at, under


# ---- 1b. rows of constant length for the slot's slack (section 8e) -----------------------------------------------------
def constant_row(off, length):
    """Codes and scale factors [N], [M] of a row whose packed length is ``length`` bits at every offset: every stored band
    has sf 127, which no offset raises, and codes that requantise to themselves (saturated +-32767 at width 16, and one or
    two bands of a chosen narrower width to reach the exact length)."""
    off = np.asarray(off, dtype=np.int64)
    L = np.diff(off)
    M = len(L)
    codes, sf = np.zeros(int(off[-1]), np.int16), np.zeros(M, np.int8)

    def store(j, w):
        sf[j] = 127
        q = np.where(np.arange(L[j]) % 2 == 0, 32767, -32767) if w == 16 else np.full(L[j], -(1 << (w - 1)))
        codes[off[j]:off[j + 1]] = q

    one, two = int(np.flatnonzero(L == 1)[0]), int(np.flatnonzero(L == 2)[0])     # the two bands that adjust the length
    left = length - 5 * M
    for j in sorted((j for j in range(M) if L[j] > 0 and j not in (one, two)), key=lambda j: -L[j]):
        if left - (8 + 16 * L[j]) >= 19:
            store(j, 16)
            left -= 8 + 16 * L[j]
    assert 19 <= left <= 64, left
    w2 = next(w for w in range(1, 17) if 9 <= left - (8 + 2 * w) <= 24)
    store(two, w2)
    store(one, left - (8 + 2 * w2) - 8)
    return codes, sf


def slot_rows(off, R):
    """Four rows of constant length around a budget R with R % 32 == 31: R (met with equality at offset 0), R + 1 = 8
    row_bytes (not met, offset 254, and the slot filled to its last bit), R + 2 (one bit more than the slot: the marked
    row) and R - 1.  Returns (codes [1, 4, N, 1], sf [1, 4, M, 1], lengths)."""
    assert R % 32 == 31
    lengths = [R, R + 1, R + 2, R - 1]
    rows = [constant_row(off, n) for n in lengths]
    codes = np.stack([r[0] for r in rows])[None, :, :, None]
    sf = np.stack([r[1] for r in rows])[None, :, :, None]
    np.testing.assert_array_equal(np_row_bits(codes, sf, off).ravel(), lengths)
    return codes, sf, lengths


# ---- 2. a clip's budget (section 8d) ---------------------------------------------------------------------------------
def clip_edges(st, kmin=0):
    """Per-clip budgets [B] on every edge of section 8d's rules, from the ClipStats ``st``: a dict name -> T int64 [B].

    ``plateau`` / ``plateau-1``: T_b = total_b(k) at the first k of a total (k > kmin), and one bit less.
    ``fill`` / ``fill-1``: T_b = total_b(k) + cumsum(d)[p] exactly, with d_p > 0 and the sum short of total_b(k - 1): rule
    3's inclusive prefix sum takes row p; one bit less and it does not.
    ``last`` / ``last-1``: T_b = total_b(254), met at 254, and one bit less, met nowhere."""
    totals = search_scan(st, np.zeros(st.B, np.int64), kmin)[1]                   # [K, B] over k = kmin .. 254
    T = {name: np.zeros(st.B, np.int64) for name in ("plateau", "fill")}
    for b in range(st.B):
        ks = np.flatnonzero(totals[1:, b] < totals[:-1, b]) + 1
        assert len(ks), "clip %d: its total never shrinks" % b
        T["plateau"][b] = totals[ks[len(ks) // 3], b]
        done = False
        for i in ks[len(ks) // 2:].tolist() + ks[:len(ks) // 2].tolist():
            kb = np.full(st.B, i + kmin, dtype=np.int64)
            d = fill(st, totals[i], kmin, kb)[2][b]
            cs = np.cumsum(d)
            ps = np.flatnonzero((d > 0) & (cs < cs[-1]))
            if len(ps):
                T["fill"][b] = totals[i, b] + cs[ps[len(ps) // 2]]
                done = True
                break
        assert done, "clip %d: no offset at which a proper prefix of its rows steps back" % b
    T["last"] = totals[-1].astype(np.int64)
    for name in ("plateau", "fill", "last"):
        T[name + "-1"] = T[name] - 1
    return T


def check_clip_edges(st, T, off, kmin=0):
    """On the reference alone: every edge of ``clip_edges`` shows in every clip.  Returns name -> reference."""
    ref = {name: quantize_clip_budget(st.X, None, off, t, kmin, st=st) for name, t in T.items()}
    kb = {name: r[4].astype(np.int64) for name, r in ref.items()}
    assert np.all(ref["plateau"][6]["total"] == T["plateau"]) and np.all(kb["plateau"] > kmin)
    assert np.all(kb["plateau-1"] > kb["plateau"])
    a, b = ref["fill"][6], ref["fill-1"][6]
    assert np.array_equal(kb["fill"], kb["fill-1"]) and np.all(kb["fill"] > kmin)
    assert np.all(a["p"] > b["p"]) and np.all(ref["fill"][5] == T["fill"])          # the clip's bits meet the budget exactly
    assert np.all(a["d"][np.arange(st.B), b["p"]] > 0)                               # the row that one bit decides
    assert np.all(ref["last"][5] == T["last"])                                       # met, with equality
    assert np.all(kb["last-1"] == K_MAX) and np.all(ref["last-1"][5] > T["last-1"])  # unmet
    return ref


# ---- 3. every edge of the scale-factor criterion ---------------------------------------------------------------------------
def criterion_values():
    """765 + 9 band minima: pred(CRIT[s]), CRIT[s] and succ(CRIT[s]) for every s, then the specials."""
    edges = np.stack([np.nextafter(CRIT, -INF), CRIT, np.nextafter(CRIT, INF)], axis=1).ravel().astype(F32)
    special = np.array([0.0, -0.0, SUB_MIN, SUB_MAX, FLT_MIN, -1e-3, -FLT_MAX, np.nextafter(CRIT[-1], INF), FLT_MAX], dtype=F32)
    return np.concatenate([edges, special])


def _fillers(v):
    """What the band's other bins may hold: succ(v), 2 v, 1.0 and FLT_MAX where finite and not below v (else v itself)."""
    with np.errstate(over="ignore"):
        cand = [np.nextafter(v, INF), F32(2) * v, F32(1), FLT_MAX]
    return [c if np.isfinite(c) and c >= v else v for c in cand]


def criterion_input(off, C, rng, B=2):
    """X, thr [B, F, N, C] in which every value of ``criterion_values`` is the smallest threshold of one (row, channel,
    band): at the band's first bin, last bin or middle in turn, the band's other bins succ(v), 2 v, 1.0 or FLT_MAX in turn.
    X is noise some tens of steps wide, far from saturating.  Returns (X, thr, v [B, F, M, C]: each band's planted value)."""
    off = np.asarray(off, dtype=np.int64)
    N, M = int(off[-1]), len(off) - 1
    L = np.diff(off)
    bands = np.flatnonzero(L > 0)
    values = criterion_values()
    per_frame = len(bands) * C
    F = -(-len(values) // (per_frame * B)) + 1                                 # one frame more: the rotation goes on
    thr = np.ones((B, F, N, C), dtype=F32)
    planted = np.ones((B, F, M, C), dtype=F32)
    level = np.ones((B, F, N, C), dtype=F32)
    i = 0
    for b in range(B):
        for f in range(F):
            for c in range(C):
                for j in bands:
                    v = values[i % len(values)]
                    lap = i // len(values)
                    a, n = off[j], L[j]
                    thr[b, f, a:a + n, c] = _fillers(v)[(i + i // 12 + lap) % 4]
                    thr[b, f, a + (0, n - 1, n // 2)[(i + i // 3 + lap) % 3], c] = v
                    planted[b, f, j, c] = v
                    level[b, f, a:a + n, c] = np.clip(v, CRIT[0], CRIT[-1])
                    i += 1
    X = (rng.standard_normal((B, F, N, C)) * 40.0 * level.astype(np.float64)).astype(F32)
    return X, thr, planted


def check_criterion_input(X, thr, planted, off):
    """On the reference alone: every value is some band's minimum, bit for bit; pred(CRIT[s]) gives s - 1, CRIT[s] and its
    successor give s, everything at or below zero and every subnormal gives -127; every s occurs; no code saturates."""
    off = np.asarray(off, dtype=np.int64)
    bands = np.flatnonzero(np.diff(off) > 0)
    mins = np.stack([thr[:, :, off[j]:off[j + 1]].min(axis=2) for j in bands], axis=2)
    got = planted[:, :, bands, :]
    np.testing.assert_array_equal(mins.view(np.uint32), got.view(np.uint32))       # (as bits: -0.0 is not +0.0)
    values = criterion_values()
    assert set(values.view(np.uint32).tolist()) <= set(got.view(np.uint32).ravel().tolist())
    codes, sf = np_quantize(X, thr, off)
    sfb = sf[:, :, bands, :].astype(np.int64)
    assert set(S_ALL.tolist()) <= set(sfb.ravel().tolist())
    assert np.abs(codes).max() < 32767 and np.abs(codes).max() > 8 and (sf != -128).all()
    for k, s in enumerate(S_ALL):
        for which, want in ((0, max(s - 1, -127)), (1, s), (2, s)):
            hit = got.view(np.uint32) == values[3 * k + which:3 * k + which + 1].view(np.uint32)[0]
            assert hit.any() and np.all(sfb[hit] == want), (s, which)
    for v in (F32(0.0), F32(-0.0), SUB_MIN, SUB_MAX, F32(-1e-3), -FLT_MAX):
        hit = got.view(np.uint32) == np.array([v]).view(np.uint32)[0]
        assert hit.any() and np.all(sfb[hit] == -127), v
    assert np.all(sfb[got == FLT_MAX] == 127) and np.all(sfb[got == FLT_MIN] == -127)
    return codes, sf


# ---- 4. ties, clamps and every scale factor ---------------------------------------------------------------------------------
TIE_K = sorted({0, 1, 2, 3, 4, 32766, 32767} | {(1 << w) - 1 for w in range(1, 15)} | {1 << w for w in range(1, 15)})


def tie_candidates(s):
    """fp32((k + 0.5) step(s)) and the float on either side of it, k over TIE_K, both signs: float32 [6 len(TIE_K)]."""
    k = np.array(TIE_K, dtype=np.float64) + 0.5
    x = (k * np_step(s).astype(np.float64)).astype(F32)
    x = np.stack([np.nextafter(x, -INF), x, np.nextafter(x, INF)], axis=1).ravel()
    return np.concatenate([x, -x]).astype(F32)


def tie_input(off, C, B=2, F=12):
    """X, thr [B, F, N, C]: every band is pinned to one scale factor s by thr = CRIT[s] -- s walks [-127, 127] over the
    (row, channel, band) slots -- and its bins walk ``tie_candidates(s)``.  The first band of two bins or more with s = -127
    holds +-FLT_MAX (the product overflows: codes +-32767)."""
    off = np.asarray(off, dtype=np.int64)
    N, M = int(off[-1]), len(off) - 1
    L = np.diff(off)
    cand = {int(s): tie_candidates(s) for s in S_ALL}
    at = collections.Counter()
    X, thr = np.zeros((B, F, N, C), F32), np.ones((B, F, N, C), F32)
    slot, big = 0, False
    for b in range(B):
        for f in range(F):
            for c in range(C):
                for j in np.flatnonzero(L > 0):
                    s = int(S_ALL[(slot * 37) % 255])
                    slot += 1
                    idx = (at[s] + 7 * np.arange(L[j])) % len(cand[s])      # (7: coprime with 6 len(TIE_K) = 186)
                    at[s] += 7 * int(L[j])
                    X[b, f, off[j]:off[j + 1], c] = cand[s][idx]
                    thr[b, f, off[j]:off[j + 1], c] = CRIT[s + 127]
                    if s == -127 and L[j] >= 2 and not big:
                        X[b, f, off[j], c], X[b, f, off[j] + 1, c] = FLT_MAX, -FLT_MAX
                        big = True
    assert big
    return X, thr


def check_tie_input(X, thr, off):
    """On the reference alone: for each residue s & 3 at least 1000 products fp32(X inv(s)) are exactly k + 0.5, with even
    and odd k among them, and at least one product of 32767.5 or just above rounds to 32768 and clamps (exactly 32767.5
    for every residue that has such a product); the +-FLT_MAX bins give +-32767; codes
    of every zigzag width 1 .. 16 occur; every s in [-127, 127] occurs.  Returns np_quantize's (codes, sf)."""
    off = np.asarray(off, dtype=np.int64)
    codes, sf = np_quantize(X, thr, off)
    band = np.repeat(np.arange(len(off) - 1), np.diff(off))
    s = sf[:, :, band, :].astype(np.int32)
    assert set(S_ALL.tolist()) <= set(s.ravel().tolist()) and (sf != -128).all()
    with np.errstate(over="ignore"):
        p = np.abs((X * np_inv(s)).astype(F32)).astype(np.float64)
    p = np.where(np.isfinite(p), p, 0.0)
    tie = p - np.floor(p) == 0.5
    for r in range(4):
        m = tie & ((s & 3) == r)
        k = np.floor(p[m]).astype(np.int64)
        assert m.sum() >= 1000 and (k % 2 == 0).any() and (k % 2 == 1).any(), (r, int(m.sum()))
        assert np.all(np.abs(codes[m]) == np.minimum(k + (k % 2), 32767))       # half to even, then the clamp
        # 32767.5 rounds to 32768 and clamps.  With s & 3 == 2 no float32 has that product (inv = fp32(2^-1/2): the
        # products next to it are 32767.498 and 32767.502); there the clamp is held by the larger of the two
        assert r == 2 or (k == 32767).any(), r
        over = ((s & 3) == r) & (p >= 32767.5) & (p < 32767.51)
        assert over.any() and np.all(np.abs(codes[over]) == 32767), r
    big = np.abs(X) == FLT_MAX
    assert big.sum() == 2 and np.array_equal(np.sort(codes[big]), [-32767, 32767])
    assert set(bit_length(zz(codes)).ravel().tolist()) >= set(range(1, 17))
    return codes, sf
