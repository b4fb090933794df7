"""Numpy restatement of the concealment of lost rows across the chunks of a stream ("Streams"), written
from the definition, frame by frame.  Per clip and channel the stream keeps

  gap g in [0, 32]   frames of the stream since the last row that arrived, at the end of the previous chunk (0: the previous
                     chunk's last row arrived; 32: no source within reach -- a new stream, after reset());
  the carried row    that row, here as its (codes, sf) the way unpack read them in the call that saw it.

Row (b, f, c) of a chunk of k frames, decoded with max_age m:
  1. the smallest a in [0, min(m, f)] with lost[b, f-a, c] == 0: read from frame f - a of the chunk, age a (conceal_reference);
  2. else, where g <= 31 and A = g + f + 1 <= m: read from the carried row, age A;
  3. else muted.
Afterwards, whatever m was: f* the last frame of the chunk that arrived -> g' = min(32, k-1 - f*) and that row is carried;
none arrived -> g' = min(32, g + k), the row is kept.
"""

import numpy as np

from conceal_reference import MAX_AGE, np_conceal_plan, np_fade

NO_SOURCE = 32
CARRIED = -2     # src: the carried row (conceal_reference: -1 = muted, >= 0 = a frame of the chunk)


def np_fresh_gap(B, C):
    return np.full((B, C), NO_SOURCE, dtype=np.int64)


def np_chunk_plan(lost, gap, max_age):
    """lost [B, k, C], gap [B, C] -> (src [B, k, C]: frame of the chunk, CARRIED or -1 (muted); age [B, k, C]; the new gap;
    last [B, C]: f*, -1 where no frame of the chunk arrived)."""
    assert 0 <= max_age <= MAX_AGE
    lost = np.asarray(lost) != 0
    gap = np.asarray(gap)
    B, k, C = lost.shape
    assert gap.shape == (B, C) and ((0 <= gap) & (gap <= NO_SOURCE)).all()
    src = np.full((B, k, C), -1, dtype=np.int64)
    age = np.zeros((B, k, C), dtype=np.int64)
    new_gap = np.empty((B, C), dtype=np.int64)
    last = np.full((B, C), -1, dtype=np.int64)
    for b in range(B):
        for c in range(C):
            g = int(gap[b, c])
            for f in range(k):
                found = False
                for a in range(min(max_age, f) + 1):
                    if not lost[b, f - a, c]:
                        src[b, f, c], age[b, f, c], found = f - a, a, True
                        break
                if not found and g <= 31 and g + f + 1 <= max_age:
                    src[b, f, c], age[b, f, c] = CARRIED, g + f + 1
                if not lost[b, f, c]:
                    last[b, c] = f
            new_gap[b, c] = min(NO_SOURCE, k - 1 - last[b, c]) if last[b, c] >= 0 else min(NO_SOURCE, g + k)
    return src, age, new_gap, last


def np_stream_plan(lost, splits, max_ages):
    """The chunks of `splits` frames of lost [B, F, C], each with its max_age, on a fresh stream -> (src, age) in frames of
    the WHOLE signal, as conceal_reference.np_conceal_plan states them (src -1: muted), and the gap after every chunk."""
    lost = np.asarray(lost)
    B, F, C = lost.shape
    assert sum(splits) == F and len(max_ages) == len(splits)
    gap = np_fresh_gap(B, C)
    carried = np.full((B, C), -1, dtype=np.int64)      # frame of the whole signal the carried row is
    srcs, ages, gaps = [], [], []
    at = 0
    for k, m in zip(splits, max_ages):
        src, age, gap, last = np_chunk_plan(lost[:, at:at + k], gap, m)
        whole = np.where(src >= 0, src + at, np.where(src == CARRIED, np.broadcast_to(carried[:, None, :], src.shape), -1))
        assert not ((src == CARRIED) & (whole < 0)).any(), "a carried row was read where there is none"
        carried = np.where(last >= 0, last + at, carried)
        srcs.append(whole)
        ages.append(age)
        gaps.append(gap.copy())
        at += k
    return np.concatenate(srcs, axis=1), np.concatenate(ages, axis=1), gaps


def np_conceal_chunk(codes, sf, lost, state, max_age):
    """One chunk: codes int16 [B, k, N, C] and sf int8 [B, k, M, C] as unpack gives them, state = (row codes [B, N, C], row sf
    [B, M, C], gap [B, C]) -> (codes', sf') of the rows a concealing decoder decodes, and the state after the chunk."""
    row_codes, row_sf, gap = state
    src, age, new_gap, last = np_chunk_plan(lost, gap, max_age)
    B, k, C = src.shape
    codes2, sf2 = np.zeros_like(codes), np.zeros_like(sf)
    new_codes, new_sf = row_codes.copy(), row_sf.copy()
    for b in range(B):
        for c in range(C):
            for f in range(k):
                s = src[b, f, c]
                if s >= 0:
                    codes2[b, f, :, c], sf2[b, f, :, c] = codes[b, s, :, c], sf[b, s, :, c]
                elif s == CARRIED:
                    codes2[b, f, :, c], sf2[b, f, :, c] = row_codes[b, :, c], row_sf[b, :, c]
            if last[b, c] >= 0:
                new_codes[b, :, c], new_sf[b, :, c] = codes[b, last[b, c], :, c], sf[b, last[b, c], :, c]
    return codes2, np_fade(sf2, age), (new_codes, new_sf, new_gap)


def np_fresh_state(B, N, M, C):
    return np.zeros((B, N, C), dtype=np.int16), np.zeros((B, M, C), dtype=np.int8), np_fresh_gap(B, C)


__all__ = ["CARRIED", "NO_SOURCE", "np_chunk_plan", "np_conceal_chunk", "np_conceal_plan", "np_fresh_gap", "np_fresh_state",
           "np_stream_plan"]
