"""Numpy restatement of the recovering decode of a chunk of a stream ("Streams"), written from the
definition, frame by frame.

A delayed stream.  A chunk of k rows is synthesised one frame behind: its k frames are ``D, row 0, ..., row k-2``, where D is
the deferred row -- the last row of the chunk before -- and the chunk's last row becomes the next D.  The state is section
8f's: gap g in [0, 32] and the carried row (stream_conceal_reference.py); D arrived exactly where g == 0, and then the
carried row is D.  On a fresh stream g = 32: D did not arrive and has no source before it.

Frame j of the chunk (j = 0: D, j >= 1: row j - 1), decoded with max_age m:
  0. it is lost and its successor -- row j of the chunk -- arrived: read from that row's start + redundant_at, age 0;
  1. else the nearest frame at or before it that arrived, a <= m frames back: a row of the chunk, or D where g == 0, or the
     carried row g frames before D where g <= 31 -- read from there, age a;
  2. else muted.
Afterwards the state is section 8f's over the chunk's rows 0 .. k-1, whatever m was (np_chunk_plan).

The flush is a chunk of one row marked lost: its one frame is D, which no successor recovers.
"""

import numpy as np

from conceal_reference import MAX_AGE
from stream_conceal_reference import CARRIED, NO_SOURCE, np_chunk_plan, np_fresh_gap


def np_recover_chunk_plan(lost, gap, max_age):
    """lost [B, k, C], gap [B, C] -> (src [B, k, C] of the chunk's k frames: a row of the chunk (of a recovered frame: its
    successor's, read at redundant_at), CARRIED or -1 (muted); age [B, k, C]; recovered bool [B, k, C]; the new gap; last
    [B, C]: the last row of the chunk that arrived, -1 where none did)."""
    assert 0 <= max_age <= MAX_AGE
    lost = np.asarray(lost) != 0
    gap = np.asarray(gap)
    B, k, C = lost.shape
    assert gap.shape == (B, C) and ((0 <= gap) & (gap <= NO_SOURCE)).all()
    src = np.full((B, k, C), -1, dtype=np.int64)
    age = np.zeros((B, k, C), dtype=np.int64)
    rec = np.zeros((B, k, C), dtype=bool)
    for b in range(B):
        for c in range(C):
            g = int(gap[b, c])
            for j in range(k):                        # the frame of row j - 1; row -1 is D
                gone = (g != 0) if j == 0 else lost[b, j - 1, c]
                if gone and not lost[b, j, c]:        # rule 0: the successor, row j, arrived
                    src[b, j, c], rec[b, j, c] = j, True
                    continue
                for a in range(max_age + 1):          # rule 1: row j - 1 - a
                    r = j - 1 - a
                    if r >= 0 and not lost[b, r, c]:
                        src[b, j, c], age[b, j, c] = r, a
                        break
                    if r < 0 and g <= 31 and r == -1 - g:
                        src[b, j, c], age[b, j, c] = CARRIED, a
                        break
                    if r < -1 - g:
                        break
    _, _, new_gap, last = np_chunk_plan(lost, gap, 0)
    return src, age, rec, new_gap, last


def np_recover_stream_plan(lost, splits, max_ages, flush_age=None):
    """The recovering chunks of `splits` rows of lost [B, F, C], each with its max_age, on a fresh stream, and the flush
    (flush_age, default the last chunk's) -> (src, age, recovered) [B, F + 1, C] in frames of the FRONT-EXTENDED signal -- frame
    0 the lost frame in front, frame f + 1 row f -- as protect_reference.np_recover_plan states them on cat(ones, lost): src -1
    where muted, e + 1 for a recovered frame e; and ``across`` bool [B, F + 1, C]: the frame was recovered from a row of a later
    call than the one that delivered it."""
    lost = np.asarray(lost)
    B, F, C = lost.shape
    assert sum(splits) == F and len(max_ages) == len(splits)
    gap = np_fresh_gap(B, C)
    carried = np.full((B, C), -1, dtype=np.int64)      # extended frame of the carried row
    srcs, ages, recs, across = [], [], [], []
    at = 0                                              # the chunk's row 0 is extended frame at + 1, its frame 0 (D) is at
    calls = [(k, m) for k, m in zip(splits, max_ages) if k > 0]
    calls.append((1, max_ages[-1] if flush_age is None else flush_age))
    for n, (k, m) in enumerate(calls):
        flush = n == len(calls) - 1
        part = np.ones((B, 1, C), dtype=np.uint8) if flush else lost[:, at:at + k]
        src, age, rec, gap, last = np_recover_chunk_plan(part, gap, m)
        whole = np.where(src >= 0, src + at + 1, np.where(src == CARRIED, np.broadcast_to(carried[:, None, :], src.shape), -1))
        assert not ((src == CARRIED) & (whole < 0)).any(), "a carried row was read where there is none"
        carried = np.where(last >= 0, last + at + 1, carried)
        srcs.append(whole)
        ages.append(age)
        recs.append(rec)
        first = np.zeros_like(rec)
        first[:, 0] = at > 0                            # frame 0 is D: delivered by the call before
        across.append(rec & first)
        at += k
    return (np.concatenate(srcs, axis=1), np.concatenate(ages, axis=1), np.concatenate(recs, axis=1),
            np.concatenate(across, axis=1))


def front_extended(lost):
    """cat(ones, lost) along frames: the pattern of the one-shot call a delayed stream equals."""
    lost = np.asarray(lost)
    return np.concatenate((np.ones_like(lost[:, :1]), lost), axis=1)


def np_protect_chunks(data, index, off, N, R, R2, splits):
    """Protect chunk by chunk ("Streams") from its definition: protect_reference.np_protect on every chunk
    of `splits` frames of index [B, F, C], where frame 0 of a chunk takes the copy at R2 of the chunk before's last INPUT row
    (np_transrate of that row), with its fits and offset, and a fresh stream the values of f = 0.  Returns the chunks' (slots
    [B, k, C, slot_bytes], fits, red_fits, offset, red_offset), put together along frames."""
    from pack_rows_reference import row_bytes
    from protect_reference import np_protect
    from transrate_reference import np_transrate
    index = np.asarray(index)
    B, F, C = index.shape
    assert sum(splits) == F
    rb, sb = row_bytes(R), row_bytes(R) + row_bytes(R2)
    carry, parts, at = None, [], 0
    for k in splits:
        if k == 0:
            continue
        part = index[:, at:at + k]
        slots, _, fits, red_fits, offset, red_offset = np_protect(data, part, off, N, R, R2)
        slots, red_fits, red_offset = slots.reshape(B, k, C, sb).copy(), red_fits.copy(), red_offset.copy()
        if carry is not None:
            slots[:, 0, :, rb:], red_fits[:, 0], red_offset[:, 0] = carry
        last = np_transrate(data, part[:, -1:], off, N, R2)
        carry = (last[0].reshape(B, C, sb - rb), np.asarray(last[2], dtype=bool)[:, 0], np.asarray(last[3], dtype=np.int16)[:, 0])
        parts.append((slots, fits, red_fits, offset, red_offset))
        at += k
    return tuple(np.concatenate([p[i] for p in parts], axis=1) for i in range(5))
