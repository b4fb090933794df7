"""numpy restatement of protected rows and the recovering decode, written from its rules on
``transrate_reference.np_transrate`` (section 8e) and ``conceal_reference`` (section 8f).

Protected rows.  With a row budget R (row_bytes rb) and a redundant budget R2 (red_bytes = ceil(R2 / 32) * 4), slot_bytes =
rb + red_bytes and slot r = (b F + f) C + c holds:

  bytes [0, rb)            the slot np_transrate writes for row (b, f, c) at R, with its fits and offset;
  bytes [rb, slot_bytes)   f >= 1: the slot np_transrate writes for the INPUT row (b, f-1, c) at R2 (red_fits, red_offset by
                           the slot that holds the copy); f = 0: zero bytes, red_fits 1, red_offset 0.

The copy of frame F - 1 has no slot.

Recovery.  Ahead of section 8f's rules: a row with lost[b, f, c] != 0, f + 1 < F and lost[b, f+1, c] == 0 is read from
index[b, f+1, c] + o with age 0.  Every other row is what ``conceal_reference.np_conceal_plan`` says, unchanged.
"""

import numpy as np

from conceal_reference import np_conceal_plan, np_src_index
from pack_rows_reference import row_bytes
from transrate_reference import np_transrate


def slot_bytes(R, R2):
    return row_bytes(R) + row_bytes(R2)


def np_protect(data, index, off, N, R, R2):
    """What protect_packed_rows stores: (data', index', fits, red_fits, offset, red_offset)."""
    index = np.asarray(index)
    B, F, C = index.shape
    rb, sb = row_bytes(R), slot_bytes(R, R2)
    prim = np_transrate(data, index, off, N, R)
    red = np_transrate(data, index, off, N, R2)
    slots = np.zeros((B, F, C, sb), dtype=np.uint8)
    red_fits = np.ones((B, F, C), dtype=bool)
    red_offset = np.zeros((B, F, C), dtype=np.int16)
    p_rows, r_rows = prim[0].reshape(B, F, C, rb), red[0].reshape(B, F, C, sb - rb)
    for b in range(B):
        for f in range(F):
            for c in range(C):
                slots[b, f, c, :rb] = p_rows[b, f, c]
                if f >= 1:     # the copy of the frame before, of the same clip and channel
                    slots[b, f, c, rb:] = r_rows[b, f - 1, c]
                    red_fits[b, f, c] = red[2][b, f - 1, c]
                    red_offset[b, f, c] = red[3][b, f - 1, c]
    index_out = (np.arange(B * F * C, dtype=np.int64) * sb).reshape(B, F, C)
    return slots.reshape(-1), index_out, np.asarray(prim[2], dtype=bool), red_fits, np.asarray(prim[3], dtype=np.int16), red_offset


def np_recover_plan(lost, max_age):
    """lost [B, F, C] -> (src frame int64, -1 where muted; age int64; recovered bool): a recovered row's src is f + 1 and
    it is read at that row's start + redundant_at."""
    lost = np.asarray(lost) != 0
    B, F, C = lost.shape
    src, age = np_conceal_plan(lost, max_age)
    rec = np.zeros((B, F, C), dtype=bool)
    for b in range(B):
        for c in range(C):
            for f in range(F):
                if lost[b, f, c] and f + 1 < F and not lost[b, f + 1, c]:      # rule 0, ahead of the others
                    rec[b, f, c], src[b, f, c], age[b, f, c] = True, f + 1, 0
    return src, age, rec


def np_recover_src_index(index, lost, nbytes, max_age, redundant_at):
    """What PsychoacousticModel.conceal_plan(..., redundant_at=) returns: (src_index int64, age uint8)."""
    index = np.asarray(index, dtype=np.int64)
    out, age = np_src_index(index, lost, nbytes, max_age)
    _, _, rec = np_recover_plan(lost, max_age)
    nxt = np.roll(index, -1, axis=1) + np.int64(redundant_at)
    return np.where(rec, nxt, out).astype(np.int64), np.where(rec, 0, age).astype(np.uint8)
