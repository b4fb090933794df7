"""Numpy restatement of the concealment of lost rows, written from the definition, frame by frame:

  age[b, f, c]  = the smallest a in [0, min(max_age, f)] with lost[b, f-a, c] == 0; the row is read from frame f - a;
  muted         = no such a: the row is silence (a row that starts at nbytes: every width 0);
  sf'           = max(s - FADE * age, -127) for every s != -128, -128 stays; the codes are the source row's.
"""

import numpy as np

FADE = 4        # AC_CONCEAL_FADE
MAX_AGE = 31    # AC_CONCEAL_MAX_AGE


def np_conceal_plan(lost, max_age):
    """lost [B, F, C] (nonzero: lost) -> (src frame int64 [B, F, C], -1 where muted; age int64 [B, F, C], 0 where muted)."""
    assert 0 <= max_age <= MAX_AGE
    lost = np.asarray(lost) != 0
    B, F, C = lost.shape
    src = np.full((B, F, C), -1, dtype=np.int64)
    age = np.zeros((B, F, C), dtype=np.int64)
    for b in range(B):
        for c in range(C):
            for f in range(F):
                for a in range(min(max_age, f) + 1):
                    if not lost[b, f - a, c]:
                        src[b, f, c], age[b, f, c] = f - a, a
                        break
    return src, age


def np_src_index(index, lost, nbytes, max_age):
    """What PsychoacousticModel.conceal_plan returns: (src_index int64, age uint8)."""
    src, age = np_conceal_plan(lost, max_age)
    index = np.asarray(index)
    b, _, c = np.meshgrid(*[np.arange(n) for n in index.shape], indexing="ij")
    out = np.where(src >= 0, index[b, np.maximum(src, 0), c], np.int64(nbytes))
    return out.astype(np.int64), age.astype(np.uint8)


def np_fade(sf, age):
    """sf int8 [B, F, M, C], age [B, F, C] -> the scale factors of the concealed rows."""
    s = sf.astype(np.int32)
    low = np.maximum(s - FADE * np.asarray(age).astype(np.int32)[:, :, None, :], -127)
    return np.where(s == -128, s, low).astype(np.int8)


def np_conceal(codes, sf, lost, max_age):
    """codes int16 [B, F, N, C] and sf int8 [B, F, M, C] of the rows as sent (unpack's output) -> (codes', sf') of the rows
    a concealing decoder decodes: the source row's codes and faded scale factors, zeros for a muted row."""
    src, age = np_conceal_plan(lost, max_age)
    b, _, c = np.meshgrid(*[np.arange(n) for n in src.shape], indexing="ij")
    s = np.maximum(src, 0)
    codes2 = np.moveaxis(codes, 2, -1)[b, s, c]          # [B, F, C, N]
    sf2 = np.moveaxis(sf, 2, -1)[b, s, c]
    muted = src < 0
    codes2 = np.where(muted[..., None], np.int16(0), codes2)
    sf2 = np.where(muted[..., None], np.int8(0), sf2)
    codes2 = np.ascontiguousarray(np.moveaxis(codes2, -1, 2)).astype(np.int16)
    sf2 = np.ascontiguousarray(np.moveaxis(sf2, -1, 2)).astype(np.int8)
    return codes2, np_fade(sf2, age)
