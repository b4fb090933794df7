"""Protected rows in a stream ("Streams"): ``StreamingMDCT.decode_packed_chunk(..., lost=,
redundant_at=)`` recovers a lost row from the copy its successor's slot carries, chunk by chunk, and ``flush_packed`` ends the
stream.  ``AudioCodec.protect_stream(...).protect_chunk`` (k_protect_ps) is the sending side: protect_packed_rows chunk by
chunk, a chunk's frame-0 slots taking the copy of the chunk before's last row from a carry.  For any split its slots, flags and
offsets equal the one-shot ``protect_packed_rows`` -- the parent's k_protect_p -- byte for byte.

A recovering stream is *delayed*: a chunk of k rows returns the frames of ``D, row 0, ..., row k-2``, D being the last row of
the chunk before, so that the successor of every frame it synthesises is a row of the chunk in hand.  The definition is by
frame index and exact: however ``index [B, K', C]`` is split, the chunks' outputs and the flush are blocks 0 .. K' of the
one-shot ``decode_packed(data, cat(index[:, :1], index), lost=cat(ones, lost), max_age=, redundant_at=)`` -- the parent's
kernel k_inv_fast_plr, the yardstick here -- bit for bit, float32 and 16-bit PCM.  Held to each other:

  * the kernel k_inv_fast_plsr (one launch per chunk where ``packed_chunk_launches(decode=True, conceal=True, recover=True)``
    is 1);
  * the composition in torch ops with the state in tensors (``AC_DECODE_PACKED_NOFUSE=1``, and every other configuration);
  * that one-shot call on the front-extended signal;
  * tests/stream_recover_reference.py, the rules in numpy chunk by chunk, against protect_reference.np_recover_plan.

The slots come from copies that carry content, protected with R = R2 = 1365: a 341-bit copy decodes to near-silence and hides
a wrong read (test_protect_layouts.py).  The splits of K' = 12 and 45 rows run on fused_layouts.tonal's recipe at that length
(``_tonal``): numpy's reading of the bytes (protect_layouts.hold_conditions) and of the plan (a frame recovered across a chunk
boundary from a copy with a non-zero code, in every split of more than one chunk) is asserted before any kernel result is
looked at.  protect_layouts.slots_noise serves the other tests and one comparison of its own; its copies hold up to 24 bands
but no code wider than 3 bits (measured on the MI355X: widths 1 .. 3, no field across a word boundary), so hold_conditions
is not asked of it, only the non-zero code behind a boundary.
"""

import ctypes
import functools
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib
from audiocodec_amd.codec import StreamingMDCT
from conftest import ROOT
from protect_reference import np_recover_plan
from stream_conceal_reference import CARRIED, np_fresh_gap
from stream_order import Harness, same_bits
from stream_recover_reference import front_extended, np_protect_chunks, np_recover_chunk_plan, np_recover_stream_plan

N0 = 1024
NOFUSE = "AC_DECODE_PACKED_NOFUSE"
AGES = (0, 1, 8, 31)
HEADER = os.path.join(ROOT, "include", "audiocodec_amd.h")
SPLITS = [(12, (12,)), (12, (1,) * 12), (12, (5, 7)), (12, (2, 3, 7)), (45, (40, 5)), (45, (3, 40, 2))]
SPLIT_IDS = ["-".join(map(str, s)) if len(s) < 12 else "1x12" for _, s in SPLITS]


def _bounds(splits):
    out, a = [], 0
    for k in splits:
        out.append((a, a + k))
        a += k
    return out


def _lost(F, frames, B=1, C=1):
    lost = np.zeros((B, F, C), dtype=np.uint8)
    lost[:, list(frames)] = 1
    return lost


def _stream_plan(lost, splits, max_age):
    return np_recover_stream_plan(lost, splits, (max_age,) * len(splits))


def _one_shot_plan(lost, max_age):
    return np_recover_plan(front_extended(lost), max_age)


def _same_plan(lost, splits, max_age):
    """The chunked plan of a split equals np_recover_plan on the front-extended pattern; returns it."""
    src, age, rec, across = _stream_plan(lost, splits, max_age)
    want = _one_shot_plan(lost, max_age)
    assert np.array_equal(src, want[0]) and np.array_equal(age, want[1]) and np.array_equal(rec, want[2]), (splits, max_age)
    return src, age, rec, across


# ---- CPU: the rules in numpy, on hand-written patterns ------------------------------------------------------------------------
def test_plan_the_last_row_of_a_chunk_lost_and_the_next_first_row_arrived():
    """Row 4 is lost, row 5 opens the next chunk and arrived: recovered across the boundary, from row 5's slot."""
    lost = _lost(12, [4])
    src, age, rec, across = _same_plan(lost, (5, 7), 8)
    assert rec[0, 5, 0] and src[0, 5, 0] == 6 and age[0, 5, 0] == 0 and across[0, 5, 0]     # extended frame 5 is row 4
    assert int(rec.sum()) == 2 and rec[0, 0, 0] and not across[0, 0, 0]                      # ... and the frame in front
    # the chunk itself: D is lost (gap 1), its successor row 0 arrived
    src, age, rec, gap, last = np_recover_chunk_plan(_lost(7, []), np.array([[1]]), 8)
    assert rec[0, :, 0].tolist() == [True] + [False] * 6 and src[0, :, 0].tolist() == [0, 0, 1, 2, 3, 4, 5]
    assert gap[0, 0] == 0 and last[0, 0] == 6


def test_plan_the_last_row_of_a_chunk_lost_and_the_next_first_row_lost():
    """Rows 4 and 5 are lost: row 4 is concealed from the carried row 3 at age 1, row 5 recovered from row 6."""
    lost = _lost(12, [4, 5])
    src, age, rec, across = _same_plan(lost, (5, 7), 8)
    assert not rec[0, 5, 0] and src[0, 5, 0] == 4 and age[0, 5, 0] == 1
    assert rec[0, 6, 0] and src[0, 6, 0] == 7 and not across[0, 6, 0]
    src, age, rec, gap, last = np_recover_chunk_plan(_lost(7, [0]), np.array([[1]]), 8)
    assert src[0, :2, 0].tolist() == [CARRIED, 1] and age[0, :2, 0].tolist() == [1, 0] and rec[0, :2, 0].tolist() == [False, True]
    # max_age 0: D is muted
    src, age, rec, _, _ = np_recover_chunk_plan(_lost(7, [0]), np.array([[1]]), 0)
    assert src[0, 0, 0] == -1 and not rec[0, 0, 0]


@pytest.mark.parametrize("max_age", [1, 3, 8, 31])
def test_plan_a_run_across_a_boundary_at_max_age_and_one_more(max_age):
    """Row 2 arrives, then a run that crosses the boundary at row 4; its last row is recovered, the one before is max_age old,
    or one more."""
    F = max_age + 9
    for extra in (0, 1):
        n = max_age + 1 + extra                          # rows 3 .. 2 + n are lost; row 3 + n arrives and recovers row 2 + n
        lost = _lost(F, range(3, 3 + n))
        src, age, rec, _ = _same_plan(lost, (4, F - 4), max_age)
        end = 3 + n                                      # extended frame of the run's last row
        assert rec[0, end, 0] and src[0, end, 0] == end + 1
        if extra == 0:
            assert src[0, end - 1, 0] == 3 and age[0, end - 1, 0] == max_age
        else:
            assert src[0, end - 1, 0] == -1 and age[0, end - 1, 0] == 0 and src[0, end - 2, 0] == 3
    # the rule on one chunk: the carried row g frames before D, at age g + j
    src, age, rec, gap, last = np_recover_chunk_plan(np.ones((1, max_age + 2, 1)), np.array([[1]]), max_age)
    assert src[0, :, 0].tolist() == [CARRIED] * max_age + [-1, -1] and age[0, :, 0].tolist() == list(range(1, max_age + 1)) + [0, 0]
    assert not rec.any() and gap[0, 0] == min(32, max_age + 3) and last[0, 0] == -1


@pytest.mark.parametrize("g", [0, 5, 31, 32])
def test_plan_a_whole_chunk_lost(g):
    k = 6
    src, age, rec, gap, last = np_recover_chunk_plan(np.ones((1, k, 1)), np.array([[g]]), 31)
    reach = max(0, min(k, 32 - g)) if g <= 31 else 0     # frames with g + j <= 31
    assert src[0, :, 0].tolist() == [CARRIED] * reach + [-1] * (k - reach)
    assert age[0, :, 0].tolist() == [g + j for j in range(reach)] + [0] * (k - reach)
    assert not rec.any() and gap[0, 0] == min(32, g + k) and last[0, 0] == -1
    lost = _lost(12, range(2, 5))                        # the middle chunk of (2, 3, 7)
    _, _, rec, across = _same_plan(lost, (2, 3, 7), 8)
    assert rec[0, :, 0].tolist() == [True] + [False] * 4 + [True] + [False] * 7 and across[0, 5, 0]


def test_plan_chunks_of_one_row():
    rng = np.random.default_rng(3)
    lost = (rng.random((2, 12, 2)) < 0.5).astype(np.uint8)
    for max_age in AGES:
        _, _, rec, across = _same_plan(lost, (1,) * 12, max_age)
        assert np.array_equal(across[:, 1:], rec[:, 1:])             # every recovery crosses a boundary
    src, age, rec, gap, last = np_recover_chunk_plan(_lost(1, []), np.array([[3]]), 8)
    assert (src[0, 0, 0], age[0, 0, 0], bool(rec[0, 0, 0]), gap[0, 0], last[0, 0]) == (0, 0, True, 0, 0)
    src, age, rec, gap, last = np_recover_chunk_plan(_lost(1, [0]), np.array([[3]]), 8)
    assert (src[0, 0, 0], age[0, 0, 0], bool(rec[0, 0, 0]), gap[0, 0], last[0, 0]) == (CARRIED, 3, False, 4, -1)


def test_plan_a_fresh_stream():
    """Row 0 arrived: the frame in front is recovered from slot 0 (on protected slots: the zero bytes of f = 0); row 0 lost
    too: silence."""
    fresh = np_fresh_gap(1, 1)
    src, age, rec, gap, last = np_recover_chunk_plan(_lost(3, []), fresh, 8)
    assert src[0, :, 0].tolist() == [0, 0, 1] and rec[0, :, 0].tolist() == [True, False, False] and gap[0, 0] == 0
    src, age, rec, gap, last = np_recover_chunk_plan(_lost(3, [0]), fresh, 8)
    assert src[0, :, 0].tolist() == [-1, 1, 1] and rec[0, :, 0].tolist() == [False, True, False] and not age.any()
    src, age, rec, gap, last = np_recover_chunk_plan(_lost(3, [0, 1, 2]), fresh, 31)
    assert (src == -1).all() and gap[0, 0] == 32 and last[0, 0] == -1


def test_plan_the_flush():
    """The flush is a chunk of one lost row: D is concealed where it was lost, never recovered."""
    for lost, want_src, want_age in ((_lost(5, []), 5, 0), (_lost(5, [4]), 4, 1), (_lost(5, [3, 4]), 3, 2), (_lost(5, range(5)), -1, 0)):
        src, age, rec, _ = _same_plan(lost, (2, 3), 8)
        assert src.shape == (1, 6, 1) and (src[0, 5, 0], age[0, 5, 0], bool(rec[0, 5, 0])) == (want_src, want_age, False)
    src, age, rec, _ = np_recover_stream_plan(_lost(5, [3, 4]), (2, 3), (8, 8), flush_age=1)       # the flush's own max_age
    assert src[0, 5, 0] == -1 and src[0, 4, 0] == 3


@pytest.mark.parametrize("seed", range(6))
def test_plan_random_patterns_chunked_equal_the_one_shot_plan(seed):
    rng = np.random.default_rng(seed)
    B, C, F = 2, 2, int(rng.integers(20, 70))
    lost = (rng.random((B, F, C)) < rng.choice([0.3, 0.7, 0.95])).astype(np.uint8)
    for max_age in AGES + (5,):
        for _ in range(4):
            cuts = np.sort(rng.choice(np.arange(1, F), size=int(rng.integers(0, 6)), replace=False))
            _same_plan(lost, tuple(int(v) for v in np.diff(np.concatenate(([0], cuts, [F])))), max_age)


# ---- CPU: the ABI surface and the argument errors -----------------------------------------------------------------------------
def _struct(text, name):
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S)
    assert m, "%s is not declared" % name
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    return [" ".join(f.split()) for f in body.split(";") if f.strip()]


def test_header_and_ctypes_mirror_of_the_recovering_chunk():
    text = open(HEADER).read()
    assert _struct(text, "ac_stream_packed_recover_in") == ["ac_stream_packed_in in", "const uint8_t* lost", "int32_t max_age",
                                                            "int64_t redundant_at"]
    assert _struct(text, "ac_stream_packed_recover_in")[:3] == _struct(text, "ac_stream_packed_lost_in")
    P, L = _lib.StreamPackedRecoverIn, _lib.StreamPackedLostIn
    assert [f[0] for f in P._fields_] == ["inner", "lost", "max_age", "redundant_at"]
    assert (P.inner.offset, P.lost.offset, P.max_age.offset, P.redundant_at.offset) == (0, 40, 48, 56) and ctypes.sizeof(P) == 64
    assert (L.inner.offset, L.lost.offset, L.max_age.offset) == (P.inner.offset, P.lost.offset, P.max_age.offset)
    assert re.search(r"\benum\s*\{\s*AC_CONCEAL_REDUNDANT\s*=\s*256\s*\}", text) and _lib.AC_CONCEAL_REDUNDANT == 256
    assert re.search(r"#define\s+AC_VERSION\s+171\b", text)
    assert "ac_stream_packed_launches(s, psy, 3)" in text
    sig = inspect.signature(StreamingMDCT.decode_packed_chunk)
    assert list(sig.parameters)[:6] == ["self", "data", "index", "pcm16", "out", "stream"]
    for name, default in (("lost", None), ("max_age", 8), ("redundant_at", None)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default
    sig = inspect.signature(StreamingMDCT.flush_packed)
    assert list(sig.parameters) == ["self", "pcm16", "out", "stream", "max_age"]
    assert sig.parameters["max_age"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["max_age"].default == 8
    sig = inspect.signature(StreamingMDCT.packed_chunk_launches)
    assert sig.parameters["recover"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["recover"].default is False


def test_library_keeps_its_version_and_takes_the_query_value():
    lib = _lib.load()
    assert lib.ac_version() == 171
    assert lib.ac_stream_packed_launches(None, None, 3) == 0
    rows = _lib.StreamPackedRecoverIn(max_age=8 | _lib.AC_CONCEAL_REDUNDANT, redundant_at=172)
    assert lib.ac_stream_inverse_typed(None, ctypes.addressof(rows), None, _lib.AC_PACKED | _lib.AC_CONCEAL, 1, None) == _lib.AC_EINVAL
    assert b"stream is NULL" in lib.ac_last_error()


def _stub(delayed=False, advanced=False):
    """A StreamingMDCT without a device: what the argument and mode checks read before anything touches the library."""
    st = object.__new__(StreamingMDCT)
    st.mdct = types.SimpleNamespace(compute_dtype=torch.float32, filters_n=N0)
    st.psy = types.SimpleNamespace(_check_redundant_at=audiocodec_amd.PsychoacousticModel._check_redundant_at)
    st._handle, st._delayed, st._advanced = None, delayed, advanced
    return st


def test_argument_and_mode_errors_come_before_any_work():
    st = _stub()
    with pytest.raises(ValueError, match="redundant_at without lost"):
        st.decode_packed_chunk(None, None, redundant_at=172)
    for bad in (0, -4, 2 ** 31):
        with pytest.raises(ValueError, match="redundant_at"):
            st.decode_packed_chunk(None, None, lost=object(), redundant_at=bad)
    for bad in (172.0, True, "172"):
        with pytest.raises(TypeError, match="redundant_at"):
            st.decode_packed_chunk(None, None, lost=object(), redundant_at=bad)
    with pytest.raises(ValueError, match="decode=True, conceal=True"):
        st.packed_chunk_launches(decode=True, recover=True)
    st = _stub(delayed=True)
    with pytest.raises(ValueError, match="inverse_chunk on a stream that decodes recovering chunks"):
        st.inverse_chunk(None)
    with pytest.raises(ValueError, match="run on a stream that decodes recovering chunks"):
        st.run(None, 4)
    assert st._delayed and not st._advanced


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _env:
    """name=1 around a block (the library reads the switches per call); what was there before comes back."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.before = os.environ.get(self.name)
        os.environ[self.name] = "1"

    def __exit__(self, *exc):
        if self.before is None:
            del os.environ[self.name]
        else:
            os.environ[self.name] = self.before
        return False


@functools.lru_cache(maxsize=None)
def _tonal(C, K):
    """fused_layouts.tonal's recipe on K blocks, float32 [3, K N0, C] (K = 5: that signal): ramped noise; four sinusoids over a
    noise floor; a quiet ramped noise with a decaying harmonic comb in its last channel."""
    S = K * N0
    rng = np.random.default_rng(4242 + C)
    n = np.arange(S, dtype=np.float64)
    x = np.zeros((3, S, C))
    x[0] = rng.uniform(-1, 1, (S, C)) * np.linspace(0.01, 1, S)[:, None]
    x[1] = 1e-4 * rng.uniform(-1, 1, (S, C))
    for c in range(C):
        for k, a in ((40.5, 0.3), (200.5, 0.25), (520.5, 0.2), (900.5, 0.25)):
            x[1, :, c] += a * np.sin(np.pi * k / N0 * n + 0.7 * c + k)
    x[2] = 0.01 * rng.uniform(-1, 1, (S, C)) * np.linspace(0.01, 1, S)[:, None]
    x[2, :, C - 1] = sum(0.5 / h * np.sin(np.pi * 7.5 * h / N0 * n + h) for h in range(1, 120))
    x /= max(1.0, np.abs(x).max())
    return x.astype(np.float32)


def test_the_tonal_recipe_is_fused_layouts_tonal_at_its_length():
    import fused_layouts as fl
    for C in (1, 2):
        assert np.array_equal(_tonal(C, fl.K0), fl.tonal(C))


@functools.lru_cache(maxsize=None)
def _slots(signal, C, Kp):
    """Protected slots [3, Kp, C] whose copies carry content: R = R2 = 1365 on rows encoded at 2730 bits.  Returns the codec of
    the slots, data, index and the numpy copies of the two."""
    import protect_layouts as pl
    base = audiocodec_amd.AudioCodec(48000, N0)
    dst = base.with_row_budget(1365)
    x = pl.slots_noise(C, Kp) if signal == "noise" else _tonal(C, Kp - 1)
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(_dev(x))
    data, index = dst.protect_packed_rows(data, index, 1365)[:2]
    assert tuple(index.shape) == (3, Kp, C)
    return dst, data, index, data.cpu().numpy(), index.cpu().numpy()


def _extended(index, lost):
    """The front-extended index and lost of the one-shot yardstick."""
    return torch.cat((index[:, :1], index), dim=1).contiguous(), torch.cat((torch.ones_like(lost[:, :1]), lost), dim=1).contiguous()


def _one_shot(codec, data, index, lost, pcm16, max_age, o):
    """Blocks [0, K'] of the parent's one-shot recovering decode on the front-extended signal."""
    ie, le = _extended(index, lost)
    return codec.decode_packed(data, ie, pcm16, lost=le, max_age=max_age, redundant_at=o)[:, :(index.shape[1] + 1) * codec.filters_n]


def _run(st, data, index, lost, splits, ages, pcm16, o, flush_age=None):
    """The recovering chunks of one split and the flush on stream object `st`: [B, (K' + 1) N, C] where one format is asked for,
    else the list of the calls' outputs.  pcm16 and ages: one value, or one per call (the flush last)."""
    n = len(splits) + 1
    ages = (ages,) * n if isinstance(ages, int) else tuple(ages)
    fmts = (pcm16,) * n if isinstance(pcm16, bool) else tuple(pcm16)
    N = st.mdct.filters_n
    outs = []
    for (a, b), m, p in zip(_bounds(splits), ages, fmts):
        outs.append(st.decode_packed_chunk(data, index[:, a:b].contiguous(), p, lost=lost[:, a:b].contiguous(), max_age=m,
                                           redundant_at=o))
        assert outs[-1].dtype == (torch.int16 if p else torch.float32) and outs[-1].shape == (index.shape[0], (b - a) * N, index.shape[2])
    outs.append(st.flush_packed(fmts[-1], max_age=ages[-1]))
    assert outs[-1].shape == (index.shape[0], N, index.shape[2]) and not st._delayed
    return torch.cat(outs, dim=1) if isinstance(pcm16, bool) else outs


def _patterns(B, Kp, C, max_age, splits):
    """test_protect._patterns, and the boundary patterns of the CPU tests laid on this split's boundaries."""
    from test_protect import _patterns as one_shot_patterns
    out = dict(one_shot_patterns(B, Kp, C, max_age))
    cuts = [a for a, _ in _bounds(splits)[1:]] or [Kp // 2]
    z = lambda: np.zeros((B, Kp, C), dtype=np.uint8)             # noqa: E731
    ends, both = z(), z()
    for p in cuts:
        ends[:, p - 1] = 1                                       # the last row of a chunk lost, the next first row arrived
        both[:, p - 1:p + 1] = 1                                 # ... and the next first row lost too
    out["last rows of the chunks"], out["last and first rows of the chunks"] = ends, both
    for name, n in (("max_age", max_age + 1), ("max_age + 1", max_age + 2)):
        runs = z()
        for b in range(B):
            for c in range(C):
                p = cuts[(b + c) % len(cuts)]
                runs[b, max(p - 1, 0):max(p - 1, 0) + n, c] = 1
        out["a run across the boundary, " + name] = runs
    if len(splits) >= 3:
        whole = z()
        a, b = _bounds(splits)[len(splits) // 2]
        whole[:, a:b] = 1
        out["a whole chunk"] = whole
    first = z()
    first[:, 0] = 1
    first[B - 1, 0, C - 1] = 0
    out["row 0 of a fresh stream"] = first
    return out


@functools.lru_cache(maxsize=None)
def _hold_the_bytes(signal, C, Kp, splits):
    """numpy's reading, before any kernel result: the copies the patterns recover carry content (hold_conditions, on the
    front-extended signal the one-shot yardstick decodes; "tonal" only, see the top of the file), and in a split of several
    chunks some frame is recovered across a chunk boundary from a copy that holds a non-zero code."""
    import protect_layouts as pl
    codec, _, _, data, index = _slots(signal, C, Kp)
    o, off = codec.row_bytes, codec.psy.scale_band_offsets
    index_ext = np.concatenate((index[:, :1], index), axis=1)
    pats = lambda max_age: {k: front_extended(v) for k, v in _patterns(3, Kp, C, max_age, splits).items()}   # noqa: E731
    if signal == "tonal":
        pl.hold_conditions(data, index_ext, o, off, pats, (signal, C, Kp, splits))
    if len(splits) > 1:
        codes, _, _ = pl.copies(data, index_ext, o, off)
        nonzero = (codes != 0).any(axis=2)                        # [B, K' + 1, C]: the copy of extended frame e
        n = 0
        for max_age in pl.AGES:
            for lost in _patterns(3, Kp, C, max_age, splits).values():
                across = _same_plan(lost, splits, max_age)[3]
                n += int((across & nonzero).sum())
        assert n >= 1, "no frame is recovered across a boundary of %s from a copy with a non-zero code" % (splits,)


@gpu
@pytest.mark.parametrize("pcm16", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("Kp,splits", SPLITS, ids=SPLIT_IDS)
@pytest.mark.parametrize("C", [1, 2])
def test_recovering_chunks_equal_the_one_shot_call(C, Kp, splits, pcm16, monkeypatch):
    """B = 3.  Every pattern at every max_age: the kernel's chunks and flush, and the composition's on a second stream, against
    blocks [0, K'] of the parent's one-shot call on the front-extended signal; the numpy plan of the split against the
    one-shot numpy plan."""
    monkeypatch.delenv(NOFUSE, raising=False)
    _hold_the_bytes("tonal", C, Kp, splits)
    codec, data, index, _, _ = _slots("tonal", C, Kp)
    o = codec.row_bytes
    fused, comp = codec.stream(3, C), codec.stream(3, C)
    assert fused.packed_chunk_launches(decode=True, conceal=True, recover=True) == 1
    recovered = 0
    for max_age in AGES:
        for name, lost in _patterns(3, Kp, C, max_age, splits).items():
            recovered += int(_same_plan(lost, splits, max_age)[3].sum())
            lost_d = _dev(lost)
            ref = _one_shot(codec, data, index, lost_d, pcm16, max_age, o)
            got = _run(fused, data, index, lost_d, splits, max_age, pcm16, o)
            assert same_bits(got, ref), "kernel != one-shot: %s max_age=%d" % (name, max_age)
            with _env(NOFUSE):
                assert comp.packed_chunk_launches(decode=True, conceal=True, recover=True) == 3
                other = _run(comp, data, index, lost_d, splits, max_age, pcm16, o)
            assert same_bits(other, ref), "composition != one-shot: %s max_age=%d" % (name, max_age)
            if name == "all":      # +0 everywhere: not -0, not NaN
                assert int((got.view(torch.int16 if pcm16 else torch.int32) != 0).sum()) == 0
    assert recovered > 0 or len(splits) == 1


@gpu
@pytest.mark.parametrize("C", [1, 2])
def test_recovering_chunks_on_noise_slots(C, monkeypatch):
    """protect_layouts.slots_noise, seven rows as (3, 4) and (1,) * 7: many narrow bands in every copy."""
    monkeypatch.delenv(NOFUSE, raising=False)
    for splits in ((3, 4), (1,) * 7):
        _hold_the_bytes("noise", C, 7, splits)
        codec, data, index, _, _ = _slots("noise", C, 7)
        o = codec.row_bytes
        fused, comp = codec.stream(3, C), codec.stream(3, C)
        for max_age in (1, 8):
            for name, lost in _patterns(3, 7, C, max_age, splits).items():
                lost_d = _dev(lost)
                for pcm16 in (False, True):
                    ref = _one_shot(codec, data, index, lost_d, pcm16, max_age, o)
                    assert same_bits(_run(fused, data, index, lost_d, splits, max_age, pcm16, o), ref), (name, max_age, pcm16, splits)
                    with _env(NOFUSE):
                        assert same_bits(_run(comp, data, index, lost_d, splits, max_age, pcm16, o), ref), (name, max_age, pcm16, splits)


@gpu
@pytest.mark.parametrize("C", [1, 2])
def test_nothing_lost_is_the_plain_stream_one_block_late(C, monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, data, index, _, _ = _slots("noise", C, 12)
    none = torch.zeros((3, 12, C), dtype=torch.uint8, device="cuda")
    for pcm16 in (False, True):
        plain = codec.stream(3, C)
        want = torch.cat([plain.decode_packed_chunk(data, index[:, a:b].contiguous(), pcm16) for a, b in _bounds((5, 7))], dim=1)
        got = _run(codec.stream(3, C), data, index, none, (5, 7), 8, pcm16, codec.row_bytes)
        assert int((got[:, :N0] != 0).sum()) == 0                 # the zero bytes of slot 0's copy: silence
        assert same_bits(got[:, N0:], want)


@gpu
@pytest.mark.parametrize("C,B,K", [(2, 64, 64), (1, 129, 96)])
def test_recovering_chunks_across_strips(C, B, K, monkeypatch):
    """The strip-crossing shapes of test_protect: the successor lies in another wave's strip, another workgroup's.  Two chunks."""
    monkeypatch.delenv(NOFUSE, raising=False)
    base = audiocodec_amd.AudioCodec(48000, N0)
    codec = base.with_row_budget(1365)
    g = torch.Generator("cuda").manual_seed(B + K)
    x = (torch.rand((B, K * N0, C), device="cuda", generator=g) * 2 - 1) * torch.linspace(0.01, 1, K * N0, device="cuda")[None, :, None]
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(x)
    data, index = codec.protect_packed_rows(data, index, 1365)[:2]
    o, Kp = codec.row_bytes, K + 1
    lost = (torch.rand((B, Kp, C), device="cuda", generator=g) < 0.3).view(torch.uint8)
    lost[0, 5:40] = 1
    lost[1, 11:20] = 1
    lost[2, 12] = 1                                               # the last row of chunk 1, recovered from chunk 2's first slot
    lost[2, 13] = 0
    st = codec.stream(B, C)
    assert st.packed_chunk_launches(decode=True, conceal=True, recover=True) == 1
    for max_age, pcm16 in ((8, False), (31, True)):
        got = _run(st, data, index, lost, (13, Kp - 13), max_age, pcm16, o)
        assert same_bits(got, _one_shot(codec, data, index, lost, pcm16, max_age, o)), (max_age, pcm16)
    single = torch.zeros_like(lost)                               # every third row lost: all recovered
    single[:, 0:K:3] = 1
    got = _run(st, data, index, single, (13, Kp - 13), 8, False, o)
    assert same_bits(got, _one_shot(codec, data, index, single, False, 8, o))
    ie, le = _extended(index, single)
    assert not same_bits(got, codec.decode_packed(data, ie, lost=le, max_age=8)[:, :(Kp + 1) * N0])


@gpu
def test_redundant_at_off_the_phase_and_past_the_end(monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, data, index, _, _ = _slots("noise", 2, 12)
    rb = codec.row_bytes
    from test_protect import _patterns as one_shot_patterns
    lost = one_shot_patterns(3, 12, 2, 8)["30 %"]
    lost[0, 4, 0], lost[0, 5, 0] = 1, 0                           # recovered across the boundary of (5, 7)
    lost[0, 10, 0], lost[0, 11, 0] = 1, 0                         # a recovered row whose copy is in the last slot
    lost_d = _dev(lost)
    fused, comp = codec.stream(3, 2), codec.stream(3, 2)

    def hold(d, o, what):
        ref = _one_shot(codec, d, index, lost_d, False, 8, o)
        assert same_bits(_run(fused, d, index, lost_d, (5, 7), 8, False, o), ref), what
        with _env(NOFUSE):
            assert same_bits(_run(comp, d, index, lost_d, (5, 7), 8, False, o), ref), what
        return ref
    # off the 4-byte phase: the bytes shifted by 3, the primary rows still read from their aligned copies in front
    shifted = torch.cat([data, torch.zeros(3, dtype=torch.uint8, device="cuda"), data])
    a = hold(shifted, rb + data.numel() + 3, "off the phase")
    assert same_bits(a, hold(data, rb, "aligned"))
    # so large that the last rows' copies start past nbytes (silence), and any odd value
    for o in (data.numel() - int(index[0, 11, 0]) - 5, data.numel(), 2 ** 31 - 1, 1, rb + 2):
        hold(data, o, "redundant_at %d" % o)


@gpu
@pytest.mark.parametrize("C", [1, 2])
def test_a_different_max_age_and_output_per_chunk(C, monkeypatch):
    """A frame takes the max_age and the format of the call that synthesises it.  The kernel against the composition in every
    block; against the one-shot call of the chunk's own max_age and format in every block but a chunk's first, which also
    holds the aliased half of a frame the call before synthesised."""
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, data, index, _, _ = _slots("noise", C, 12)
    o = codec.row_bytes
    splits, ages, pcm = (2, 3, 3, 4), (1, 8, 0, 31, 2), (False, True, True, False, True)
    lost = np.zeros((3, 12, C), dtype=np.uint8)
    lost[:, 1:11] = 1
    lost[1, 6, C - 1] = 0
    lost_d = _dev(lost)
    got = _run(codec.stream(3, C), data, index, lost_d, splits, ages, pcm, o)
    with _env(NOFUSE):
        other = _run(codec.stream(3, C), data, index, lost_d, splits, ages, pcm, o)
    for i, ((a, b), m, p) in enumerate(zip(_bounds(splits) + [(12, 13)], ages, pcm)):
        assert same_bits(got[i], other[i]), "kernel != composition, call %d" % i
        ref = _one_shot(codec, data, index, lost_d, p, m, o)
        assert same_bits(got[i][:, N0:], ref[:, (a + 1) * N0:b * N0]), "kernel != one-shot, call %d" % i
    assert int((got[1] != 0).sum()) > 0


@gpu
@pytest.mark.parametrize("nofuse", [False, True], ids=["one launch", "composition"])
def test_mode_errors_leave_the_state_untouched(nofuse, monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, data, index, _, _ = _slots("noise", 2, 12)
    o = codec.row_bytes
    from test_protect import _patterns as one_shot_patterns
    lost = _dev(one_shot_patterns(3, 12, 2, 8)["30 %"])
    ref = _one_shot(codec, data, index, lost, False, 8, o)
    plain = codec.decode_packed(data, index)[:, :12 * N0]
    if nofuse:
        monkeypatch.setenv(NOFUSE, "1")
    st = codec.stream(3, 2)
    assert st.packed_chunk_launches(decode=True, conceal=True, recover=True) == (3 if nofuse else 1)
    idx1, idx2, l1, l2 = index[:, :5].contiguous(), index[:, 5:].contiguous(), lost[:, :5].contiguous(), lost[:, 5:].contiguous()
    first = st.decode_packed_chunk(data, idx1, lost=l1, max_age=8, redundant_at=o)
    X = codec.psy.dequantize(*codec.psy.unpack(data, idx2))
    for call in (lambda: st.inverse_chunk(X), lambda: st.decode_packed_chunk(data, idx2), lambda: st.decode_packed_chunk(data, idx2, lost=l2),
                 lambda: st.run([torch.zeros((3, 4 * N0, 2), device="cuda")], 4)):
        with pytest.raises(ValueError, match="recovering chunks"):
            call()
    with pytest.raises(ValueError, match="redundant_at without lost"):
        st.decode_packed_chunk(data, idx2, redundant_at=o)
    with pytest.raises(ValueError, match="max_age"):
        st.decode_packed_chunk(data, idx2, lost=l2, max_age=32, redundant_at=o)
    assert same_bits(st.decode_packed_chunk(data, index[:, :0].contiguous(), lost=lost[:, :0].contiguous(), redundant_at=o),
                     torch.empty((3, 0, 2), device="cuda"))       # k = 0 changes nothing
    rest = torch.cat((st.decode_packed_chunk(data, idx2, lost=l2, max_age=8, redundant_at=o), st.flush_packed()), dim=1)
    assert same_bits(torch.cat((first, rest), dim=1), ref)
    # after the flush the stream is fresh: the plain calls serve again, and then a recovering chunk is refused
    a = st.decode_packed_chunk(data, idx1)
    with pytest.raises(ValueError, match="has advanced without it"):
        st.decode_packed_chunk(data, idx2, lost=l2, max_age=8, redundant_at=o)
    with pytest.raises(ValueError, match="has advanced without it"):
        st.flush_packed()
    assert same_bits(torch.cat((a, st.decode_packed_chunk(data, idx2)), dim=1), plain)
    st.reset()
    assert same_bits(_run(st, data, index, lost, (5, 7), 8, False, o), ref)


@gpu
@pytest.mark.parametrize("N,C,nofuse", [(512, 3, False), (1024, 2, True)])
def test_where_the_one_launch_is_not_served(N, C, nofuse, monkeypatch):
    """filters_n = 512 with three channels, and filters_n = 1024 behind the switch: the composition, equal to the one-shot
    composition."""
    monkeypatch.delenv(NOFUSE, raising=False)
    from test_encode_quantized_fused import _pcm
    base = audiocodec_amd.AudioCodec(48000, N)
    codec = base.with_row_budget(1365)
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(_pcm(N, C, 2, 11, seed=N + C, inject=False))
    data, index = codec.protect_packed_rows(data, index, 1365)[:2]
    if nofuse:
        monkeypatch.setenv(NOFUSE, "1")
    st = codec.stream(2, C)
    assert st.packed_chunk_launches(decode=True, conceal=True, recover=True) == 3 and codec.decode_packed_launches(C) != 1
    o = codec.row_bytes
    for max_age in (0, 2, 31):
        for splits in ((5, 7), (2, 3, 7), (1,) * 12):
            for name, lost in _patterns(2, 12, C, max_age, splits).items():
                lost_d = _dev(lost)
                ie, le = _extended(index, lost_d)
                ref = codec.decode_packed(data, ie, lost=le, max_age=max_age, redundant_at=o)[:, :13 * N]
                assert same_bits(_run(st, data, index, lost_d, splits, max_age, False, o), ref), (name, max_age, splits)


@gpu
def test_recovering_chunk_c_abi(monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    lib = _lib.load()
    codec, data, index, _, _ = _slots("noise", 2, 12)
    from test_protect import _patterns as one_shot_patterns
    lost = _dev(one_shot_patterns(3, 12, 2, 8)["two runs"])
    lost[:, 4], lost[:, 5] = 1, 0
    RED, o = _lib.AC_CONCEAL_REDUNDANT, codec.row_bytes
    ref = _one_shot(codec, data, index, lost, False, 8, o)
    psy = codec.psy._plan(data.device)
    dtype = _lib.AC_PACKED | _lib.AC_CONCEAL
    idx1, idx2, l1, l2 = index[:, :5].contiguous(), index[:, 5:].contiguous(), lost[:, :5].contiguous(), lost[:, 5:].contiguous()
    st = codec.stream(3, 2)
    out = torch.full((3, 7 * N0, 2), 7.0, device="cuda")

    def call(idx, lost_ptr, max_age, at, k, x=None, struct=_lib.StreamPackedRecoverIn):
        inner = _lib.StreamPackedIn(_lib.PackedRows(data.data_ptr(), data.numel(), idx.data_ptr()), psy.value, 0)
        rows = struct(inner, lost_ptr, max_age, at) if struct is _lib.StreamPackedRecoverIn else struct(inner, lost_ptr, max_age)
        status = lib.ac_stream_inverse_typed(st._handle, ctypes.addressof(rows), ctypes.c_void_p((out if x is None else x).data_ptr()),
                                             dtype, k, None)
        torch.cuda.synchronize()
        return status
    assert lib.ac_stream_packed_launches(st._handle, psy, 3) == 1
    first = torch.empty((3, 5 * N0, 2), device="cuda")
    assert call(idx1, l1.data_ptr(), 8 | RED, o, 5, first) == _lib.AC_OK, lib.ac_last_error()
    for bad_age, bad_at in ((32 | RED, o), (255 | RED, o), (8 | RED, 0), (8 | RED, 2 ** 31), (8 | RED, -4)):
        assert call(idx2, l2.data_ptr(), bad_age, bad_at, 7) == _lib.AC_EINVAL and lib.ac_last_error(), (bad_age, bad_at)
    assert call(idx2, None, 8 | RED, o, 7) == _lib.AC_EINVAL and b"lost is NULL" in lib.ac_last_error()
    # the stream is delayed: the concealing chunk without the bit, the plain chunk and ac_stream_inverse are refused
    assert call(idx2, l2.data_ptr(), 8, o, 7) == _lib.AC_EINVAL and b"one frame behind" in lib.ac_last_error()
    assert call(idx2, l2.data_ptr(), 8, 0, 7, struct=_lib.StreamPackedLostIn) == _lib.AC_EINVAL
    inner = _lib.StreamPackedIn(_lib.PackedRows(data.data_ptr(), data.numel(), idx2.data_ptr()), psy.value, 0)
    assert lib.ac_stream_inverse_typed(st._handle, ctypes.addressof(inner), ctypes.c_void_p(out.data_ptr()), _lib.AC_PACKED, 7, None) == _lib.AC_EINVAL
    X = torch.zeros((3, 7, N0, 2), device="cuda")
    assert lib.ac_stream_inverse(st._handle, ctypes.c_void_p(X.data_ptr()), ctypes.c_void_p(out.data_ptr()), 7, None) == _lib.AC_EINVAL
    assert b"ac_stream_inverse on a stream that decodes recovering chunks" in lib.ac_last_error()
    with _env(NOFUSE):
        assert lib.ac_stream_packed_launches(st._handle, psy, 3) == 3
        assert call(idx2, l2.data_ptr(), 8 | RED, o, 7) == _lib.AC_EUNSUPPORTED and b"ac_unpack" in lib.ac_last_error()
    assert call(idx2, l2.data_ptr(), 8 | RED, o, 0) == _lib.AC_OK                # k = 0
    assert int((out != 7.0).sum()) == 0                                         # the refused calls wrote nothing
    # ... and left the state: the rest of the signal, and the flush as a chunk of one lost row
    assert call(idx2, l2.data_ptr(), 8 | RED, o, 7) == _lib.AC_OK, lib.ac_last_error()
    one, last = torch.ones((3, 1, 2), dtype=torch.uint8, device="cuda"), torch.empty((3, N0, 2), device="cuda")
    assert call(idx2, one.data_ptr(), 8 | RED, 1, 1, last) == _lib.AC_OK
    assert same_bits(torch.cat((first, out, last), dim=1), ref)
    # a stream whose synthesis has advanced without the bit refuses it until it is reset
    assert lib.ac_stream_reset(st._handle, None) == _lib.AC_OK
    assert call(idx1, l1.data_ptr(), 8, 0, 5, first, struct=_lib.StreamPackedLostIn) == _lib.AC_OK
    assert call(idx2, l2.data_ptr(), 8 | RED, o, 7) == _lib.AC_EINVAL and b"ac_stream_reset" in lib.ac_last_error()
    assert lib.ac_stream_reset(st._handle, None) == _lib.AC_OK
    assert call(idx1, l1.data_ptr(), 8 | RED, o, 5, out[:, :5 * N0].contiguous()) == _lib.AC_OK
    st.reset()


@pytest.fixture(scope="module")
def harness():
    assert torch.cuda.is_available(), "the stream contract is checked on the GPU"
    return Harness()


@gpu
@pytest.mark.parametrize("pcm16", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("nofuse", [False, True], ids=["one launch", "composition"])
def test_the_recovering_chunk_and_the_flush_only_enqueue(nofuse, pcm16, harness, monkeypatch):
    """decode_packed_chunk with redundant_at and flush_packed keep to their stream and do not wait for the device
    (tests/stream_order.py): two chunks and the flush after a reset, so that every run starts from the same state."""
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, data, index, _, _ = _slots("noise", 2, 12)
    o = codec.row_bytes
    lost = _dev((np.random.default_rng(2).random((3, 12, 2)) < 0.3).astype(np.uint8))
    lost[:, 4], lost[:, 5] = 1, 0
    ref0 = _one_shot(codec, data, index, lost, pcm16, 8, o)
    if nofuse:
        monkeypatch.setenv(NOFUSE, "1")
    st = codec.stream(3, 2)
    assert st.packed_chunk_launches(decode=True, conceal=True, recover=True) == (3 if nofuse else 1)

    def two_chunks(data, index, lost):
        st.reset()
        a = st.decode_packed_chunk(data, index[:, :5].contiguous(), pcm16, lost=lost[:, :5].contiguous(), max_age=8, redundant_at=o)
        b = st.decode_packed_chunk(data, index[:, 5:].contiguous(), pcm16, lost=lost[:, 5:].contiguous(), max_age=8, redundant_at=o)
        return a, b

    def chunk_and_flush(data, index, lost):
        st.reset()
        return st.decode_packed_chunk(data, index, pcm16, lost=lost, max_age=8, redundant_at=o), st.flush_packed(pcm16)
    what = "%s,%s" % ("pcm16" if pcm16 else "f32", "composition" if nofuse else "one launch")

    def one_chunk(data, index, lost):
        st.reset()
        return st.decode_packed_chunk(data, index, pcm16, lost=lost, max_age=8, redundant_at=o)

    def flush_alone(data, index, lost):
        st.reset()
        return st.flush_packed(pcm16)
    # the composition is some forty torch calls, about a millisecond of host time each way (measured: 2.2 to 2.4 ms for two):
    # its cases hold one composed call each, so that the harness's delay keeps its margin of 20 calls on a slower host
    cases = ((("decode_packed_chunk[redundant_at,%s]" % what, one_chunk, 12), ("flush_packed[%s]" % what, flush_alone, 0)) if nofuse
             else (("decode_packed_chunk[redundant_at,%s]" % what, two_chunks, 12), ("flush_packed[%s]" % what, chunk_and_flush, 13)))
    for name, fn, blocks in cases:
        case = ((data, index, lost), fn)
        ref = harness.reference(case)
        if blocks:
            assert same_bits(torch.cat(ref, dim=1), ref0[:, :blocks * N0])
        else:
            assert int((ref[0] != 0).sum()) == 0                  # the flush of a fresh stream: silence
        harness.delayed_producer(name, case, ref)
        harness.busy_default(name, case, ref)
        print("%s: the warmed call took %.2f ms, host entry to completion" % (name, harness.call_s[name] * 1e3))
    ref = harness.reference(((data, index, lost), two_chunks)) + harness.reference(((data, index, lost), chunk_and_flush))[1:]
    # out= and stream=: the same bits, written where the caller said
    side = harness.fresh()
    out, end = torch.empty_like(ref[0]), torch.empty_like(ref[2])
    st.reset()
    torch.cuda.synchronize()
    got = st.decode_packed_chunk(data, index[:, :5].contiguous(), pcm16, out=out, stream=side, lost=lost[:, :5].contiguous(), redundant_at=o)
    st.decode_packed_chunk(data, index[:, 5:].contiguous(), pcm16, stream=side, lost=lost[:, 5:].contiguous(), redundant_at=o)
    assert st.flush_packed(pcm16, out=end, stream=side) is end
    side.synchronize()
    assert got is out and same_bits(out, ref[0]) and same_bits(end, ref[2])


# ---- protect chunk by chunk (k_protect_ps) ---------------------------------------------------------------------------------
PROTECT_NOFUSE = "AC_PROTECT_NOFUSE"
NAMES = ("data", "index", "fits", "red_fits", "offset", "red_offset")


def test_np_protect_chunks_equal_np_protect_on_the_whole_signal():
    """The definition in numpy: for any split the chunks, with the carried copy in frame 0, are np_protect's slots, flags and
    offsets on all rows."""
    import fused_layouts as fl
    from pack_reference import np_pack
    from protect_reference import np_protect
    off = fl.host_offsets(48000)
    rng = np.random.default_rng(11)
    codes = (rng.integers(-40, 41, (2, 5, N0, 2)) * (rng.random((2, 5, N0, 2)) < 0.2)).astype(np.int16)
    sf = rng.integers(-20, 20, (2, 5, 64, 2)).astype(np.int8)
    data, index = np_pack(codes, sf, off)
    for R, R2 in ((1365, 341), (1365, 1365)):
        whole = np_protect(data, index, off, N0, R, R2)
        want = (whole[0].reshape(2, 5, 2, -1),) + tuple(whole[2:])
        assert int(np.asarray(whole[5]).max()) > 0                    # some copy was requantised
        for splits in ((5,), (2, 3), (1,) * 5, (4, 0, 1)):
            got = np_protect_chunks(data, index, off, N0, R, R2, splits)
            for g, w, name in zip(got, want, ("slots", "fits", "red_fits", "offset", "red_offset")):
                assert np.array_equal(g, w), (name, splits, R2)


def test_header_and_ctypes_mirror_of_the_protect_carry():
    text = open(HEADER).read()
    assert _struct(text, "ac_protect_carry") == ["const uint8_t* row_in", "const uint8_t* fits_in", "const int16_t* offset_in",
                                                 "uint8_t* row_out", "uint8_t* fits_out", "int16_t* offset_out"]
    P = _lib.ProtectCarry
    assert [f[0] for f in P._fields_] == ["row_in", "fits_in", "offset_in", "row_out", "fits_out", "offset_out"]
    assert ctypes.sizeof(P) == 48 and [getattr(P, f[0]).offset for f in P._fields_] == [0, 8, 16, 24, 32, 40]
    assert re.search(r"AC_EMIT_REDUNDANT\s*=\s*256\s*,\s*AC_EMIT_CARRY\s*=\s*512\s*\}", text) and _lib.AC_EMIT_CARRY == 512
    assert re.search(r"AC_API\s+int\s+ac_protect_chunk_launches\s*\(\s*const\s+ac_psy_plan\s*\*\s*psy\s*,\s*int\s+C\s*,\s*int\s+red_bits\s*\)", text)
    lib = _lib.load()
    assert lib.ac_protect_chunk_launches(None, 2, 341) == 0
    flags = _lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED | _lib.AC_EMIT_REDUNDANT | _lib.AC_EMIT_CARRY
    assert lib.ac_encode_fused_ex(None, None, None, None, None, None, 0.0, _lib.AC_EMIT_CARRY, None, None, 0, 1, 1, 1, None) == _lib.AC_EINVAL
    assert b"AC_EMIT_CARRY beside the three" in lib.ac_last_error()
    assert lib.ac_encode_fused_ex(None, None, None, None, None, None, 0.0, flags, None, None, 0, 1, 1, 1, None) == _lib.AC_EINVAL
    sig = inspect.signature(audiocodec_amd.AudioCodec.protect_stream)
    assert list(sig.parameters) == ["self", "batches_n", "channels_n", "red_bits", "device"]
    sig = inspect.signature(audiocodec_amd.ProtectStream.protect_chunk)
    assert list(sig.parameters) == ["self", "data", "index", "return_offset", "stream"]
    assert all(hasattr(audiocodec_amd.ProtectStream, m) for m in ("reset", "launches"))


def _cat_chunks(parts, B, C, sb):
    """The chunks' outputs put together along frames: (slots [B, F, C, sb], fits, red_fits[, offset, red_offset])."""
    slots = torch.cat([p[0].view(B, -1, C, sb) for p in parts], dim=1)
    return (slots,) + tuple(torch.cat([p[i] for p in parts], dim=1) for i in range(2, len(parts[0])))


def _protect_chunks(ps, data, index, splits, return_offset):
    ps.reset()
    parts = []
    for a, b in _bounds(splits):
        out = ps.protect_chunk(data, index[:, a:b].contiguous(), return_offset)
        sb = ps.codec.protected_slot_bytes(ps.red_bits)
        want = (torch.arange(index.shape[0] * (b - a) * index.shape[2], dtype=torch.int64, device="cuda") * sb).view(index.shape[0], b - a, -1)
        assert torch.equal(out[1], want) and len(out) == (6 if return_offset else 4)
        parts.append(out)
    return parts


def _hold_protect(codec, data, index, R2, splits, what):
    """The kernel's chunks, the composition's and the one-shot protect_packed_rows on all rows, byte for byte, with and without
    the offsets."""
    B, F, C = index.shape
    sb = codec.protected_slot_bytes(R2)
    whole = codec.protect_packed_rows(data, index, R2, True)
    want = (whole[0].view(B, F, C, sb),) + tuple(whole[2:])
    fused, comp = codec.protect_stream(B, C, R2), codec.protect_stream(B, C, R2)
    assert fused.launches() == 1 and codec.protect_packed_rows_launches(C, red_bits=R2) == 1
    for return_offset in (True, False):
        got = _cat_chunks(_protect_chunks(fused, data, index, splits, return_offset), B, C, sb)
        with _env(PROTECT_NOFUSE):
            assert comp.launches() != 1
            other = _cat_chunks(_protect_chunks(comp, data, index, splits, return_offset), B, C, sb)
        for g, o, w, name in zip(got, other, want, ("slots", "fits", "red_fits", "offset", "red_offset")):
            assert same_bits(o, w), "composition != one-shot: %s %s %s" % (name, what, splits)
            assert same_bits(g, w), "kernel != one-shot: %s %s %s" % (name, what, splits)
    return whole


PROTECT_SPLITS = ((12,), (1,) * 12, (5, 7), (2, 3, 7))


@gpu
@pytest.mark.parametrize("R2", [341, 1365, 2730])
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 3])
def test_protect_chunks_equal_the_one_shot_call(B, C, R2, monkeypatch):
    """Rows at 2730 bits to slots of R = 1365 with a copy at R2 (B C k is no multiple of the four waves of a workgroup in most
    chunks: tail waves), over the splits of the decode."""
    monkeypatch.delenv(PROTECT_NOFUSE, raising=False)
    from test_encode_quantized_fused import _pcm
    base = audiocodec_amd.AudioCodec(48000, N0)
    codec = base.with_row_budget(1365)
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(_pcm(N0, C, B, 11, seed=50 + B + C, inject=False))
    for splits in PROTECT_SPLITS:
        whole = _hold_protect(codec, data, index, R2, splits, (B, C, R2))
    assert int(whole[5].max()) > 0 or R2 >= 2730                    # copies were requantised (at 2730 bits they fit as they are)


@gpu
def test_protect_chunks_marked_saturating_and_dense_rows_reset_and_empty_chunks(monkeypatch):
    monkeypatch.delenv(PROTECT_NOFUSE, raising=False)
    from test_protect import _adversarial
    tight = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    _, _, adv, adv_index, _ = _adversarial()
    data, index = _dev(adv), _dev(adv_index)
    F = index.shape[1]
    for splits in ((1,) * F, (2, F - 2), (3, F - 3)):              # every row is the carried copy once: the marked and the saturating one
        whole = _hold_protect(tight, data, index, 320, splits, "adversarial")
    assert not bool(whole[3].all()) and int(whole[5].max()) >= 254  # a marked copy, a copy at the last offset
    # dense input: pack()'s rows
    base = audiocodec_amd.AudioCodec(48000, N0)
    from test_encode_quantized_fused import _pcm
    codes, sf = base.encode_quantized(_pcm(N0, 2, 3, 6, seed=9, inject=False))
    dense = base.psy.pack(codes, sf)
    codec = base.with_row_budget(1365)
    _hold_protect(codec, dense[0], dense[1], 341, (3, 4), "dense")
    # reset(): frame 0 takes the values of f = 0 again; k = 0 changes nothing
    ps = codec.protect_stream(3, 2, 341)
    idx1, idx2 = dense[1][:, :3].contiguous(), dense[1][:, 3:].contiguous()
    for nofuse in (False, True):
        if nofuse:
            monkeypatch.setenv(PROTECT_NOFUSE, "1")
        ps.reset()
        ps.protect_chunk(dense[0], idx1, True)
        empty = ps.protect_chunk(dense[0], dense[1][:, :0].contiguous(), True)
        assert empty[0].shape == (0,) and [tuple(t.shape) for t in empty[1:]] == [(3, 0, 2)] * 5
        carried = ps.protect_chunk(dense[0], idx2, True)
        ps.reset()
        fresh = ps.protect_chunk(dense[0], idx2, True)
        alone = codec.protect_packed_rows(dense[0], idx2, 341, True)
        whole = codec.protect_packed_rows(dense[0], dense[1], 341, True)
        sb = codec.protected_slot_bytes(341)
        for f, a, c, w in zip(fresh, alone, carried, whole):
            assert same_bits(f, a)
        assert same_bits(carried[0].view(3, 4, 2, sb), whole[0].view(3, 7, 2, sb)[:, 3:]) and same_bits(carried[5], whole[5][:, 3:])
        assert not same_bits(carried[5], fresh[5])                 # (a 341-bit copy of this noise is zero bytes: the offsets tell)
    with pytest.raises(ValueError, match="index must be"):
        ps.protect_chunk(dense[0], dense[1][:, :, :1].contiguous())
    with pytest.raises(ValueError, match="row budget"):
        base.protect_stream(3, 2, 341)


@gpu
def test_protect_chunk_c_abi(monkeypatch):
    monkeypatch.delenv(PROTECT_NOFUSE, raising=False)
    lib = _lib.load()
    codec, _, _, _, _ = _slots("noise", 2, 12)
    base = audiocodec_amd.AudioCodec(48000, N0)
    from test_encode_quantized_fused import _pcm
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(_pcm(N0, 2, 3, 11, seed=5, inject=False))
    dev, R2 = data.device, 341
    sb, rb, red = codec.protected_slot_bytes(R2), codec.row_bytes, (R2 + 31) // 32 * 4
    whole = codec.protect_packed_rows(data, index, R2, True)
    psy = codec.psy._plan(dev)
    assert lib.ac_protect_chunk_launches(psy, 2, R2) == 1 and lib.ac_protect_chunk_launches(psy, 2, 100) == 0
    halves = [(torch.zeros((3, 2, red), dtype=torch.uint8, device=dev), torch.zeros((3, 2), dtype=torch.uint8, device=dev),
               torch.zeros((3, 2), dtype=torch.int16, device=dev)) for _ in range(2)]
    flags = _lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED | _lib.AC_EMIT_REDUNDANT | _lib.AC_EMIT_CARRY

    def call(idx, carry, fl=flags):
        k = idx.shape[1]
        out = (torch.full((3 * k * 2 * sb,), 7, dtype=torch.uint8, device=dev), torch.zeros((3, k, 2), dtype=torch.uint8, device=dev),
               torch.zeros((3, k, 2), dtype=torch.uint8, device=dev), torch.zeros((3, k, 2), dtype=torch.int16, device=dev),
               torch.zeros((3, k, 2), dtype=torch.int16, device=dev))
        src = _lib.PackedRows(data.data_ptr(), data.numel(), idx.data_ptr())
        dst = _lib.ProtectedOut(out[0].data_ptr(), rb, out[1].data_ptr(), R2, out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr())
        st = lib.ac_encode_fused_ex(codec.mdct._plan(dev), psy, ctypes.addressof(src), None, None, None, 0.0, fl, ctypes.addressof(dst),
                                    ctypes.addressof(carry) if carry is not None else None, 0, 3, k - 1, 2, None)
        torch.cuda.synchronize()
        return st, out
    ptrs = lambda h: [t.data_ptr() for t in h]                    # noqa: E731
    idx1, idx2 = index[:, :5].contiguous(), index[:, 5:].contiguous()
    st, a = call(idx1, _lib.ProtectCarry(None, None, None, *ptrs(halves[0])))
    assert st == _lib.AC_OK, lib.ac_last_error()
    for bad in (None, _lib.ProtectCarry(*ptrs(halves[0]), *ptrs(halves[0])), _lib.ProtectCarry(*ptrs(halves[0]), None, None, None),
                _lib.ProtectCarry(halves[0][0].data_ptr(), None, None, *ptrs(halves[1]))):
        st, out = call(idx2, bad)
        assert st == _lib.AC_EINVAL and lib.ac_last_error() and int((out[0] != 7).sum()) == 0
    with _env(PROTECT_NOFUSE):
        assert lib.ac_protect_chunk_launches(psy, 2, R2) == lib.ac_protect_launches(psy, 2, R2) != 1
        st, out = call(idx2, _lib.ProtectCarry(*ptrs(halves[0]), *ptrs(halves[1])))
        assert st == _lib.AC_EUNSUPPORTED and int((out[0] != 7).sum()) == 0
    st, b = call(idx2, _lib.ProtectCarry(*ptrs(halves[0]), *ptrs(halves[1])))
    assert st == _lib.AC_OK, lib.ac_last_error()
    got = (torch.cat((a[0].view(3, 5, 2, sb), b[0].view(3, 7, 2, sb)), dim=1),) + tuple(torch.cat((a[i], b[i]), dim=1) for i in range(1, 5))
    want = (whole[0].view(3, 12, 2, sb), whole[2].view(torch.uint8), whole[3].view(torch.uint8), whole[4], whole[5])
    for g, w, name in zip(got, want, ("slots", "fits", "red_fits", "offset", "red_offset")):
        assert same_bits(g, w), name


@gpu
@pytest.mark.parametrize("pcm16", [False, True], ids=["f32", "pcm16"])
def test_chain_encode_chunks_protect_chunks_lose_recover_chunks(pcm16, monkeypatch):
    """128 kbit/s rows chunk by chunk -> 64 kbit/s slots with a 16 kbit/s copy chunk by chunk -> rows lost -> recovering chunks
    and a flush: bit-equal to the one-shot chain (encode_packed_rows, protect_packed_rows, decode_packed with redundant_at) on
    the front-extended pattern."""
    monkeypatch.delenv(NOFUSE, raising=False)
    monkeypatch.delenv(PROTECT_NOFUSE, raising=False)
    from test_encode_quantized_fused import _pcm
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_bitrate(128000), base.with_bitrate(64000)
    R2 = base.row_bits_for_bitrate(16000)
    assert (src.row_bits, dst.row_bits, R2) == (2730, 1365, 341)
    B, K, C = 2, 9, 2
    x = _pcm(N0, C, B, K, seed=64, inject=False)
    data, index, _ = src.encode_packed_rows(x)
    index = index[:, :K].contiguous()                              # a stream of K blocks has K rows
    out, idx, fits, red_fits = dst.protect_packed_rows(data, index, R2)
    assert bool(fits.all()) and bool(red_fits.all())
    lost = np.zeros((B, K, C), dtype=np.uint8)
    lost[0, 3, 0] = lost[1, 0, 1] = lost[1, 6, :] = 1              # isolated; row 3 is the last row of a chunk
    lost[0, 7:9, 1] = 1                                            # a run of 2 that ends the stream
    lost_d, o = _dev(lost), dst.row_bytes
    want = _one_shot(dst, out, idx, lost_d, pcm16, 8, o)
    enc, ps, dec = src.stream(B, C), dst.protect_stream(B, C, R2), dst.stream(B, C)
    got = []
    for a, b in _bounds((4, 1, 4)):
        rows = enc.encode_packed_rows_chunk(x[:, a * N0:b * N0].contiguous())
        slots = ps.protect_chunk(rows[0], rows[1])
        assert same_bits(slots[0].view(B, b - a, C, -1), out.view(B, K, C, -1)[:, a:b])
        got.append(dec.decode_packed_chunk(slots[0], slots[1], pcm16, lost=lost_d[:, a:b].contiguous(), max_age=8, redundant_at=o))
    got.append(dec.flush_packed(pcm16))
    assert same_bits(torch.cat(got, dim=1), want)
    plain = _one_shot(dst, out, idx, torch.zeros_like(lost_d), pcm16, 8, o).view(B, K + 1, N0, C)
    blocks = torch.cat(got, dim=1).view(B, K + 1, N0, C)
    assert not same_bits(blocks[0, 4:6, :, 0], plain[0, 4:6, :, 0])   # (the copy at 16 kbit/s is not the row)


@gpu
@pytest.mark.parametrize("route", ["one launch", "composition"])
def test_protect_chunk_only_enqueues(route, harness, monkeypatch):
    monkeypatch.delenv(PROTECT_NOFUSE, raising=False)
    from test_encode_quantized_fused import _pcm
    base = audiocodec_amd.AudioCodec(48000, N0)
    codec = base.with_row_budget(1365)
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(_pcm(N0, 2, 2, 11, seed=77, inject=False))
    whole = codec.protect_packed_rows(data, index, 341, True)
    if route == "composition":
        codec.protect_stream(2, 2, 341).protect_chunk(data, index)   # (the plan of the redundant budget exists)
        monkeypatch.setenv(PROTECT_NOFUSE, "1")
    ps = codec.protect_stream(2, 2, 341)
    assert (ps.launches() == 1) == (route == "one launch")
    torch.cuda.synchronize()

    def fn(data, index):
        ps.reset()
        return ps.protect_chunk(data, index[:, :5].contiguous(), True) + ps.protect_chunk(data, index[:, 5:].contiguous(), True)
    case = ((data, index), fn)
    name = "protect_chunk[1024-2,%s]" % route
    ref = harness.reference(case)
    sb = codec.protected_slot_bytes(341)
    assert same_bits(torch.cat((ref[0].view(2, 5, 2, sb), ref[6].view(2, 7, 2, sb)), dim=1), whole[0].view(2, 12, 2, sb))
    harness.delayed_producer(name, case, ref)
    harness.busy_default(name, case, ref)
    side = harness.fresh()
    ps.reset()
    torch.cuda.synchronize()
    a = ps.protect_chunk(data, index[:, :5].contiguous(), True, stream=side)
    b = ps.protect_chunk(data, index[:, 5:].contiguous(), True, stream=side)
    side.synchronize()
    assert same_bits(a[0], ref[0]) and same_bits(b[0], ref[6]) and same_bits(b[5], ref[11])


@gpu
def test_noise_slots_store_narrow_codes_only():
    """Why hold_conditions is asked of the tonal recipe and not of protect_layouts.slots_noise (top of the file): numpy's reading
    of the noise slots' copies at R = R2 = 1365 finds no code field of 9 bits or more (on the recovered copies of the mono
    slots: widths 1 .. 3), so none across a word boundary."""
    import protect_layouts as pl
    for C in (1, 2):
        codec, _, _, data, index = _slots("noise", C, 12)
        _, _, w = pl.copies(data, np.concatenate((index[:, :1], index), axis=1), codec.row_bytes, codec.psy.scale_band_offsets)
        stored = w[(w >= 1) & (w <= 16)]
        assert stored.size > 0 and int(stored.max()) < 9 and not pl.crossing_rows(w, codec.psy.scale_band_offsets).any()
