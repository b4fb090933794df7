"""Protected rows and the recovering decode: ``AudioCodec.protect_packed_rows`` (the ``AC_IN_PACKED |
AC_EMIT_PACKED | AC_EMIT_REDUNDANT`` form of ``ac_encode_fused_ex``, k_protect_p) and ``decode_packed(..., lost=,
redundant_at=)`` (``ac_conceal_redundant``, k_inv_fast_plr).

Every comparison is bit for bit.  Protect: the one launch, the composition -- ``transrate_packed_rows`` at both budgets and
torch copies, everywhere while ``AC_PROTECT_NOFUSE=1`` is set -- and ``protect_reference.np_protect``.  Recover: the kernel,
the composition -- ``conceal_plan(redundant_at=)``, ``unpack``, ``conceal_fade``, ``decode_quantized``, everywhere while
``AC_DECODE_PACKED_NOFUSE=1`` is set -- and ``decode_quantized`` of the rows numpy plans and fades.  The 341-bit copies recovered
from here store at most one band; test_protect_layouts.py recovers from copies that carry content, at other layouts and budgets.
"""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib
from conftest import ROOT

import boundary_inputs as bi
import fused_layouts as fl
from conceal_reference import np_conceal_plan, np_fade
from pack_reference import np_pack, np_row_bits, np_unpack
from pack_rows_reference import marked_row, row_bytes
from protect_reference import np_protect, np_recover_plan, np_recover_src_index, slot_bytes
from rate_reference import quantize_budget
from stream_order import same_bits
from test_encode_quantized_fused import _pcm, _where
from test_rate_control import EX_OFF, EX_THR, EX_X, unlimited
from transrate_reference import np_transrate, requant_fast

gpu = pytest.mark.gpu
N0, M0 = 1024, 64
CAP = _lib.AC_PACK_ROWS_MAX_BITS
HEADER = os.path.join(ROOT, "include", "audiocodec_amd.h")
NAMES = ("data", "index", "fits", "red_fits", "offset", "red_offset")


# ---- CPU: the plan ------------------------------------------------------------------------------------------------------
def _lost(F, frames, B=1, C=1):
    lost = np.zeros((B, F, C), dtype=np.uint8)
    lost[:, list(frames)] = 1
    return lost


def _plan(F, frames, max_age=8):
    src, age, rec = np_recover_plan(_lost(F, frames), max_age)
    return src[0, :, 0].tolist(), age[0, :, 0].tolist(), rec[0, :, 0].tolist()


def test_plan_an_isolated_loss_is_recovered():
    src, age, rec = _plan(6, [2])
    assert src == [0, 1, 3, 3, 4, 5] and age == [0] * 6 and rec == [False, False, True, False, False, False]


def test_plan_frame_0_lost_is_recovered_where_concealment_mutes_it():
    assert np_conceal_plan(_lost(4, [0]), 8)[0][0, :, 0].tolist() == [-1, 1, 2, 3]
    src, age, rec = _plan(4, [0])
    assert src == [1, 1, 2, 3] and rec == [True, False, False, False] and age == [0] * 4


def test_plan_the_last_frame_has_no_successor():
    src, age, rec = _plan(4, [3])
    assert src == [0, 1, 2, 2] and age == [0, 0, 0, 1] and not any(rec)
    src, age, rec = _plan(1, [0])                                       # a clip of one frame
    assert src == [-1] and not any(rec)


def test_plan_only_the_last_row_of_a_run_is_recovered():
    src, age, rec = _plan(8, [2, 3])                                    # a run of 2
    assert src == [0, 1, 1, 4, 4, 5, 6, 7] and age == [0, 0, 1, 0, 0, 0, 0, 0] and rec[3] and sum(rec) == 1
    src, age, rec = _plan(8, [2, 3, 4])                                 # a run of 3: ages 1, 2 from before the run
    assert src == [0, 1, 1, 1, 5, 5, 6, 7] and age == [0, 0, 1, 2, 0, 0, 0, 0] and rec[4] and sum(rec) == 1
    # a run that reaches the clip's end has no recovered row; the one before it is still recovered
    src, age, rec = _plan(8, [2, 4, 5, 6, 7])
    assert rec == [False, False, True] + [False] * 5 and src[4:] == [3, 3, 3, 3] and age[4:] == [1, 2, 3, 4]


def test_plan_a_run_reaching_frame_0():
    src, age, rec = _plan(6, [0, 1, 2])
    assert src == [-1, -1, 3, 3, 4, 5] and rec == [False, False, True, False, False, False] and age == [0] * 6


def test_plan_max_age_0_and_31():
    src, age, rec = _plan(6, [1, 2, 4], max_age=0)
    assert src == [0, -1, 3, 3, 5, 5] and age == [0] * 6 and rec == [False, False, True, False, True, False]
    frames = list(range(1, 39))
    src, age, rec = _plan(40, frames, max_age=31)
    assert age[:32] == list(range(32)) and src[32:38] == [-1] * 6 and src[38] == 39 and rec[38] and sum(rec) == 1


def test_plan_clips_and_channels_are_independent():
    lost = np.zeros((2, 3, 2), dtype=np.uint8)
    lost[0, 2, 0] = 1            # the last frame of clip 0 is not recovered from frame 0 of clip 1
    lost[1, 0, 1] = 1            # recovered from frame 1 of its own channel
    lost[1, 1, 0] = 1            # its successor in the OTHER channel did not arrive: no bearing
    lost[1, 2, 0] = 1
    src, age, rec = np_recover_plan(lost, 8)
    assert rec.sum() == 1 and rec[1, 0, 1] and src[1, 0, 1] == 1
    assert src[0, :, 0].tolist() == [0, 1, 1] and src[1, :, 0].tolist() == [0, 0, 0] and age[1, :, 0].tolist() == [0, 1, 2]
    index = np.arange(12, dtype=np.int64).reshape(2, 3, 2) * 1000
    got, a8 = np_recover_src_index(index, lost, 99999, 8, 7)
    assert got[1, 0, 1] == index[1, 1, 1] + 7 and got[0, 2, 0] == index[0, 1, 0] and a8.dtype == np.uint8


def test_plan_nothing_lost_is_the_identity():
    lost = np.zeros((2, 5, 2), dtype=np.uint8)
    src, age, rec = np_recover_plan(lost, 8)
    assert not rec.any() and not age.any() and (src == np.arange(5)[None, :, None]).all()
    index = np.arange(20, dtype=np.int64).reshape(2, 5, 2) * 64
    assert np.array_equal(np_recover_src_index(index, lost, 5, 8, 100)[0], index)


# ---- CPU: protected rows on the worked example --------------------------------------------------------------------------
def test_np_protect_on_the_worked_example():
    """Section 8c's row (M = 4, 100 bits) and quieter copies of it, B = 2, F = 3: R = 96, R2 = 56."""
    X = np.concatenate([EX_X * g for g in (1.0, 0.5, 0.25)], axis=1)
    X = np.concatenate([X, X[:, ::-1] * 0.8], axis=0)
    thr = np.broadcast_to(EX_THR, X.shape)
    codes, sf, _, _ = quantize_budget(X, thr, EX_OFF, 200, 0)
    data, index = np_pack(codes, sf, EX_OFF)
    R, R2 = 96, 56
    out, idx, fits, red_fits, offset, red_offset = np_protect(data, index, EX_OFF, 8, R, R2)
    rb, sb = row_bytes(R), slot_bytes(R, R2)
    assert (rb, sb) == (12, 20) and out.shape == (6 * sb,) and idx.ravel().tolist() == [r * sb for r in range(6)]
    prim, red = np_transrate(data, index, EX_OFF, 8, R), np_transrate(data, index, EX_OFF, 8, R2)
    slots = out.reshape(2, 3, 1, sb)
    assert np.array_equal(slots[..., :rb].reshape(-1), prim[0])                      # the primary parts
    assert np.array_equal(slots[:, 1:, :, rb:], red[0].reshape(2, 3, 1, sb - rb)[:, :2])   # frame f carries frame f - 1
    assert not slots[:, 0, :, rb:].any() and red_fits[:, 0].all() and not red_offset[:, 0].any()
    # the copy of the last frame is nowhere, and slot (1, 0) takes nothing from clip 0
    assert red[0].reshape(2, 3, 1, -1)[0, 2].any() and not slots[1, 0, :, rb:].any()
    assert np.array_equal(fits, prim[2]) and np.array_equal(offset, prim[3]) and np.array_equal(red_offset[:, 1:], red[3][:, :2])
    assert int(offset.max()) > 0 and int(red_offset.max()) > int(offset.max())


# ---- CPU: header, library, Python validation ----------------------------------------------------------------------------
def _struct(text, name):
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S)
    assert m, "%s is not declared" % name
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    return [" ".join(f.split()) for f in body.split(";") if f.strip()]


def test_header_declares_the_flags_the_structs_and_the_query():
    text = open(HEADER).read()
    assert re.search(r"\bAC_EMIT_REDUNDANT\s*=\s*256\b", text) and re.search(r"\bAC_CONCEAL_REDUNDANT\s*=\s*256\b", text)
    assert (_lib.AC_EMIT_REDUNDANT, _lib.AC_CONCEAL_REDUNDANT) == (256, 256)
    assert _struct(text, "ac_protected_out") == ["uint8_t* data", "int64_t row_bytes", "uint8_t* fits", "int32_t red_bits",
                                                 "uint8_t* red_fits", "int16_t* offset", "int16_t* red_offset"]
    assert _struct(text, "ac_conceal_redundant") == ["const uint8_t* lost", "int32_t max_age", "int64_t redundant_at"]
    assert _struct(text, "ac_conceal_redundant")[:2] == _struct(text, "ac_conceal")
    m = re.search(r"AC_API\s+int\s+ac_protect_launches\s*\(([^;]*)\)\s*;", text)
    assert m and "stream" not in m.group(1), m and m.group(1)
    assert re.search(r"#define\s+AC_VERSION\s+171\b", text)


def test_ctypes_mirrors_have_the_headers_layout():
    P = _lib.ProtectedOut
    assert [f[0] for f in P._fields_] == ["data", "row_bytes", "fits", "red_bits", "red_fits", "offset", "red_offset"]
    assert [getattr(P, f[0]).offset for f in P._fields_] == [0, 8, 16, 24, 32, 40, 48] and ctypes.sizeof(P) == 56
    assert P.red_bits.size == 4
    R = _lib.ConcealRedundant
    assert [f[0] for f in R._fields_] == ["lost", "max_age", "redundant_at"]
    assert (R.lost.offset, R.max_age.offset, R.redundant_at.offset, R.max_age.size) == (0, 8, 16, 4) and ctypes.sizeof(R) == 24
    assert (R.lost.offset, R.max_age.offset) == (_lib.Conceal.lost.offset, _lib.Conceal.max_age.offset)


def test_library_exports_the_launch_query():
    lib = _lib.load()
    assert "ac_protect_launches" in _lib.PROTOTYPES and lib.ac_protect_launches(None, 2, 341) == 0
    assert lib.ac_version() == 171


def test_python_interface_validates_its_arguments():
    base = audiocodec_amd.AudioCodec(48000, N0)
    data, index = torch.zeros(64, dtype=torch.uint8), torch.zeros((1, 2, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"with_bitrate\(\)"):
        base.protect_packed_rows(data, index, 341)
    with pytest.raises(ValueError, match=r"with_bitrate\(\)"):
        base.protected_slot_bytes(341)
    cbr = base.with_bitrate(64000)
    assert cbr.protected_slot_bytes(341) == cbr.row_bytes + 44 and cbr.protected_slot_bytes(320) == cbr.row_bytes + 40
    for bad in (341.0, True, None, "341"):
        with pytest.raises(TypeError, match="red_bits"):
            cbr.protect_packed_rows(data, index, bad)
    for bad in (319, 0, -5):
        with pytest.raises(ValueError, match="red_bits"):
            cbr.protect_packed_rows(data, index, bad)
        with pytest.raises(ValueError, match="red_bits"):
            cbr.protected_slot_bytes(bad)
    for bad in ((data.to(torch.int8), index), (data, index.to(torch.int32)), (data, index[0]), (data, index)):   # the last: host
        with pytest.raises(ValueError):
            cbr.protect_packed_rows(*bad, 341)
    lost = torch.zeros((1, 2, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="without lost"):
        base.decode_packed(data, index, redundant_at=8)
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match="redundant_at"):
            base.decode_packed(data, index, lost=lost, redundant_at=bad)
        with pytest.raises(ValueError, match="redundant_at"):
            base.psy.conceal_plan(index, lost, 64, 8, redundant_at=bad)
    for bad in (8.0, True, "8"):
        with pytest.raises(TypeError, match="redundant_at"):
            base.decode_packed(data, index, lost=lost, redundant_at=bad)
    sig = inspect.signature(audiocodec_amd.AudioCodec.decode_packed)
    assert sig.parameters["redundant_at"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["redundant_at"].default is None
    sig = inspect.signature(audiocodec_amd.PsychoacousticModel.conceal_plan)
    assert sig.parameters["redundant_at"].default is None and sig.parameters["max_age"].default == 8
    sig = inspect.signature(audiocodec_amd.AudioCodec.protect_packed_rows_launches)
    assert sig.parameters["red_bits"].kind is inspect.Parameter.KEYWORD_ONLY


def test_the_kept_redundant_codec_is_freed_with_its_owner():
    """The composition keeps ``with_row_budget(red_bits)`` per codec.  Neither codec may sit in a reference cycle: a cycle is
    freed by the garbage collector at some later allocation, and a plan destroyed there -- it frees device memory -- ends a
    graph capture that happens to be under way."""
    import gc
    import weakref
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        dst = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
        red = dst._redundant_codec(341)
        assert red is dst._redundant_codec(341) and red.row_bits == 341 and red is not dst._redundant_codec(400)
        assert red._red_codecs is not dst._red_codecs and not red._red_codecs
        refs = [weakref.ref(o) for o in (dst, red, red.psy, dst.psy)]
        del dst, red
        assert [r() for r in refs] == [None] * 4, "a codec or its model is only freed by the garbage collector"
    finally:
        if was:
            gc.enable()


# ---- GPU: protect -------------------------------------------------------------------------------------------------------
class _env:
    """NAME=1 (read per call) around a block."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        os.environ[self.name] = "1"

    def __exit__(self, *exc):
        del os.environ[self.name]
        return False


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _x(B, K, C, seed):
    """Ramped noise at a level per clip; from two blocks on, block 0 of clip 0 is zeroed (an all-zero row)."""
    x = _pcm(N0, C, B, K, seed=seed, inject=False)
    if K >= 2:
        x[0, :N0] = 0.0
    return x


def _protect_composition(codec, data, index, R2):
    with _env("AC_PROTECT_NOFUSE"):
        assert codec.protect_packed_rows_launches(index.shape[2], red_bits=R2) == 2
        return codec.protect_packed_rows(data, index, R2, True)


def _protect3(codec, data, index, R2, off=None):
    """numpy, the composition and the one launch on the same rows (numpy arrays); returns the reference."""
    off = codec.psy.scale_band_offsets if off is None else off
    ref = np_protect(data, index, off, N0, codec.row_bits, R2)
    d, i = _dev(np.asarray(data, dtype=np.uint8)), _dev(np.asarray(index, dtype=np.int64))
    comp = _protect_composition(codec, d, i, R2)
    assert codec.protect_packed_rows_launches(index.shape[2], red_bits=R2) == 1
    fused = codec.protect_packed_rows(d, i, R2, True)
    assert len(codec.protect_packed_rows(d, i, R2)) == 4
    for name, g, c, r in zip(NAMES, fused, comp, ref):
        assert g.dtype == c.dtype and g.shape == c.shape, name
        np.testing.assert_array_equal(c.cpu().numpy(), r, err_msg="composition != numpy: %s, R2 = %d" % (name, R2))
        assert torch.equal(g, c), ("kernel != composition", name, R2, _where(g, c))
    return ref


@gpu
@pytest.mark.parametrize("B,F,C", [(1, 1, 1), (2, 3, 2), (3, 5, 1), (1, 2, 3), (2, 1, 2)])
def test_protect_fused_composition_numpy(B, F, C):
    """1, 12, 15, 6 and 4 rows: tail waves in the last workgroup; F = 1: only frame-0 slots."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    x = _x(B, F - 1, C, 3 * B + F + C)
    for R, R1, reds in ((2730, 1365, (320, 682, 1365)), (1365, 1365, (320,))):
        data, index, _ = base.with_row_budget(R).encode_packed_rows(x)
        assert tuple(index.shape) == (B, F, C)
        dst = base.with_row_budget(R1)
        for R2 in reds:
            ref = _protect3(dst, data.cpu().numpy(), index.cpu().numpy(), R2)
            assert ref[0].shape == (B * F * C * dst.protected_slot_bytes(R2),)
            assert ref[3][:, 0].all() and not ref[5][:, 0].any()
            if F >= 2 and R2 < R:
                assert int(ref[5].max()) > 0, "the redundant budget does not bind"
            if R1 == R:                                                   # the primary part is the input row's bytes
                rb = dst.row_bytes
                got = ref[0].reshape(B, F, C, -1)[..., :rb]
                assert np.array_equal(got.reshape(-1), data.cpu().numpy()) and ref[2].all() and not ref[4].any()


def _adversarial():
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    band = np.repeat(np.arange(M0), np.diff(off))
    rng = np.random.default_rng(78)
    B, F, C = 1, 6, 2
    codes = rng.integers(-200, 201, (B, F, N0, C)).astype(np.int16)
    sf = rng.integers(-40, 0, (B, F, M0, C)).astype(np.int8)
    codes[0, 0, :, 0] = np.where(np.arange(N0) % 3 == 0, -32768, np.where(np.arange(N0) % 3 == 1, 32767, -32767))   # 17216 bits
    sf[0, 0, :, 1] = np.where(np.arange(M0) % 2 == 0, 127, -127)
    codes[0, 1, :, 0] = np.where(np.arange(N0) % 2 == 0, 32767, -32767)     # the saturating row: fits no budget below its own
    sf[0, 1, :, 0] = 127
    sf[0, 1, ::3, 1] = -128
    codes[0, 1, :, 1] = np.where((band % 3 == 1), 0, codes[0, 1, :, 1])
    sf[0, 3, :, 1] = -128                                                  # a marked input row
    data, index = np_pack(codes, sf, off)
    assert int(np_row_bits(codes, sf, off)[0, 0, 0]) == 16 * N0 + 13 * M0 > CAP
    return base, off, data, index, rng


@gpu
def test_protect_adversarial_rows():
    base, off, data, index, rng = _adversarial()
    for R, R2 in ((1365, 320), (1365, 682), (CAP, 1365)):
        ref = _protect3(base.with_row_budget(R), data, index, R2)
        assert not ref[3][0, 2, 0] and int(ref[5][0, 2, 0]) == 254         # the saturating row's copy, in frame 2's slot
        if R < CAP:
            assert not ref[2][0, 1, 0] and int(ref[4][0, 1, 0]) == 254     # ... and its primary part
        sb, rb = slot_bytes(R, R2), row_bytes(R)
        assert np.array_equal(ref[0].reshape(1, 6, 2, sb)[0, 2, 0, rb:], marked_row(M0, R2))
        assert ref[3][0, 4, 1] and int(ref[5][0, 4, 1]) == 0               # a marked input row passes through and fits
    dst = base.with_row_budget(1365)
    damaged = data.copy()                                                  # widths 17 .. 30 read as 31
    bits = np.unpackbits(damaged, bitorder="little")
    start = int(index[0, 2, 0]) * 8
    for j, wv in ((3, 17), (10, 30), (40, 23)):
        bits[start + 5 * j:start + 5 * j + 5] = [(wv >> k) & 1 for k in range(5)]
    _protect3(dst, np.packbits(bits, bitorder="little"), index, 400)
    for cut in (int(index[0, 5, 1]) + 100, int(index[0, 5, 1]) + 13, int(index[0, 3, 0]) + 2):    # truncated data
        _protect3(dst, data[:cut], index, 400)
    odd = index.copy()                                                     # negative, past the end, off the 4-byte phase
    odd[0, 0, 0], odd[0, 1, 1], odd[0, 2, 0], odd[0, 3, 1], odd[0, 4, 0] = -7, len(data) + 1000, index[0, 2, 0] + 1, -(1 << 50), len(data) - 3
    odd[0, 5, 0] = (1 << 40)
    _protect3(dst, data, odd, 400)
    perm = index.reshape(-1)[rng.permutation(index.size)].reshape(index.shape)
    ref = _protect3(dst, data, perm, 400)
    assert len(np.unique(ref[5])) >= 3
    _protect3(dst, data, np.ascontiguousarray(index[:, 1:4]), 400)
    d, i = _dev(data), _dev(index)
    got = dst.protect_packed_rows(d, i[:, 1:4], 400, True)                 # a strided view of the index tensor
    for g, w in zip(got, dst.protect_packed_rows(d, i[:, 1:4].contiguous(), 400, True)):
        assert torch.equal(g, w)


@gpu
def test_protect_dense_input():
    base = audiocodec_amd.AudioCodec(48000, N0)
    data, index = base.encode_packed(_x(3, 4, 2, 21))                      # dense rows of the unbudgeted quantiser
    ref = _protect3(base.with_row_budget(2730), data.cpu().numpy(), index.cpu().numpy(), 682)
    assert int(ref[5].max()) > 0 and len(np.unique(ref[5])) >= 2


@gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", fl.LAYOUTS, ids=fl.LAYOUT_IDS)
def test_protect_band_layouts(layout, C):
    sr, alpha = fl.resolve(layout)
    base = audiocodec_amd.AudioCodec(sr, N0, alpha=alpha)
    x = torch.from_numpy(fl.tonal(C)).cuda()
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(x)
    ref = _protect3(base.with_row_budget(1365), data.cpu().numpy(), index.cpu().numpy(), 400)
    assert int((ref[4] > 0).sum()) >= 1 and len(np.unique(ref[5])) >= 2


@gpu
def test_protect_second_search_at_equality():
    """R2 = bits_r(k) at the first offset of a length, and R2 - 1: the copy of that row, in the next frame's slot."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(_x(2, 3, 2, 9))
    data, index = data.cpu().numpy(), index.cpu().numpy()
    codes, sf = np_unpack(data, index, off, N0)
    bits = requant_fast(codes, sf, off, unlimited(N0, M0), 0)[4]
    targets = [t for t in bi.plateau_starts(bits, 0, hi=2730) if t.row[1] + 1 < index.shape[1]]
    dst = base.with_row_budget(2730)
    for t in bi.pick_three(targets):
        b, f, c = t.row
        at = _protect3(dst, data, index, t.R)
        assert int(at[5][b, f + 1, c]) == t.k and at[3][b, f + 1, c]
        under = _protect3(dst, data, index, t.R - 1)
        assert int(under[5][b, f + 1, c]) > t.k


@gpu
def test_protect_redundant_slot_slack():
    """R2 against 8 red_bytes on rows of constant length: R2 bits stay at offset 0; one more bit ends on the slot's last bit
    (offset 254, fits); one more than the slot is the marked row."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    R2 = 1375
    codes, sf, _ = bi.slot_rows(off, R2)                                  # [1, 4, N, 1]: R2, R2 + 1, R2 + 2, R2 - 1 bits
    codes = np.concatenate([codes, codes[:, :1]], axis=1)                 # a fifth frame to carry the fourth's copy
    sf = np.concatenate([sf, sf[:, :1]], axis=1)
    data, index = np_pack(codes, sf, off)
    ref = _protect3(base.with_row_budget(2730), data, index, R2)
    assert ref[3].ravel().tolist() == [True, True, True, False, True] and ref[5].ravel().tolist() == [0, 0, 254, 254, 0]


@gpu
def test_protect_chip_filling():
    """8224 rows -- 2056 workgroups of four waves -- against the composition."""
    B, K, C = 16, 256, 2
    base = audiocodec_amd.AudioCodec(48000, N0)
    g = torch.Generator(device="cuda").manual_seed(4321)
    x = torch.rand((B, K * N0, C), generator=g, device="cuda") * 2 - 1
    x *= torch.logspace(-3, 0, B, device="cuda")[:, None, None] * torch.linspace(0.05, 1, K * N0, device="cuda")[None, :, None]
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(x)
    dst = base.with_row_budget(1365)
    assert index.numel() == 8224 and dst.protect_packed_rows_launches(C, red_bits=341) == 1
    fused = dst.protect_packed_rows(data, index, 341, True)
    comp = _protect_composition(dst, data, index, 341)
    for name, a, b in zip(NAMES, fused, comp):
        assert torch.equal(a, b), (name, _where(a, b))
    assert int((comp[5] > comp[4]).sum()) >= 1000 and bool(comp[3].all())


@gpu
def test_protect_launch_table_and_fallbacks(monkeypatch):
    base = audiocodec_amd.AudioCodec(48000, N0)
    assert base.protect_packed_rows_launches(2, red_bits=341) == 0
    cbr = base.with_row_budget(1365)
    for C in (1, 2, 3, 7):
        for R2 in (320, 1365, CAP):
            assert cbr.protect_packed_rows_launches(C, red_bits=R2) == 1, (C, R2)
    assert cbr.protect_packed_rows_launches(2, red_bits=CAP + 32) == 4     # one launch at R, three at R2
    monkeypatch.setenv("AC_PROTECT_NOFUSE", "1")
    assert cbr.protect_packed_rows_launches(2, red_bits=341) == 2
    monkeypatch.setenv("AC_TRANSRATE_NOFUSE", "1")
    assert cbr.protect_packed_rows_launches(2, red_bits=341) == 6
    monkeypatch.delenv("AC_PROTECT_NOFUSE")
    assert cbr.protect_packed_rows_launches(2, red_bits=341) == 6          # no one launch without k_transrate_p's
    monkeypatch.delenv("AC_TRANSRATE_NOFUSE")
    # R2 above the cap: the composition, numpy's bytes
    x = _x(2, 2, 2, 5)
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(x)
    ref = np_protect(data.cpu().numpy(), index.cpu().numpy(), base.psy.scale_band_offsets, N0, 1365, CAP + 32)
    for name, g, r in zip(NAMES, cbr.protect_packed_rows(data, index, CAP + 32, True), ref):
        np.testing.assert_array_equal(g.cpu().numpy(), r, err_msg=name)
    # filters_n = 2048: six launches
    wide = audiocodec_amd.AudioCodec(48000, 2048)
    x = _pcm(2048, 2, 2, 3, seed=4, inject=False)
    data, index, _ = wide.with_row_budget(2730).encode_packed_rows(x)
    dst = wide.with_row_budget(1365)
    assert dst.protect_packed_rows_launches(2, red_bits=400) == 6
    ref = np_protect(data.cpu().numpy(), index.cpu().numpy(), wide.psy.scale_band_offsets, 2048, 1365, 400)
    assert int(ref[5].max()) > 0
    for name, g, r in zip(NAMES, dst.protect_packed_rows(data, index, 400, True), ref):
        np.testing.assert_array_equal(g.cpu().numpy(), r, err_msg=name)


def _protect_abi(codec, data, index, bufs, rb, R2, flags=None, out1=None, X=None, B=None, src=True, dst=True, offsets=True):
    lib = _lib.load()
    dev = data.device
    rows = _lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr())
    out, fits, red_fits, offset, red_offset = bufs
    po = _lib.ProtectedOut(out.data_ptr(), rb, fits.data_ptr(), R2, red_fits.data_ptr(), offset.data_ptr() if offsets else None,
                           red_offset.data_ptr() if offsets else None)

    def p(v):
        return ctypes.c_void_p(v.data_ptr()) if v is not None else None
    IN, EMIT, RED = _lib.AC_IN_PACKED, _lib.AC_EMIT_PACKED, _lib.AC_EMIT_REDUNDANT
    st = lib.ac_encode_fused_ex(codec.mdct._plan(dev), codec.psy._plan(dev), ctypes.addressof(rows) if src else None, p(X), None,
                                None, 0.0, (IN | EMIT | RED) if flags is None else flags, ctypes.addressof(po) if dst else None,
                                p(out1), 0, index.shape[0] if B is None else B, index.shape[1] - 1, index.shape[2], None)
    torch.cuda.synchronize()
    return st


@gpu
def test_protect_c_abi():
    lib = _lib.load()
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    data, index, _ = src.encode_packed_rows(_x(3, 5, 2, 17))
    rows, rb, R2 = index.numel(), dst.row_bytes, 341
    bufs = (torch.full((rows * dst.protected_slot_bytes(R2),), 0xA5, dtype=torch.uint8, device="cuda"),
            torch.full((rows,), 7, dtype=torch.uint8, device="cuda"), torch.full((rows,), 7, dtype=torch.uint8, device="cuda"),
            torch.full((rows,), -3, dtype=torch.int16, device="cuda"), torch.full((rows,), -3, dtype=torch.int16, device="cuda"))
    refused = tuple(b.clone() for b in bufs)
    spare = torch.zeros((3, 6, N0, 2), device="cuda")
    IN, EMIT, RED = _lib.AC_IN_PACKED, _lib.AC_EMIT_PACKED, _lib.AC_EMIT_REDUNDANT
    for flags in (RED, IN | RED, EMIT | RED, IN | EMIT | RED | _lib.AC_IN_PCM16, IN | EMIT | RED | _lib.AC_EMIT_CODES,
                  _lib.AC_EMIT_CODES | RED, IN | EMIT | RED | 128, IN | EMIT | 128, IN | EMIT | RED | 512):
        assert _protect_abi(dst, data, index, bufs, rb, R2, flags=flags) == _lib.AC_EINVAL, flags
        assert lib.ac_last_error()
    for kw in ({"X": spare}, {"out1": spare}, {"src": False}, {"dst": False}):
        assert _protect_abi(dst, data, index, bufs, rb, R2, **kw) == _lib.AC_EINVAL, kw
    assert _protect_abi(dst, data, index, bufs, rb + 4, R2) == _lib.AC_EINVAL and b"row_bytes" in lib.ac_last_error()
    assert _protect_abi(dst, data, index, bufs, rb, 319) == _lib.AC_EINVAL and b"red_bits" in lib.ac_last_error()
    assert _protect_abi(base, data, index, bufs, rb, R2) == _lib.AC_EINVAL and b"row budget" in lib.ac_last_error()
    wide = audiocodec_amd.AudioCodec(48000, 2048).with_row_budget(1365)
    assert _protect_abi(wide, data, index, bufs, rb, R2) == _lib.AC_EUNSUPPORTED and b"composition" in lib.ac_last_error()
    assert _protect_abi(dst, data, index, bufs, rb, CAP + 32) == _lib.AC_EUNSUPPORTED
    with _env("AC_PROTECT_NOFUSE"):
        assert _protect_abi(dst, data, index, bufs, rb, R2) == _lib.AC_EUNSUPPORTED
    for got, want in zip(bufs, refused):                                   # the refused calls wrote nothing
        assert torch.equal(got, want)
    assert _protect_abi(dst, data, index, bufs, rb, R2, B=0) == _lib.AC_OK
    assert torch.equal(bufs[0], refused[0])
    ref = _protect_composition(dst, data, index, R2)
    assert _protect_abi(dst, data, index, bufs, rb, R2) == _lib.AC_OK, lib.ac_last_error()
    assert torch.equal(bufs[0], ref[0])
    for got, want in zip(bufs[1:], ref[2:]):
        assert torch.equal(got.view(3, 6, 2), want.to(got.dtype))
    bufs[0].fill_(0xA5)
    bufs[3].fill_(-3)
    assert _protect_abi(dst, data, index, bufs, rb, R2, offsets=False) == _lib.AC_OK      # both offsets may be NULL
    assert torch.equal(bufs[0], ref[0]) and int((bufs[3] != -3).sum()) == 0


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
def test_protect_graph_capture(route):
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    call = (lambda d, i: dst.protect_packed_rows(d, i, 341, True)) if route == "fused" else (lambda d, i: _protect_composition(dst, d, i, 341))
    data, index, _ = src.encode_packed_rows(_x(3, 5, 2, 5))
    call(data, index)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(data, index)
    for seed in (6, 7):
        data.copy_(src.encode_packed_rows(_x(3, 5, 2, seed))[0])
        g.replay()
        torch.cuda.synchronize()
        ref = call(data.clone(), index)
        assert int((ref[5] > 0).sum()) >= 1 and int(ref[0].max()) > 0
        for got, want in zip(out, ref):
            assert torch.equal(got, want), (seed, _where(got, want))


@gpu
def test_protect_an_empty_batch_gives_empty_results():
    dst = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    data = torch.zeros((64,), dtype=torch.uint8, device="cuda")
    for shape in ((0, 3, 2), (2, 0, 2)):
        got = dst.protect_packed_rows(data, torch.zeros(shape, dtype=torch.int64, device="cuda"), 341, True)
        assert got[0].shape == (0,) and [tuple(t.shape) for t in got[1:]] == [shape] * 5
        assert [t.dtype for t in got] == [torch.uint8, torch.int64, torch.bool, torch.bool, torch.int16, torch.int16]


@pytest.fixture(scope="module")
def harness():
    from stream_order import Harness
    return Harness()


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
@pytest.mark.parametrize("check", ["delayed_producer", "busy_default"])
def test_protect_stream_contract(harness, check, route):
    base = audiocodec_amd.AudioCodec(48000, N0)
    dst = base.with_row_budget(1365)
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(_pcm(N0, 2, 4, 20, seed=77, inject=False))
    _protect_composition(dst, data, index, 341)                            # (the plan of the redundant budget exists)
    torch.cuda.synchronize()
    assert dst.protect_packed_rows_launches(2, red_bits=341) == 1
    fn = (lambda d, i: dst.protect_packed_rows(d, i, 341, True)) if route == "fused" else (lambda d, i: _protect_composition(dst, d, i, 341))
    getattr(harness, check)("cbr.protect_packed_rows[1024-2,%s]" % route, ([data, index], fn))


# ---- GPU: recover -------------------------------------------------------------------------------------------------------
NOFUSE = "AC_DECODE_PACKED_NOFUSE"
_protected = {}


def _slots(C, Kp):
    """Protected slots [3, Kp, C] of seeded noise: R = 1365, R2 = 341."""
    if (C, Kp) not in _protected:
        base = audiocodec_amd.AudioCodec(48000, N0)
        dst = base.with_row_budget(1365)
        x = _pcm(N0, C, 3, max(Kp - 1, 1), seed=30 + Kp, inject=False)[:, :(Kp - 1) * N0].contiguous()
        data, index, _ = base.with_row_budget(2730).encode_packed_rows(x)
        out = dst.protect_packed_rows(data, index, 341)
        assert tuple(out[1].shape) == (3, Kp, C)
        _protected[(C, Kp)] = (dst, out[0], out[1])
    return _protected[(C, Kp)]


def _patterns(B, Kp, C, max_age):
    rng = np.random.default_rng(1000 * Kp + 10 * max_age + C)
    pats = {"none": np.zeros((B, Kp, C), dtype=np.uint8), "all": np.ones((B, Kp, C), dtype=np.uint8),
            "30 %": (rng.random((B, Kp, C)) < 0.3).astype(np.uint8)}
    for name, frames in (("isolated", [2]), ("frame 0", [0]), ("last", [Kp - 1]), ("run of 2", [2, 3]), ("run of 3", [2, 3, 4]),
                         ("run from 0", [0, 1, 2]), ("two runs", [1, 2, 4, 5])):
        pats[name] = _lost(Kp, [f for f in frames if f < Kp], B, C)
        pats[name][B - 1, :, C - 1] = 0                                   # one signal keeps every row
    return pats


def _recover_composition(codec, data, index, pcm16, lost, max_age, o):
    with _env(NOFUSE):
        assert codec.decode_packed_launches(index.shape[2]) != 1
        return codec.decode_packed(data, index, pcm16, lost=lost, max_age=max_age, redundant_at=o)


def _hold(codec, data, index, lost, max_age, o, what="", formats=(False, True)):
    """The kernel, the composition and decode_quantized of the rows numpy plans and fades; returns the float32 PCM."""
    assert codec.decode_packed_launches(index.shape[2]) == 1
    lost_d = _dev(lost)
    src, age = np_recover_src_index(index.cpu().numpy(), lost, data.numel(), max_age, o)
    plan = codec.psy.conceal_plan(index, lost_d, data.numel(), max_age, redundant_at=o)
    assert np.array_equal(plan[0].cpu().numpy(), src) and np.array_equal(plan[1].cpu().numpy(), age), (what, max_age)
    codes, sf = codec.psy.unpack(data, _dev(src))
    sf = _dev(np_fade(sf.cpu().numpy(), age))
    out = None
    for pcm16 in formats:
        fused = codec.decode_packed(data, index, pcm16, lost=lost_d, max_age=max_age, redundant_at=o)
        comp = _recover_composition(codec, data, index, pcm16, lost_d, max_age, o)
        ref = codec.decode_quantized(codes, sf, pcm16=pcm16)
        assert fused.dtype == (torch.int16 if pcm16 else torch.float32)
        assert same_bits(comp, ref), "composition != numpy: %s max_age=%d pcm16=%s" % (what, max_age, pcm16)
        assert same_bits(fused, comp), "kernel != composition: %s max_age=%d pcm16=%s" % (what, max_age, pcm16)
        out = fused if not pcm16 else out
    return out


def _substituted(index, lost, o):
    """index with index[b, f+1, c] + o at the lost rows (every one of which has a successor that arrived)."""
    sub = index.clone()
    sub[:, :-1] = torch.where(lost[:, :-1] != 0, index[:, 1:] + o, index[:, :-1])
    return sub


@gpu
@pytest.mark.parametrize("Kp", [1, 2, 7, 12])
@pytest.mark.parametrize("C", [1, 2])
def test_recover_fused_composition_numpy(C, Kp, monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, data, index = _slots(C, Kp)
    o = codec.row_bytes
    plain = {p: codec.decode_packed(data, index, pcm16=p) for p in (False, True)}
    recovered = 0
    for max_age in (0, 1, 8, 31):
        for name, lost in _patterns(3, Kp, C, max_age).items():
            out = _hold(codec, data, index, lost, max_age, o, name)
            rec = np_recover_plan(lost, max_age)[2]
            recovered += int(rec.sum())
            if name == "none":                                            # bit-equal to the plain decode, both formats
                assert same_bits(out, plain[False])
                assert same_bits(codec.decode_packed(data, index, True, lost=_dev(lost), max_age=max_age, redundant_at=o), plain[True])
            if rec.sum() == (lost != 0).sum():                            # every lost row recovered: the parent's kernel says so
                sub = _substituted(index, _dev(lost), o)
                assert same_bits(out, codec.decode_packed(data, sub)), (name, max_age)
            if name == "isolated" and Kp >= 7:                            # ... and it differs from concealing alone
                assert not same_bits(out, codec.decode_packed(data, index, lost=_dev(lost), max_age=max(max_age, 1)))
    assert recovered > 0 or Kp == 1


@gpu
@pytest.mark.parametrize("C,B,K", [(2, 64, 64), (1, 129, 96)])
def test_recover_across_strips(C, B, K, monkeypatch):
    """The strip-crossing shapes of test_conceal: frame f + 1 lies in another strip, another wave's, another workgroup's."""
    monkeypatch.delenv(NOFUSE, raising=False)
    base = audiocodec_amd.AudioCodec(48000, N0)
    codec = base.with_row_budget(1365)
    g = torch.Generator("cuda").manual_seed(B + K)
    x = (torch.rand((B, K * N0, C), device="cuda", generator=g) * 2 - 1) * torch.linspace(0.01, 1, K * N0, device="cuda")[None, :, None]
    data, index, _ = base.with_row_budget(2730).encode_packed_rows(x)
    data, index = codec.protect_packed_rows(data, index, 341)[:2]
    o = codec.row_bytes
    lost = torch.rand((B, K + 1, C), device="cuda", generator=g) < 0.3
    lost[0, 5:40] = True
    for max_age, pcm16 in ((8, False), (31, True)):
        fused = codec.decode_packed(data, index, pcm16, lost=lost, max_age=max_age, redundant_at=o)
        assert same_bits(fused, _recover_composition(codec, data, index, pcm16, lost, max_age, o)), (max_age, pcm16)
    single = torch.zeros_like(lost)                                       # every third row lost: all recovered
    single[:, 0:K:3] = True
    fused = codec.decode_packed(data, index, lost=single, max_age=8, redundant_at=o)
    assert same_bits(fused, codec.decode_packed(data, _substituted(index, single, o)))
    assert not same_bits(fused, codec.decode_packed(data, index, lost=single, max_age=8))


@gpu
def test_recover_redundant_at_cases(monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, data, index = _slots(2, 7)
    rb = codec.row_bytes
    lost = _patterns(3, 7, 2, 8)["30 %"]
    lost[0, 5, 0], lost[0, 6, 0] = 1, 0                                   # a recovered row whose copy is in the last slot
    # off the 4-byte phase: the bytes shifted by 3, the primary rows still read from their aligned copies in front
    shifted = torch.cat([data, torch.zeros(3, dtype=torch.uint8, device="cuda"), data])
    a = _hold(codec, shifted, index, lost, 8, rb + data.numel() + 3, "off the phase")
    assert same_bits(a, _hold(codec, data, index, lost, 8, rb, "aligned", formats=(False,)))
    # so large that the last rows' copies start past nbytes (silence), and any odd value
    for o in (data.numel() - int(index[0, 6, 0]) - 5, data.numel(), 2 ** 31 - 1, 1, rb + 2):
        _hold(codec, data, index, lost, 8, o, "redundant_at %d" % o, formats=(False,))
    # a permuted, strided index: frame f + 1 is whatever the index says
    perm = index[:, torch.tensor([3, 0, 6, 1, 5, 2, 4], device="cuda")]
    wide = torch.stack([perm, perm + 1], dim=-1)[..., 0]
    assert not wide.is_contiguous()
    b = _hold(codec, data, perm.contiguous(), lost, 8, rb, "permuted")
    assert same_bits(codec.decode_packed(data, wide, lost=_dev(lost), max_age=8, redundant_at=rb), b)
    # a marked copy decodes as a marked row does: NaN in the two blocks it covers
    tight = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    base, off, adv, adv_index, _ = _adversarial()
    out = tight.protect_packed_rows(_dev(adv), _dev(adv_index), 320, True)
    assert not bool(out[3][0, 2, 0])
    l2 = np.zeros((1, 6, 2), dtype=np.uint8)
    l2[0, 1, 0] = 1
    pcm = _hold(tight, out[0], out[1], l2, 8, tight.row_bytes, "marked copy")
    assert bool(torch.isnan(pcm.view(1, 7, N0, 2)[0, 1:3, :, 0]).all())


@gpu
def test_recover_fallbacks(monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    for N, C in ((512, 3), (1024, 2)):
        base = audiocodec_amd.AudioCodec(48000, N)
        codec = base.with_row_budget(1365)
        x = _pcm(N, C, 2, 5, seed=N + C, inject=False)
        data, index, _ = base.with_row_budget(2730).encode_packed_rows(x)
        data, index = codec.protect_packed_rows(data, index, 400)[:2]
        lost = _lost(6, [0, 2, 3, 5], 2, C)
        if N == 1024:
            monkeypatch.setenv(NOFUSE, "1")
        assert codec.decode_packed_launches(C) != 1
        o = codec.row_bytes
        src, age = np_recover_src_index(index.cpu().numpy(), lost, data.numel(), 8, o)
        codes, sf = codec.psy.unpack(data, _dev(src))
        ref = codec.decode_quantized(codes, _dev(np_fade(sf.cpu().numpy(), age)))
        assert same_bits(codec.decode_packed(data, index, lost=_dev(lost), max_age=8, redundant_at=o), ref)
        assert int(np_recover_plan(lost, 8)[2].sum()) == 2 * 2 * C


@gpu
def test_recover_c_abi(monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    lib = _lib.load()
    codec, data, index = _slots(2, 7)
    dev = data.device
    lost = _dev(_patterns(3, 7, 2, 8)["two runs"])
    rows = _lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr())
    x = torch.full((3, 8 * N0, 2), 7.0, device="cuda")

    def call(struct):
        st = lib.ac_decode_quantized(codec.mdct._plan(dev), codec.psy._plan(dev), ctypes.addressof(rows), None,
                                     ctypes.c_void_p(x.data_ptr()), None, ctypes.addressof(struct), 3, 7, 2, None)
        torch.cuda.synchronize()
        return st
    RED, o = _lib.AC_CONCEAL_REDUNDANT, codec.row_bytes
    for bad in (_lib.ConcealRedundant(lost.data_ptr(), 32 | RED, o), _lib.ConcealRedundant(lost.data_ptr(), 255 | RED, o),
                _lib.ConcealRedundant(lost.data_ptr(), 8 | RED, 0), _lib.ConcealRedundant(lost.data_ptr(), 8 | RED, 2 ** 31),
                _lib.ConcealRedundant(lost.data_ptr(), 8 | RED, -4), _lib.ConcealRedundant(None, 8 | RED, o),
                _lib.ConcealRedundant(lost.data_ptr(), -1, o), _lib.ConcealRedundant(lost.data_ptr(), 32, o)):
        assert call(bad) == _lib.AC_EINVAL and lib.ac_last_error(), (bad.max_age, bad.redundant_at)
    assert int((x != 7.0).sum()) == 0                                     # the refused calls wrote nothing
    # the bit absent: today's result, whatever lies behind the first two members
    assert call(_lib.ConcealRedundant(lost.data_ptr(), 8, o)) == _lib.AC_OK
    assert same_bits(x, codec.decode_packed(data, index, lost=lost, max_age=8))
    assert call(_lib.ConcealRedundant(lost.data_ptr(), 8 | RED, o)) == _lib.AC_OK, lib.ac_last_error()
    want = codec.decode_packed(data, index, lost=lost, max_age=8, redundant_at=o)
    assert same_bits(x, want) and not same_bits(want, codec.decode_packed(data, index, lost=lost, max_age=8))
    with _env(NOFUSE):
        assert call(_lib.ConcealRedundant(lost.data_ptr(), 8 | RED, o)) == _lib.AC_EUNSUPPORTED


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
def test_recover_graph_capture(route, monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, data, index = _slots(2, 7)
    data, o = data.clone(), codec.row_bytes
    lost = _dev(_patterns(3, 7, 2, 8)["30 %"])
    call = ((lambda d: codec.decode_packed(d, index, lost=lost, max_age=8, redundant_at=o)) if route == "fused"
            else (lambda d: _recover_composition(codec, d, index, False, lost, 8, o)))
    call(data)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(data)
    data.copy_(data.flip(0).view(-1, 4).flip(0).reshape(-1))              # other bytes, read as damaged rows
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out, call(data.clone()))


@gpu
@pytest.mark.parametrize("check", ["delayed_producer", "busy_default"])
def test_recover_stream_contract(harness, check, monkeypatch):
    monkeypatch.delenv(NOFUSE, raising=False)
    codec, data, index = _slots(2, 7)
    lost, o = _dev(_patterns(3, 7, 2, 8)["30 %"]), codec.row_bytes
    torch.cuda.synchronize()
    fn = lambda d, i, l: codec.decode_packed(d, i, lost=l, max_age=8, redundant_at=o)   # noqa: E731
    getattr(harness, check)("cbr.decode_packed[1024-2,redundant_at]", ([data, index, lost], fn))


# ---- GPU: the chain -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pcm16", [False, True])
def test_chain_encode_protect_lose_recover(pcm16, monkeypatch):
    """128 kbit/s rows -> 64 kbit/s slots with a 16 kbit/s copy -> a decode that lost rows.  A recovered frame is the R2
    transrate of the input row: with the recovered rows read from ``transrate_packed_rows`` at R2 directly, the blocks they
    cover are the same bits."""
    monkeypatch.delenv(NOFUSE, raising=False)
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_bitrate(128000), base.with_bitrate(64000)
    R2 = base.row_bits_for_bitrate(16000)
    assert (src.row_bits, dst.row_bits, R2) == (2730, 1365, 341)
    B, K, C = 2, 9, 2
    data, index, _ = src.encode_packed_rows(_pcm(N0, C, B, K, seed=64, inject=False))
    out, idx, fits, red_fits = dst.protect_packed_rows(data, index, R2)
    assert bool(fits.all()) and bool(red_fits.all())
    lost = np.zeros((B, K + 1, C), dtype=np.uint8)
    lost[0, 3, 0] = lost[1, 0, 1] = lost[1, 6, :] = 1                     # isolated: both neighbours arrived
    lost[0, 7:9, 1] = 1                                                   # a run of 2
    lost_d, o = _dev(lost), dst.row_bytes
    got = dst.decode_packed(out, idx, pcm16, lost=lost_d, max_age=8, redundant_at=o)
    assert same_bits(got, _recover_composition(dst, out, idx, pcm16, lost_d, 8, o))
    red = dst.with_row_budget(R2).transrate_packed_rows(data, index)
    both = torch.cat([out, red[0]])
    direct = torch.where(lost_d != 0, red[1] + out.numel(), idx)
    want = dst.decode_packed(both, direct, pcm16)
    blocks = lambda t: t.view(B, K + 2, N0, C)                            # noqa: E731
    for b, f, c in ((0, 3, 0), (1, 0, 1), (1, 6, 0), (1, 6, 1)):
        assert same_bits(blocks(got)[b, f:f + 2, :, c], blocks(want)[b, f:f + 2, :, c]), (b, f, c)
        assert not same_bits(blocks(got)[b, f:f + 2, :, c], blocks(dst.decode_packed(out, idx, pcm16))[b, f:f + 2, :, c])
