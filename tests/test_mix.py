"""Mixing the packed rows of several sources at a bitrate, without decoding:
``PsychoacousticModel.mix_to_budget``, ``AudioCodec.mix_packed_rows`` (the ``AC_IN_PACKED | AC_EMIT_PACKED | AC_IN_MIX`` form of
``ac_encode_fused_ex``) and the one launch at filters_n = 1024 that reads S rows, sums them bin by bin, searches the offset and
packs the sum in one wave (k_mix_p).

Every GPU comparison of the one launch is ``torch.equal`` against the composition -- ``unpack`` and ``dequantize`` per source,
float32 adds in source order, ``quantize_to_budget`` under the threshold crit(s0), rows longer than their slot marked, ``ac_pack``
at the fixed row starts into zero-filled data -- which runs everywhere while ``AC_MIX_NOFUSE=1`` is set; the composition is
compared byte for byte with the numpy restatement of ``mix_reference.py``.  Before any kernel result is compared, numpy alone
must show that the input exercises the rules (``_conditions``).

Seeded defect (a scratch build, not committed): with the fold of ``s0`` in ``mix_row`` taken from the first source only, 30
of the 48 GPU cases of this file fail and no CPU test does (the CPU tests hold the numpy restatement and the interface, not
the kernel): the 12 cases of test_mix_fused_composition_numpy with S >= 2, test_heterogeneous_sources,
test_gains_at_the_clamp, test_active_patterns, test_hostile_input, the 10 cases of test_band_layouts, test_chip_filling and
test_c_abi on the ``torch.equal`` of the fused bytes against the composition's, and both cases of test_end_to_end on the
bound of rule 6.  The S = 1 cases, the sizes and the S = 9 that run the composition, and the tests that compare a route
with itself (stream contract, graph capture, chunks) pass, as they must.
"""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib
from conftest import ROOT

import fused_layouts as fl
from mix_reference import mix_brute, mix_budget, mix_fast, mix_spectrum, np_mix, threshold_of
from pack_reference import np_canon, np_pack, np_row_bits, np_unpack, np_widths
from pack_rows_reference import marked_row, np_rows_from_codes, row_bytes
from rate_reference import quantize_budget
from test_encode_cbr import _input
from test_encode_quantized_fused import _pcm, _same, _where
from test_quantizer import np_dequantize, np_offsets, np_quantize, np_step
from test_rate_control import EX_OFF, EX_THR, EX_X
from test_transrate import _random_rows
from transrate_reference import np_transrate

gpu = pytest.mark.gpu
N0, M0 = 1024, 64
CAP = _lib.AC_PACK_ROWS_MAX_BITS
HEADER = os.path.join(ROOT, "include", "audiocodec_amd.h")
SHAPES = [(1, 1, 1), (2, 3, 2), (3, 5, 1), (2, 2, 3)]          # (B, K, C): 2, 16, 18 (tail waves in the last workgroup), 18 rows
BUDGETS = [1365, 682, 320, CAP]                                # from sources held at 2730 bits
GAINS = {1: [0], 2: [1, -1], 3: [0, 254, -254], 8: [0, 1, -1, 7, -12, 40, -40, 130]}


def _eq(a, b, what=""):
    for i, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg="%s, output %d" % (what, i))


# ---- CPU: the definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,N,M", [(44100, 256, 48), (48000, 128, 64)])
def test_consequences_of_the_definition(sr, N, M):
    """(a) .. (e) of section 8h on random non-canonical rows with -128 bands, at three budgets; both searches agree."""
    rng = np.random.default_rng(N + M)
    off = np_offsets(sr, N, M)
    A, Bq = _random_rows(rng, off, 2, 3, 2), _random_rows(rng, off, 2, 3, 2)
    dA, iA = np_pack(*A, off)
    dB, iB = np_pack(*Bq, off)
    seen = set()
    for R in (5 * M + 40, 900, 16 * N + 13 * M):
        # (a) one source at gain 0 is the transrating call, byte for byte, flags and offsets included
        _eq(np_mix([(dA, iA)], off, N, R), np_transrate(dA, iA, off, N, R), "(a) at %d" % R)
        # (b) two sources commute
        ab = np_mix([(dA, iA), (dB, iB)], off, N, R, [3, -5])
        _eq(ab, np_mix([(dB, iB), (dA, iA)], off, N, R, [-5, 3]), "(b) at %d" % R)
        seen |= set(np.unique(ab[3]).tolist())
        # (c) an inactive source, or a source of all-zero rows, changes nothing, whatever its gain
        act = np.ones((3, 2, 3, 2), np.uint8)
        act[1] = 0
        zero = (np.zeros_like(A[0]), A[1])
        _eq(mix_budget([A, Bq, zero], off, R, [3, 99, -200], act), mix_budget([A], off, R, [3]), "(c) at %d" % R)
        # (d) the quantiser under thr = crit(s0) gives the same codes, scale factors, offsets and rows
        Xh, s0, _ = mix_spectrum([A, Bq], off, [3, -5])
        assert (s0 == -128).any() and np.isnan(Xh).any()
        m = mix_budget([A, Bq], off, R, [3, -5])
        q = quantize_budget(Xh, threshold_of(s0, off), off, R)
        _eq(q, m, "(d) at %d" % R)
        _eq(np_rows_from_codes(q[0], q[1], q[3], off, R), ab[:3], "(d) rows at %d" % R)
        _eq(mix_brute([A, Bq], off, R, [3, -5]), mix_fast([A, Bq], off, R, [3, -5]), "searches at %d" % R)
    assert len(seen) >= 3
    # (e) a source mixed with its negation (no -128 band, no -32768: neither has a negation): zero bytes, fits, offset 0
    q, s = np_canon(*A, off)
    q, s = np.maximum(q, -32767), np.where(s == -128, 5, s).astype(np.int8)
    dP, iP = np_pack(q, s, off)
    dM, iM = np_pack(-q, s, off)
    out = np_mix([(dP, iP), (dM, iM)], off, N, 900)
    assert not out[0].any() and out[2].all() and not out[3].any() and (out[4] == 5 * M).all()


def test_worked_example_mixed_with_itself_and_its_negation():
    """Section 8c's example (M = 4) mixed with itself: the sum is twice the spectrum, one doubling is four scale-factor units,
    so every offset of section 8e's table moves up by 4 and the codes and lengths repeat.  The table is the brute-force search's."""
    c0, s0 = np_quantize(EX_X, EX_THR, EX_OFF)
    assert np_row_bits(c0, s0, EX_OFF).ravel()[0] == 100
    table = {120: (0, 108, [0, -30, -22, -44], [108, -72, 90, -64, 4, 40, 0, -82]),
             108: (0, 108, [0, -30, -22, -44], [108, -72, 90, -64, 4, 40, 0, -82]),
             100: (4, 100, [0, -26, -18, -40], [54, -36, 45, -32, 2, 20, 0, -41]),
             96: (7, 94, [0, -23, -15, -37], [32, -21, 27, -19, 1, 12, 0, -24]),
             64: (24, 62, [0, -6, 2, -20], [2, -1, 1, -1, 0, 1, 0, -1]),
             56: (30, 32, [0, 0, 8, -14], [1, 0, 0, 0, 0, 0, 0, 0]),
             20: (32, 20, [0, 2, 10, -12], [0, 0, 0, 0, 0, 0, 0, 0])}
    for R, (k, bits, sf, codes) in table.items():
        brute = mix_brute([(c0, s0), (c0, s0)], EX_OFF, R)
        _eq(brute, mix_fast([(c0, s0), (c0, s0)], EX_OFF, R), "searches at %d" % R)
        assert (int(brute[2].ravel()[0]), int(brute[3].ravel()[0])) == (k, bits), R
        assert brute[1].ravel().tolist() == sf and brute[0].ravel().tolist() == codes, R
    neg = mix_brute([(c0, s0), (-c0, s0)], EX_OFF, 20)
    assert not neg[0].any() and int(neg[2].ravel()[0]) == 0 and int(neg[3].ravel()[0]) == 20
    data, index = np_pack(c0, s0, EX_OFF)
    nd, ni = np_pack(-c0, s0, EX_OFF)
    out = np_mix([(data, index), (nd, ni)], EX_OFF, 8, 20)
    assert not out[0].any() and out[2].all()
    # a gain of +4 on one source alone is that source doubled: the self-mix at R = 100 is the source's own row
    one = mix_brute([(c0, s0)], EX_OFF, 120, [4])
    assert one[0].ravel().tolist() == c0.ravel().tolist() and one[1].ravel().tolist() == [0, -26, -18, -40]


def test_a_saturating_sum_never_fits():
    """Two rows of +-32767 at sf 127: the sum's codes clamp at +-32767 at every offset (section 8a rule 4; documented, not
    worked round), its 16-bit widths push the search to 254 and the row is marked."""
    codes = np.full((1, 1, 8, 1), 32767, np.int16)
    codes[0, 0, 1::2] = -32767
    sf = np.full((1, 1, 4, 1), 127, np.int8)
    rc, rs, offset, bits = mix_budget([(codes, sf), (codes, sf)], EX_OFF, 20)
    assert rs.ravel().tolist() == [0, 127, 127, 127] and int(offset.ravel()[0]) == 254
    assert int(bits.ravel()[0]) == 20 + 3 * 8 + 16 * 8 > 8 * row_bytes(20)
    np.testing.assert_array_equal(rc, codes)                                # twice 32767 steps, clamped
    data, index = np_pack(codes, sf, EX_OFF)
    out = np_mix([(data, index), (data, index)], EX_OFF, 8, 20)
    assert not out[2].any() and int(out[3].ravel()[0]) == 254
    np.testing.assert_array_equal(out[0], marked_row(4, 20))
    Xh = mix_spectrum([(codes, sf), (codes, sf)], EX_OFF)[0]
    assert np.isfinite(Xh).all() and np.isfinite(np.float32(8 * 32767) * np_step(127))


def test_a_marked_source_row_comes_out_marked_with_fits():
    """A marked row is a row of -128 bands: every band of the sum is bad whatever the other source holds."""
    off = np_offsets(48000, N0, M0)
    marked = np_pack(np.zeros((1, 1, N0, 1), np.int16), np.full((1, 1, M0, 1), -128, np.int8), off)
    np.testing.assert_array_equal(marked[0], marked_row(M0, 320))            # (dense: the 40 bytes of its 320 bits)
    rng = np.random.default_rng(3)
    other = np_pack(rng.integers(-50, 51, (1, 1, N0, 1)).astype(np.int16), rng.integers(-40, 0, (1, 1, M0, 1)).astype(np.int8), off)
    for srcs in ([marked, other], [other, marked], [marked]):
        out = np_mix(srcs, off, N0, 1365)
        assert out[2].all() and int(out[3].ravel()[0]) == 0
        np.testing.assert_array_equal(out[0], marked_row(M0, 1365))
    act = np.array([0, 1], np.uint8).reshape(2, 1, 1, 1)                    # ... unless the marked row is inactive
    _eq(np_mix([marked, other], off, N0, 1365, None, act), np_mix([other], off, N0, 1365))


# ---- CPU: header, library, Python validation ------------------------------------------------------------------------------
def test_header_declares_the_flag_the_struct_and_the_launch_query():
    text = open(HEADER).read()
    assert re.search(r"\bAC_IN_MIX\s*=\s*1024\b", text)
    assert re.search(r"#define\s+AC_MIX_MAX_SOURCES\s+8\b", text)
    m = re.search(r"typedef\s+struct\s+ac_mix_rows\s*\{(.*?)\}\s*ac_mix_rows\s*;", text, flags=re.S)
    assert m, "ac_mix_rows is not declared"
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["int32_t sources_n", "const struct ac_packed_rows* src", "const int32_t* gain", "const uint8_t* active"], fields
    m = re.search(r"AC_API\s+int\s+ac_mix_launches\s*\(([^;]*)\)\s*;", text)
    assert m and "stream" not in m.group(1) and m.group(1).count(",") == 2, m and m.group(1)
    assert re.search(r"#define\s+AC_VERSION\s+171\b", text)


def test_library_exports_the_launch_query():
    lib = _lib.load()
    assert "ac_mix_launches" in _lib.PROTOTYPES and callable(lib.ac_mix_launches)
    assert lib.ac_mix_launches(None, 2, 2) == 0
    assert lib.ac_version() == 171
    assert _lib.AC_IN_MIX == 1024 and _lib.AC_MIX_MAX_SOURCES == 8


def test_ctypes_mirror_has_the_headers_layout():
    Q = _lib.MixRows
    assert [f[0] for f in Q._fields_] == ["sources_n", "src", "gain", "active"]
    assert (Q.sources_n.offset, Q.src.offset, Q.gain.offset, Q.active.offset) == (0, 8, 16, 24) and ctypes.sizeof(Q) == 32
    assert ctypes.sizeof(_lib.PackedRows) == 24                             # the stride of src


def test_python_interface_validates_its_arguments():
    base = audiocodec_amd.AudioCodec(48000, N0)
    data, index = torch.zeros(64, dtype=torch.uint8), torch.zeros((1, 1, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"with_bitrate\(\)"):
        base.mix_packed_rows([(data, index)])
    cbr = base.with_bitrate(64000)
    with pytest.raises(ValueError, match="at least one source"):
        cbr.mix_packed_rows([])
    with pytest.raises(ValueError, match="at least one source"):
        base.psy.mix_to_budget([], None, 1365)
    for bad in ([1.0], [True], [None], ["3"]):
        with pytest.raises(TypeError, match="gain"):
            cbr.mix_packed_rows([(data, index)], gains=bad)
    for bad in ([255], [-255], [0, 0]):
        with pytest.raises(ValueError, match="gain"):
            cbr.mix_packed_rows([(data, index)], gains=bad)
    for bad in ((data.to(torch.int8), index), (data, index.to(torch.int32)), (data.view(8, 8), index), (data, index[0]),
                (data, index)):                               # the last: host tensors
        with pytest.raises(ValueError):
            cbr.mix_packed_rows([bad])
    with pytest.raises(TypeError):
        cbr.mix_packed_rows([(data.numpy(), index)])
    with pytest.raises(NotImplementedError, match="float32"):
        audiocodec_amd.AudioCodec(48000, N0, compute_dtype=torch.float64).mix_packed_rows([(data, index)])
    assert cbr.mix_packed_rows_launches.__kwdefaults__ is None               # sources_n is required, by keyword
    with pytest.raises(TypeError):
        cbr.mix_packed_rows_launches(2)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
class _nofuse:
    """AC_MIX_NOFUSE=1 (read per call) around a block."""

    def __enter__(self):
        os.environ["AC_MIX_NOFUSE"] = "1"

    def __exit__(self, *exc):
        del os.environ["AC_MIX_NOFUSE"]
        return False


def _composition(codec, sources, gains=None, active=None, return_offset=True):
    with _nofuse():
        assert codec.mix_packed_rows_launches(sources[0][1].shape[2], sources_n=len(sources)) == 2 * len(sources) + 2
        return codec.mix_packed_rows(sources, gains, active, return_offset)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _x(B, K, C, seed, N=N0, flip=False):
    """test_transrate's input: test_encode_cbr's with its injections where the shape allows them (B >= 3, K >= 4), elsewhere
    the ramped noise with block 0 of clip 0 zeroed; ``flip``: the ramp runs down, so that the louder source changes along a clip."""
    inject = B >= 3 and K >= 4
    x = _input(C, B, K, seed, inject, N)
    if not inject and K >= 2:
        x[0, :N] = 0.0
    return x.flip(1).contiguous() if flip else x


def _sources(base, B, K, C, S, seed, R=2730):
    """S sources of the shape at R bits a row: seeds apart; every second one has its ramp reversed -- the louder source changes
    along a clip, so each decides some s0 -- and carries the finite part of the source before it, so that where that part
    dominates the two add in phase and a band's codes grow past both sources'."""
    src = base.with_row_budget(R)
    xs = []
    for i in range(S):
        x = _x(B, K, C, seed + 11 * i, flip=bool(i & 1))
        if i & 1:
            x = x + torch.nan_to_num(xs[-1], nan=0.0, posinf=0.0, neginf=0.0).clamp_(-1.0, 1.0)
        xs.append(x)
    return [src.encode_packed_rows(x)[:2] for x in xs]


def _unpacked(sources, off, N=N0):
    return [np_unpack(d.cpu().numpy(), i.cpu().numpy(), off, N) for d, i in sources]


def _reference(rows, off, R, gains=None, active=None):
    """np_mix on rows that are unpacked already: (data, index, fits, offset, bits)."""
    rc, rs, offset, bits = mix_budget(rows, off, R, gains, None if active is None else active.cpu().numpy())
    return np_rows_from_codes(rc, rs, bits, off, R) + (offset, bits)


def _three_ways(dst, sources, rows, off, gains=None, active=None, what=""):
    """numpy, the composition and the one launch on the same sources: returns the reference."""
    ref = _reference(rows, off, dst.row_bits, gains, active)
    comp = _composition(dst, sources, gains, active)
    C, S = sources[0][1].shape[2], len(sources)
    assert dst.mix_packed_rows_launches(C, sources_n=S) == 1
    fused = dst.mix_packed_rows(sources, gains, active, True)
    for name, g, c, r in zip(("data", "index", "fits", "offset"), fused, comp, ref):
        np.testing.assert_array_equal(c.cpu().numpy(), r, err_msg="%s %s" % (name, what))
        assert torch.equal(g, c), (name, what, _where(g, c))
    return ref


def _conditions(rows, off, gains, ref_cap, refs):
    """What numpy alone must show before a kernel is asked (two sources or more, 16 rows or more): across the budgets at
    least 3 distinct offsets and a row that fits only above offset 0; for every one of the first two sources a band whose
    s0 is that source's alone; a band whose width in the mix exceeds its width in every source."""
    offsets = np.concatenate([r[3].ravel() for r in refs])
    assert len(np.unique(offsets)) >= 3, np.unique(offsets)
    assert any(int(((r[3] > 0) & r[2]).sum()) >= 1 for r in refs), "no row that fits only at k > 0"
    _, s0, gs = mix_spectrum(rows, off, gains)
    for i in range(2):
        others = np.delete(gs, i, axis=0).max(axis=0)
        assert int(((gs[i] > others) & (s0 == gs[i])).sum()) >= 1, "no band whose s0 comes from source %d" % i
    wm = np_widths(*np_unpack(ref_cap[0], ref_cap[1], off, N0), off)
    ws = np.stack([np_widths(*np_canon(q, s, off), off) for q, s in rows]).max(axis=0)
    assert int(((wm <= 16) & (ws <= 16) & (wm > ws)).sum()) >= 1, "no band wider in the mix than in every source"


@gpu
@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("B,K,C", SHAPES)
def test_mix_fused_composition_numpy(B, K, C, S):
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    sources = _sources(base, B, K, C, S, C + 2 * B + K)
    rows = _unpacked(sources, off)
    gains = GAINS[S]
    refs = {R: _reference(rows, off, R, gains) for R in BUDGETS}
    for R in BUDGETS:
        print("S = %d to %d: %d rows, offsets %s, %d unfit" % (S, R, refs[R][3].size, np.unique(refs[R][3]).tolist(), int((~refs[R][2]).sum())))
    if S == 2 and B * (K + 1) * C >= 16:                                     # (S = 3, 8: gains of +-254 and 130 decide every s0)
        _conditions(rows, off, gains, refs[CAP], [refs[R] for R in BUDGETS])
    if S == 1:
        _eq(refs[1365][:4], np_transrate(sources[0][0].cpu().numpy(), sources[0][1].cpu().numpy(), off, N0, 1365)[:4], "(a)")
    for R in BUDGETS:
        dst = base.with_row_budget(R)
        _three_ways(dst, sources, rows, off, gains, None, "S = %d at %d" % (S, R))
        assert len(dst.mix_packed_rows(sources, gains)) == 3
    if S == 1:                                                              # (a) on the device: the transrating call's bytes
        dst = base.with_row_budget(682)
        for g, t in zip(dst.mix_packed_rows(sources, None, None, True), dst.transrate_packed_rows(*sources[0], True)):
            assert torch.equal(g, t)
    if S == 2:                                                              # (b) on the device
        dst = base.with_row_budget(682)
        for g, t in zip(dst.mix_packed_rows(sources, gains, None, True), dst.mix_packed_rows(sources[::-1], gains[::-1], None, True)):
            assert torch.equal(g, t)


@gpu
def test_heterogeneous_sources():
    """A dense encode_packed result, 2730-bit fixed-stride rows, protected slots and a permuted index, mixed with each other."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    B, K, C = 3, 5, 2
    dense = base.encode_packed(_x(B, K, C, 41))
    fixed = base.with_row_budget(2730).encode_packed_rows(_x(B, K, C, 42, flip=True))[:2]
    prot = base.with_row_budget(1365).protect_packed_rows(*base.with_row_budget(2730).encode_packed_rows(_x(B, K, C, 43))[:2], 640)[:2]
    d4, i4 = base.with_row_budget(2048).encode_packed_rows(_x(B, K, C, 44))[:2]
    perm = (d4, i4.reshape(-1)[torch.randperm(i4.numel(), generator=torch.Generator().manual_seed(4)).cuda()].view(i4.shape).contiguous())
    sources = [dense, fixed, prot, perm]
    rows = _unpacked(sources, off)
    gains = [0, -2, 4, 1]
    refs = [_three_ways(base.with_row_budget(R), sources, rows, off, gains, None, "to %d" % R) for R in (1365, 682)]
    assert len(np.unique(np.concatenate([r[3].ravel() for r in refs]))) >= 3 and int(refs[0][3].max()) > 0


@gpu
def test_gains_at_the_clamp():
    """+-254 and gains that meet the clamp of the scale factor at +-127 from both sides."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    sources = _sources(base, 2, 3, 2, 2, 9)
    rows = _unpacked(sources, off)
    g0 = mix_spectrum(rows, off)[2]                                          # the stored scale factors of each source
    hi, lo = int(g0[0].max()), int(g0[1][g0[1] > -129].min())              # the largest of source 0, the smallest of source 1
    # ... the last pair stops one unit short of both ends: no scale factor is clamped
    for gains in ([254, -254], [-254, 254], [127 - hi, -127 - lo], [128 - hi, -128 - lo], [127 - hi - 1, -127 - lo + 1]):
        gs = mix_spectrum(rows, off, gains)[2]
        ends = (int(gs[0].max()), int(gs[1][gs[1] > -129].min()))
        assert ends == ((126, -126) if gains[0] == 127 - hi - 1 else (127, -127) if gains[0] > 0 else ends), (gains, ends)
        assert gains[0] > 0 or (int(gs[0][gs[0] > -129].max()) == -127 and int(gs[1].max()) == 127)
        for R in (1365, CAP):
            _three_ways(base.with_row_budget(R), sources, rows, off, gains, None, "gains %s at %d" % (gains, R))


@gpu
def test_active_patterns():
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    B, K, C, S = 2, 3, 2, 3
    sources = _sources(base, B, K, C, S, 23)
    rows = _unpacked(sources, off)
    gains = [2, -3, 5]
    dst = base.with_row_budget(1365)
    F = K + 1
    # all off: slots of zeros
    none = torch.zeros((S, B, F, C), dtype=torch.uint8, device="cuda")
    ref = _three_ways(dst, sources, rows, off, gains, none, "all off")
    assert not ref[0].any() and ref[2].all() and not ref[3].any()
    # one source off: the mix without it; as bool and as uint8 with values other than 1
    one = torch.ones((S, B, F, C), dtype=torch.uint8, device="cuda")
    one[1] = 0
    ref = _three_ways(dst, sources, rows, off, gains, one, "one off")
    _eq(ref, _reference([rows[0], rows[2]], off, 1365, [2, 5]), "one off against the mix without it")
    got = dst.mix_packed_rows(sources, gains, one.bool(), True)
    other = dst.mix_packed_rows([sources[0], sources[2]], [2, 5], None, True)
    for g, t in zip(got, other):
        assert torch.equal(g, t)
    assert torch.equal(dst.mix_packed_rows(sources, gains, one * 200, True)[0], got[0])
    # a source that is off is never read: its data may be anything, its index out of range
    junk = (torch.full_like(sources[1][0], 0xFF), torch.full_like(sources[1][1], 1 << 45))
    assert torch.equal(dst.mix_packed_rows([sources[0], junk, sources[2]], gains, one, True)[0], got[0])
    # a checkerboard over (source, row)
    b, f, c = np.meshgrid(np.arange(B), np.arange(F), np.arange(C), indexing="ij")
    board = _dev(np.stack([((b + f + c + i) % 2).astype(np.uint8) for i in range(S)]))
    ref = _three_ways(dst, sources, rows, off, gains, board, "checkerboard")
    assert int(ref[3].max()) > 0


def _upload(data, index):
    return _dev(np.asarray(data, dtype=np.uint8)), _dev(np.asarray(index, dtype=np.int64))


@gpu
def test_hostile_input():
    """Damaged and truncated data, row starts that are negative, past the end or off the 4-byte phase, marked rows, and the
    NaN / Inf-carrying input of test_encode_cbr._input (in _x at this shape)."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    B, K, C = 3, 5, 2
    good = _sources(base, B, K, C, 2, 61)
    rows_good = _unpacked(good, off)
    assert sum(int((r[1] == -128).sum()) for r in rows_good) >= 1              # the NaN / Inf frames arrived as -128 bands
    dst = base.with_row_budget(1365)
    data, index = (t.cpu().numpy() for t in good[1])

    def run(d, i, what):
        srcs = [good[0], _upload(d, i)]
        return _three_ways(dst, srcs, [rows_good[0], np_unpack(d, i, off, N0)], off, [1, -1], None, what)

    # widths 17 .. 30 read as 31, and a stored scale-factor byte of -128
    bits = np.unpackbits(data, bitorder="little")
    start = int(index[0, 2, 0]) * 8
    for j, wv in ((3, 17), (10, 30), (40, 23)):
        bits[start + 5 * j:start + 5 * j + 5] = [(wv >> k) & 1 for k in range(5)]
    start = int(index[1, 1, 1]) * 8 + 5 * M0
    bits[start:start + 8] = [0, 0, 0, 0, 0, 0, 0, 1]
    run(np.packbits(bits, bitorder="little"), index, "damaged")
    rng = np.random.default_rng(8)
    run(rng.integers(0, 256, data.shape).astype(np.uint8), index, "random bytes")
    for cut in (int(index[2, 5, 1]) + 100, int(index[2, 5, 1]) + 13, int(index[2, 3, 0]) + 2):
        run(data[:cut], index, "truncated at %d" % cut)
    odd = index.copy()
    odd[0, 0, 0], odd[0, 1, 1], odd[0, 2, 0], odd[0, 3, 1], odd[0, 4, 0] = -7, len(data) + 1000, index[0, 2, 0] + 1, -(1 << 50), len(data) - 3
    odd[0, 5, 0], odd[1, 0, 0], odd[1, 0, 1] = (1 << 40), index[1, 0, 0] + 2, index[1, 0, 1] + 3
    run(data, odd, "odd row starts")
    # marked rows: every row of the second source that the 320-bit budget cannot hold
    small = base.with_row_budget(320).encode_packed_rows(_x(B, K, C, 62))
    assert int((~small[2]).sum()) >= 1
    d, i = (t.cpu().numpy() for t in small[:2])
    ref = run(d, i, "marked rows")
    unfit = ~small[2].cpu().numpy()
    assert ref[2][unfit].all()                                              # marked in, marked-looking out, fits 1
    rb = dst.row_bytes
    for r in np.flatnonzero(unfit.ravel()):
        np.testing.assert_array_equal(ref[0][r * rb:(r + 1) * rb], marked_row(M0, 1365))


@gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", fl.LAYOUTS, ids=fl.LAYOUT_IDS)
def test_band_layouts(layout, C):
    """One-bin bands, granules that straddle bands and empty bands (fused_layouts.LAYOUTS), on its ``tonal`` input."""
    sr, alpha = fl.resolve(layout)
    base = audiocodec_amd.AudioCodec(sr, N0, alpha=alpha)
    off = base.psy.scale_band_offsets
    x = torch.from_numpy(fl.tonal(C)).cuda()
    src = base.with_row_budget(2730)
    sources = [src.encode_packed_rows(x)[:2], src.encode_packed_rows((0.5 * x.flip(1)).contiguous())[:2]]
    rows = _unpacked(sources, off)
    for R in (1365, 400):
        ref = _three_ways(base.with_row_budget(R), sources, rows, off, [0, 3], None, "to %d" % R)
        assert int((ref[3] > 0).sum()) >= 1 and len(np.unique(ref[3])) >= 2


def _check_mix_to_budget(psy, rows, R, gains, active=None):
    """mix_to_budget against the numpy restatement, bit for bit; returns the reference."""
    off = psy.scale_band_offsets
    got = psy.mix_to_budget([(_dev(q), _dev(s)) for q, s in rows], gains, R, None if active is None else _dev(active))
    ref = mix_budget(rows, off, R, gains, active)
    B, F, N, C = rows[0][0].shape
    assert got[0].dtype == torch.int16 and got[1].dtype == torch.int8 and got[1].shape == rows[0][1].shape
    assert got[2].dtype == torch.int16 and got[2].shape == (B, F, C) and got[3].dtype == torch.int32
    for name, g, r in zip(("offset", "row_bits", "sf", "codes"), (got[2], got[3], got[1], got[0]), (ref[2], ref[3], ref[1], ref[0])):
        np.testing.assert_array_equal(g.cpu().numpy(), r, err_msg="%s at R = %d" % (name, R))
    return ref


@gpu
@pytest.mark.parametrize("sr,N,M,C", [(48000, 2048, 64, 2), (48000, 960, 64, 1), (44100, 256, 48, 3)])
def test_mix_to_budget_and_the_composition_at_other_sizes(sr, N, M, C):
    """mix_to_budget serves every plan the quantiser serves: non-canonical random rows against numpy, then the rows-to-rows
    composition (the query is not 1) against np_mix."""
    base = audiocodec_amd.AudioCodec(sr, N, bark_bands_n=M)
    off = base.psy.scale_band_offsets
    rng = np.random.default_rng(N + C)
    rows = [_random_rows(rng, off, 2, 3, C) for _ in range(3)]
    for q, s in rows[1:]:
        s[...] = np.where(s == -128, -128, np.clip(s.astype(np.int32) // 4 - 20, -127, 127)).astype(np.int8)   # levels that meet
    active = (rng.random((3, 2, 3, C)) < 0.7).astype(np.uint8)
    seen = set()
    for R in (16 * N + 13 * M, 8 * N, 5 * M + 200):
        ref = _check_mix_to_budget(base.psy, rows, R, [0, 30, -7], active)
        seen |= set(np.unique(ref[2]).tolist())
        _check_mix_to_budget(base.psy, rows[:1], R, None)
    assert len(seen) >= 3
    dst = base.with_row_budget(1365)
    assert dst.mix_packed_rows_launches(C, sources_n=2) == 6
    packed = [np_pack(q, s, off) for q, s in rows[:2]]
    got = dst.mix_packed_rows([_upload(d, i) for d, i in packed], [4, -4], None, True)
    _eq([g.cpu().numpy() for g in got], np_mix(packed, off, N, 1365, [4, -4])[:4], "composition")


@gpu
def test_nine_sources_run_the_composition():
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    dst = base.with_row_budget(1365)
    sources = _sources(base, 2, 2, 1, 9, 70)
    assert dst.mix_packed_rows_launches(1, sources_n=9) == 20 and dst.mix_packed_rows_launches(1, sources_n=8) == 1
    got = dst.mix_packed_rows(sources, list(range(-4, 5)), None, True)
    ref = _reference(_unpacked(sources, off), off, 1365, list(range(-4, 5)))
    _eq([g.cpu().numpy() for g in got], ref[:4], "S = 9")
    assert int(ref[3].max()) > 0


@gpu
def test_launch_table(monkeypatch):
    base = audiocodec_amd.AudioCodec(48000, N0)
    assert base.mix_packed_rows_launches(2, sources_n=2) == 0                # no budget
    lib = _lib.load()
    plan = base.with_row_budget(1365).psy._plan(torch.device("cuda", torch.cuda.current_device()))
    assert lib.ac_mix_launches(plan, 0, 2) == 0 and lib.ac_mix_launches(plan, 2, 0) == 0 and lib.ac_mix_launches(plan, 2, -1) == 0
    for C in (1, 2, 3, 7):
        for R in (320, 1365, CAP):
            for S in (1, 2, 8):
                assert base.with_row_budget(R).mix_packed_rows_launches(C, sources_n=S) == 1, (C, R, S)
            assert base.with_row_budget(R).mix_packed_rows_launches(C, sources_n=9) == 20
    assert base.with_row_budget(CAP + 32).mix_packed_rows_launches(2, sources_n=2) == 6
    for N, M in ((2048, 64), (960, 64), (1024, 32)):
        assert audiocodec_amd.AudioCodec(48000, N, bark_bands_n=M).with_row_budget(1365).mix_packed_rows_launches(2, sources_n=3) == 8
    cbr = base.with_row_budget(1365)
    monkeypatch.setenv("AC_MIX_NOFUSE", "1")
    for S in (1, 2, 8, 9):
        assert cbr.mix_packed_rows_launches(2, sources_n=S) == 2 * S + 2
    monkeypatch.delenv("AC_MIX_NOFUSE")
    assert cbr.mix_packed_rows_launches(2, sources_n=2) == 1
    monkeypatch.setenv("AC_TRANSRATE_NOFUSE", "1")                           # fused where the transrating launch is
    assert cbr.mix_packed_rows_launches(2, sources_n=2) == 6
    monkeypatch.delenv("AC_TRANSRATE_NOFUSE")


@gpu
def test_chip_filling():
    """8224 rows -- 2056 workgroups of four waves -- of seeded noise at many levels, two sources, against the composition."""
    B, K, C = 16, 256, 2
    base = audiocodec_amd.AudioCodec(48000, N0)
    g = torch.Generator(device="cuda").manual_seed(1234)
    src = base.with_row_budget(2730)
    sources = []
    for i in range(2):
        x = torch.rand((B, K * N0, C), generator=g, device="cuda") * 2 - 1
        x *= torch.logspace(-3, 0, B, device="cuda")[:, None, None] * torch.linspace(0.05, 1, K * N0, device="cuda")[None, :, None]
        x[i] = 0.0                                                          # 514 all-zero rows in each source
        sources.append(src.encode_packed_rows(x if i == 0 else x.flip(0).contiguous())[:2])
    dst = base.with_row_budget(1365)
    assert sources[0][1].numel() == 8224 and dst.mix_packed_rows_launches(C, sources_n=2) == 1
    fused = dst.mix_packed_rows(sources, [0, 2], None, True)
    comp = _composition(dst, sources, [0, 2])
    for name, a, b in zip(("data", "index", "fits", "offset"), fused, comp):
        assert torch.equal(a, b), (name, _where(a, b))
    off = comp[3]
    assert int((off > 0).sum()) >= 1000 and len(torch.unique(off)) >= 3 and bool(comp[2].all()) and int(fused[0].max()) > 0


def _mix_abi(codec, sources, out, fits, rb, gains=None, active=None, flags=None, X=None, t=None, thr=None, offset=None, B=None,
             src=True, dst=True, S=None, null_source=False, null_src=False):
    lib = _lib.load()
    dev = out.device
    n = len(sources)
    arr = (_lib.PackedRows * n)(*[_lib.PackedRows(d.data_ptr(), d.numel(), i.data_ptr()) for d, i in sources])
    if null_source:
        arr[n - 1].index = None
    gain = (ctypes.c_int32 * n)(*gains) if gains is not None else None
    mix = _lib.MixRows(n if S is None else S, None if null_src else arr, gain, active.data_ptr() if active is not None else None)
    po = _lib.PackedOut(out.data_ptr(), rb, fits.data_ptr())
    index = sources[0][1]

    def p(v):
        return ctypes.c_void_p(v.data_ptr()) if v is not None else None
    st = lib.ac_encode_fused_ex(codec.mdct._plan(dev), codec.psy._plan(dev), ctypes.addressof(mix) if src else None, p(X), p(t),
                                p(thr), 0.0, (_lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED | _lib.AC_IN_MIX) if flags is None else flags,
                                ctypes.addressof(po) if dst else None, p(offset), 0, index.shape[0] if B is None else B,
                                index.shape[1] - 1, index.shape[2], None)
    torch.cuda.synchronize()
    return st


@gpu
def test_c_abi():
    lib = _lib.load()
    base = audiocodec_amd.AudioCodec(48000, N0)
    dst = base.with_row_budget(1365)
    sources = _sources(base, 3, 5, 2, 2, 17)
    rows, rb = sources[0][1].numel(), dst.row_bytes
    out = torch.full((rows * rb,), 0xA5, dtype=torch.uint8, device="cuda")
    fits = torch.full((rows,), 7, dtype=torch.uint8, device="cuda")
    offset = torch.full((rows,), -3, dtype=torch.int16, device="cuda")
    spare = torch.zeros((3, 6, N0, 2), device="cuda")
    refused = (out.clone(), fits.clone(), offset.clone())
    IN, EMIT, MIX = _lib.AC_IN_PACKED, _lib.AC_EMIT_PACKED, _lib.AC_IN_MIX
    for flags in (MIX, MIX | IN, MIX | EMIT, MIX | IN | EMIT | _lib.AC_IN_PCM16, MIX | IN | EMIT | _lib.AC_EMIT_REDUNDANT,
                  MIX | IN | EMIT | _lib.AC_EMIT_CARRY, MIX | IN | EMIT | _lib.AC_EMIT_CODES, MIX | IN | EMIT | 128, MIX | IN | EMIT | 2048):
        assert _mix_abi(dst, sources, out, fits, rb, flags=flags, offset=offset) == _lib.AC_EINVAL, flags
        assert lib.ac_last_error()
    for kw in ({"X": spare}, {"t": spare}, {"thr": spare}, {"src": False}, {"dst": False}, {"S": 0}, {"S": -1}, {"null_src": True},
               {"null_source": True}, {"gains": [0, 255]}, {"gains": [-255, 0]}):
        assert _mix_abi(dst, sources, out, fits, rb, offset=offset, **kw) == _lib.AC_EINVAL, kw
    assert _mix_abi(dst, sources, out, fits, rb + 4, offset=offset) == _lib.AC_EINVAL
    assert b"row_bytes" in lib.ac_last_error()
    assert _mix_abi(base, sources, out, fits, rb, offset=offset) == _lib.AC_EINVAL and b"row budget" in lib.ac_last_error()
    wide = audiocodec_amd.AudioCodec(48000, 2048).with_row_budget(1365)
    assert _mix_abi(wide, sources, out, fits, rb, offset=offset) == _lib.AC_EUNSUPPORTED
    assert b"composition" in lib.ac_last_error()
    with _nofuse():
        assert _mix_abi(dst, sources, out, fits, rb, offset=offset) == _lib.AC_EUNSUPPORTED
    nine = sources * 4 + sources[:1]
    assert _mix_abi(dst, nine, out, fits, rb, offset=offset) == _lib.AC_EUNSUPPORTED
    for got, want in zip((out, fits, offset), refused):                   # the refused calls wrote nothing
        assert torch.equal(got, want)
    assert _mix_abi(dst, sources, out, fits, rb, offset=offset, B=0) == _lib.AC_OK
    assert torch.equal(out, refused[0])
    gains = [6, -9]
    active = (torch.arange(2 * rows, device="cuda") % 5 != 0).to(torch.uint8).view(2, 3, 6, 2)
    assert _mix_abi(dst, sources, out, fits, rb, gains, active, offset=offset) == _lib.AC_OK, lib.ac_last_error()
    ref = _composition(dst, sources, gains, active)
    assert torch.equal(out, ref[0]) and torch.equal(fits.view(3, 6, 2), ref[2].to(torch.uint8))
    assert torch.equal(offset.view(3, 6, 2), ref[3])
    out.fill_(0xA5)
    assert _mix_abi(dst, sources, out, fits, rb) == _lib.AC_OK            # gain, active and out1 may be NULL
    assert torch.equal(out, _composition(dst, sources)[0])


@gpu
def test_python_interface_validates_device_tensors():
    cbr = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    data = torch.zeros(64, dtype=torch.uint8, device="cuda")
    index = torch.zeros((1, 2, 2), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="shape"):
        cbr.mix_packed_rows([(data, index), (data, index[:, :1])])
    for bad in (torch.ones((1, 1, 2, 2), dtype=torch.uint8, device="cuda"), torch.ones((2, 1, 2), dtype=torch.uint8, device="cuda"),
                torch.ones((2, 1, 2, 2), dtype=torch.int32, device="cuda"), torch.ones((2, 1, 2, 2), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="active"):
            cbr.mix_packed_rows([(data, index), (data, index)], active=bad)
    with pytest.raises(TypeError, match="active"):
        cbr.mix_packed_rows([(data, index)], active=np.ones((1, 1, 2, 2), np.uint8))
    codes, sf = torch.zeros((1, 2, N0, 2), dtype=torch.int16, device="cuda"), torch.zeros((1, 2, M0, 2), dtype=torch.int8, device="cuda")
    with pytest.raises(ValueError, match="shape"):
        cbr.psy.mix_to_budget([(codes, sf), (codes[:, :1], sf[:, :1])], None, 1365)
    with pytest.raises(ValueError, match="row_bits"):
        cbr.psy.mix_to_budget([(codes, sf)], None, 10)


@pytest.fixture(scope="module")
def harness():
    from stream_order import Harness
    return Harness()


def _flat_call(dst, route):
    def fused(da, ia, db, ib, act):
        return dst.mix_packed_rows([(da, ia), (db, ib)], [2, -3], act, True)

    def comp(da, ia, db, ib, act):
        return _composition(dst, [(da, ia), (db, ib)], [2, -3], act)
    return fused if route == "fused" else comp


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
@pytest.mark.parametrize("check", ["delayed_producer", "busy_default"])
def test_stream_contract(harness, check, route):
    base = audiocodec_amd.AudioCodec(48000, N0)
    dst = base.with_row_budget(1365)
    src = base.with_row_budget(2730)
    (da, ia), (db, ib) = (src.encode_packed_rows(_pcm(N0, 2, 4, 20, seed=77 + i, inject=False))[:2] for i in range(2))
    act = (torch.arange(2 * ia.numel(), device="cuda") % 7 != 0).to(torch.uint8).view((2,) + tuple(ia.shape))
    torch.cuda.synchronize()
    assert dst.mix_packed_rows_launches(2, sources_n=2) == 1
    getattr(harness, check)("cbr.mix_packed_rows[1024-2,%s]" % route, ([da, ia, db, ib, act], _flat_call(dst, route)))


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
def test_graph_capture(route):
    """One eager call (plans, allocator, the band table), then a linear capture on one stream, replayed on new contents."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    call = _flat_call(dst, route)
    (da, ia), (db, ib) = (src.encode_packed_rows(_x(3, 5, 2, 5 + i))[:2] for i in range(2))
    act = torch.ones((2,) + tuple(ia.shape), dtype=torch.uint8, device="cuda")
    call(da, ia, db, ib, act)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(da, ia, db, ib, act)
    for seed in (6, 7):
        da.copy_(src.encode_packed_rows(_x(3, 5, 2, seed))[0])
        db.copy_(src.encode_packed_rows(_x(3, 5, 2, seed + 20, flip=True))[0])
        act.copy_((torch.arange(act.numel(), device="cuda") % (seed + 1) != 0).view(act.shape))
        g.replay()
        torch.cuda.synchronize()
        ref = call(da.clone(), ia, db.clone(), ib, act.clone())
        assert int((ref[3] > 0).sum()) >= 1 and int(ref[0].max()) > 0
        for got, want in zip(out, ref):
            assert torch.equal(got, want), (seed, _where(got, want))


@gpu
def test_an_empty_batch_gives_empty_results():
    dst = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    data = torch.zeros((64,), dtype=torch.uint8, device="cuda")
    for shape in ((0, 3, 2), (2, 0, 2)):
        index = torch.zeros(shape, dtype=torch.int64, device="cuda")
        got = dst.mix_packed_rows([(data, index), (data, index)], [1, 2], None, True)
        assert got[0].shape == (0,) and got[1].shape == shape and got[2].shape == shape and got[2].dtype == torch.bool
        assert got[3].shape == shape and got[3].dtype == torch.int16 and len(dst.mix_packed_rows([(data, index)])) == 3
    codes = torch.zeros((0, 3, N0, 2), dtype=torch.int16, device="cuda")
    sf = torch.zeros((0, 3, M0, 2), dtype=torch.int8, device="cuda")
    assert dst.psy.mix_to_budget([(codes, sf), (codes, sf)], None, 1365)[2].shape == (0, 3, 2)


@gpu
def test_chunks_of_two_streams_mix_to_the_one_shot_rows():
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    B, K, C = 3, 5, 2
    xs = [_x(B, K, C, 31), _x(B, K, C, 32, flip=True)]
    whole = dst.mix_packed_rows([src.encode_packed_rows(x)[:2] for x in xs], [1, -2], None, True)
    rb = dst.row_bytes
    rows = whole[0].view(B, K + 1, C, rb)
    sts = [src.stream(B, C), src.stream(B, C)]
    a = 0
    for k in (2, 1, 2):
        chunks = [st.encode_packed_rows_chunk(x[:, a * N0:(a + k) * N0].contiguous())[:2] for st, x in zip(sts, xs)]
        got = dst.mix_packed_rows(chunks, [1, -2], None, True)
        assert torch.equal(got[0].view(B, k, C, rb), rows[:, a:a + k]), (a, k)
        assert torch.equal(got[2], whole[2][:, a:a + k]) and torch.equal(got[3], whole[3][:, a:a + k])
        a += k
    assert int((whole[3] > 0).sum()) >= 1


@gpu
@pytest.mark.parametrize("pcm16", [False, True])
def test_end_to_end(pcm16):
    """On rows that fit at offset 0 with R = 16384, dequantize(unpack(mix)) obeys section 8a rule 6 against X^_A + X^_B with
    the step step(s0): |error| <= step / 2 -- the rounding of rint, exact up to the two roundings of the products (the
    (1 + 1e-6) and 1e-6 |X| of rule 6).  decode_packed(mix) equals decode_quantized(*unpack(mix))."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_row_budget(1365), base.with_row_budget(CAP)
    off = base.psy.scale_band_offsets
    sources = [src.encode_packed_rows(_pcm(N0, 2, 3, 5, seed=32 + i, inject=False))[:2] for i in range(2)]
    out, idx, fits, offset = dst.mix_packed_rows(sources, None, None, True)
    assert bool(fits.all()) and int(offset.max()) == 0
    codes, sf = dst.psy.unpack(out, idx)
    Xm = dst.psy.dequantize(codes, sf).cpu().numpy().astype(np.float64)
    ua, ub = (base.psy.unpack(d, i) for d, i in sources)
    Xs = (base.psy.dequantize(*ua) + base.psy.dequantize(*ub)).cpu().numpy().astype(np.float64)
    _, s0, _ = mix_spectrum(_unpacked(sources, off), off)
    assert (s0 != -128).all()
    band = np.repeat(np.arange(M0), np.diff(off))
    step = np_step(s0.astype(np.int32))[:, :, band, :].astype(np.float64)
    ok = np.abs(codes.cpu().numpy().astype(np.int32)) < 32767
    err = np.abs(Xm - Xs)
    bound = step / 2 * (1 + 1e-6) + 1e-6 * np.abs(Xs)
    print("largest error / bound: %.6f" % float((err[ok] / bound[ok]).max()))
    assert ok.all() and (err <= bound).all()
    got = dst.decode_packed(out, idx, pcm16)
    ref = dst.decode_quantized(codes, sf, pcm16)
    assert _same(got, ref), _where(got, ref)
