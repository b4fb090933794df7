"""Routing the packed rows of S sources to O mixes at a bitrate, without decoding:
``AudioCodec.route_packed_rows`` (the ``AC_IN_PACKED | AC_EMIT_PACKED | AC_IN_ROUTE`` form of ``ac_encode_fused_ex``),
``mix_minus_routes`` and the one launch at filters_n = 1024 that stages every source row once and packs every output's row from
the staged copies (k_route_p).

Every GPU comparison of the one launch is ``torch.equal`` against the composition -- one ``mix_packed_rows`` per output on the
sources it hears, which runs everywhere while ``AC_ROUTE_NOFUSE=1`` is set -- and the composition is compared byte for byte with
the numpy restatement of ``route_reference.py``, a loop over ``mix_reference``.  Before any kernel result is compared, numpy
alone must show that the input exercises the rule per output (``_conditions``).

Seeded defects (scratch builds, not committed), each run once against this file on an MI355X:
(1) ``s0`` folded over all staged sources instead of the output's heard ones;
(2) the accumulators reused across outputs without clearing.
The cases that fail under each are listed in ``MUTATIONS`` below.
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
from mix_reference import mix_spectrum, np_mix
from pack_reference import np_pack, np_row_bits, np_unpack
from pack_rows_reference import marked_row
from route_reference import heard, mix_minus, np_route, route_budget, route_rows
from test_encode_quantized_fused import _pcm, _same, _where
from test_mix import GAINS, SHAPES, _dev, _sources, _unpacked, _upload, _x
from test_quantizer import np_offsets, np_quantize
from test_rate_control import EX_OFF, EX_THR, EX_X
from test_transrate import _random_rows
from transrate_reference import np_transrate

gpu = pytest.mark.gpu
N0, M0 = 1024, 64
CAP = _lib.AC_PACK_ROWS_MAX_BITS
HEADER = os.path.join(ROOT, "include", "audiocodec_amd.h")
BUDGETS = [1365, 320, CAP]                                     # from sources held at 2730 bits
SO = [(1, 1), (2, 2), (3, 3), (8, 8), (3, 1), (1, 3), (8, 2), (4, 4), (4, 8)]   # (S = 8: the composition; 4: the launch's most)
MUTE = _lib.AC_ROUTE_MUTE

MUTATIONS = """
Both builds leave the 8 CPU tests and every case that runs the composition alone passing: (S, O) = (8, 8) and (8, 2), the
other sizes, nine sources or outputs, the launch table, the stream contract, graph capture and the chunks (a route against
itself), the argument checks and the end-to-end decode (which asks no more than that an output decodes as it unpacks).
(1) s0 folded over every staged source: 34 of the 69 GPU cases fail -- test_route_fused_composition_numpy at (S, O) = (2, 2),
    (3, 3), (4, 4) and (4, 8) on all four shapes and at (1, 3) on (3, 5, 1) (a -128 band poisons the output that hears nothing);
    test_the_longest_staged_row, test_route_kinds, test_active_patterns, test_isolation, test_heterogeneous_sources, the 10
    cases of test_band_layouts, test_chip_filling and test_c_abi.  (1, 1) and (3, 1), whose outputs hear every staged source,
    pass, as they must.
(2) accumulators kept across outputs: 37 fail -- the same 34 and (1, 3) on the other three shapes: every case whose second
    output follows a row with a non-zero code.
"""


def _eq(a, b, what=""):
    for i, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg="%s, output %d" % (what, i))


def _routes(S, O):
    """The table of a case: mix-minus where S = O, else outputs that hear different subsets at different gains."""
    if S == O:
        return mix_minus(S, {1: [0], 2: [1, -1], 3: [0, 3, -5], 4: [0, 3, -5, 2], 8: GAINS[8]}[S]) if S > 1 else [[0]]
    if O == 1:
        return [[2, -3, 5]]
    if S == 1:
        return [[0], [7], [None]]
    if S == 4:
        return mix_minus(4, [0, 3, -5, 2]) + [[-1 if i == o else None for i in range(4)] for o in range(3)] + [[1, 1, 1, 1]]
    return [list(GAINS[8]), [g if i % 2 == 0 else None for i, g in enumerate(GAINS[8])]]


# ---- CPU: the definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,N,M", [(44100, 256, 48), (48000, 128, 64)])
def test_consequences_of_the_definition(sr, N, M):
    """(a) .. (e) of section 8i on random non-canonical rows with -128 bands, at three budgets."""
    rng = np.random.default_rng(N + M + 1)
    off = np_offsets(sr, N, M)
    packed = [np_pack(*_random_rows(rng, off, 2, 3, 2), off) for _ in range(3)]
    gains = [3, -5, 40]
    act = (rng.random((3, 2, 3, 2)) < 0.8).astype(np.uint8)
    for R in (5 * M + 40, 900, 16 * N + 13 * M):
        # (a) an output that hears everything is the mix
        _eq([a[0] for a in np_route(packed, off, N, R, [gains], act)[:1]] + [np_route(packed, off, N, R, [gains], act)[3][0]],
            [np_mix(packed, off, N, R, gains, act)[0], np_mix(packed, off, N, R, gains, act)[3]], "(a) at %d" % R)
        # (b) the identity route gives the transrating call's bytes per output
        ident = np_route(packed, off, N, R, [[0 if i == o else None for i in range(3)] for o in range(3)])
        for o in range(3):
            t = np_transrate(*packed[o], off, N, R)
            _eq((ident[0][o], ident[1], ident[2][o], ident[3][o]), t[:4], "(b) at %d, output %d" % (R, o))
        # (c) mix-minus of two hands each party the other's transrated rows
        mm = np_route(packed[:2], off, N, R, mix_minus(2))
        for o in range(2):
            t = np_transrate(*packed[1 - o], off, N, R)
            _eq((mm[0][o], mm[2][o], mm[3][o]), (t[0], t[2], t[3]), "(c) at %d, output %d" % (R, o))
        # (d) permuting the outputs permutes data', fits' and offset
        table = [[3, None, 40], [None, -5, None], [None, None, None], [3, -5, 40]]
        perm = [2, 0, 3, 1]
        one, two = np_route(packed, off, N, R, table, act), np_route(packed, off, N, R, [table[p] for p in perm], act)
        for k in (0, 2, 3):
            np.testing.assert_array_equal(two[k], one[k][perm])
        assert not one[0][2].any() and one[2][2].all() and not one[3][2].any()          # the output that hears nothing
        # (e) an output does not depend on rows it does not hear
        junk = list(packed)
        junk[1] = (np.full_like(packed[1][0], 0xFF), packed[1][1])
        three = np_route(junk, off, N, R, table, act)
        for o in (0, 2):
            for k in (0, 2, 3):
                np.testing.assert_array_equal(three[k][o], one[k][o])
        assert not np.array_equal(three[0][1], one[0][1])


def test_worked_example_routed_as_mix_minus_of_two():
    """Section 8h's example (M = 4) held by both parties of a bridge: each hears the other's row transrated, section 8e's
    table; and what the negation's listener hears is not the table negated (zigzag widths are not even in the code)."""
    c0, s0 = np_quantize(EX_X, EX_THR, EX_OFF)
    assert np_row_bits(c0, s0, EX_OFF).ravel()[0] == 100
    table = {100: (0, 100, [0, -30, -22, -44], [54, -36, 45, -32, 2, 20, 0, -41]),
             96: (3, 94, [0, -27, -19, -41], [32, -21, 27, -19, 1, 12, 0, -24]),
             64: (20, 62, [0, -10, -2, -24], [2, -1, 1, -1, 0, 1, 0, -1]),
             56: (26, 32, [0, -4, 4, -18], [1, 0, 0, 0, 0, 0, 0, 0]),
             20: (28, 20, [0, -2, 6, -16], [0, 0, 0, 0, 0, 0, 0, 0])}
    for R, (k, bits, sf, codes) in table.items():
        for out in route_budget([(c0, s0), (c0, s0)], EX_OFF, R, mix_minus(2)):
            assert (int(out[2].ravel()[0]), int(out[3].ravel()[0])) == (k, bits), R
            assert out[1].ravel().tolist() == sf and out[0].ravel().tolist() == codes, R
    hears_neg, hears_pos = route_budget([(c0, s0), (-c0, s0)], EX_OFF, 96, mix_minus(2))
    assert int(hears_pos[2].ravel()[0]) == 3 and hears_pos[0].ravel().tolist() == table[96][3]
    assert int(hears_neg[2].ravel()[0]) == 2 and hears_neg[0].ravel().tolist() == [-38, 25, -32, 23, -1, -14, 0, 29]
    # a gain of +4 (one doubling) on source 0 moves its listener's scale factors up by 4: the same codes at the same offset
    up = route_budget([(c0, s0), (c0, s0)], EX_OFF, 96, mix_minus(2, [4, 0]))
    assert int(up[1][2].ravel()[0]) == 3 and up[1][0].ravel().tolist() == table[96][3] and up[1][1].ravel().tolist() == [0, -23, -15, -37]
    assert int(up[0][2].ravel()[0]) == 3 and up[0][1].ravel().tolist() == table[96][2]


# ---- CPU: header, library, Python validation ------------------------------------------------------------------------------
def test_header_declares_the_flag_the_struct_and_the_launch_query():
    text = open(HEADER).read()
    assert re.search(r"\bAC_IN_ROUTE\s*=\s*2048\b", text)
    assert re.search(r"#define\s+AC_ROUTE_MAX_SOURCES\s+4\b", text) and re.search(r"#define\s+AC_ROUTE_MAX_OUTPUTS\s+8\b", text)
    assert re.search(r"#define\s+AC_ROUTE_MUTE\s+\(-32768\)", text)
    m = re.search(r"typedef\s+struct\s+ac_route_rows\s*\{(.*?)\}\s*ac_route_rows\s*;", text, flags=re.S)
    assert m, "ac_route_rows is not declared"
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["int32_t sources_n", "int32_t outputs_n", "const struct ac_packed_rows* src", "const int32_t* gain",
                      "const uint8_t* active"], fields
    m = re.search(r"AC_API\s+int\s+ac_route_launches\s*\(([^;]*)\)\s*;", text)
    assert m and "stream" not in m.group(1) and m.group(1).count(",") == 3, m and m.group(1)
    assert re.search(r"#define\s+AC_VERSION\s+171\b", text)


def test_library_exports_the_launch_query():
    lib = _lib.load()
    assert "ac_route_launches" in _lib.PROTOTYPES and callable(lib.ac_route_launches)
    assert lib.ac_route_launches(None, 2, 2, 2) == 0
    assert lib.ac_version() == 171
    assert _lib.AC_IN_ROUTE == 2048 and _lib.AC_ROUTE_MAX_SOURCES == 4 and _lib.AC_ROUTE_MAX_OUTPUTS == 8 and MUTE == -32768


def test_ctypes_mirror_has_the_headers_layout():
    Q = _lib.RouteRows
    assert [f[0] for f in Q._fields_] == ["sources_n", "outputs_n", "src", "gain", "active"]
    assert (Q.sources_n.offset, Q.outputs_n.offset, Q.src.offset, Q.gain.offset, Q.active.offset) == (0, 4, 8, 16, 24)
    assert ctypes.sizeof(Q) == 32 and ctypes.sizeof(_lib.PackedRows) == 24


def test_mix_minus_routes():
    mk = audiocodec_amd.AudioCodec.mix_minus_routes
    assert mk(1) == [[None]]
    assert mk(2) == [[None, 0], [0, None]]
    assert mk(3, [1, -2, 254]) == [[None, -2, 254], [1, None, 254], [1, -2, None]]
    assert mk(3, [1, -2, 254]) == mix_minus(3, [1, -2, 254])
    for bad in (0, -1):
        with pytest.raises(ValueError):
            mk(bad)
    for bad in (2.0, True, "2"):
        with pytest.raises(TypeError):
            mk(bad)
    with pytest.raises(ValueError, match="gain"):
        mk(2, [0, 255])
    with pytest.raises(ValueError, match="gains"):
        mk(2, [0])
    with pytest.raises(TypeError, match="gain"):
        mk(2, [0, 1.0])


def test_python_interface_validates_its_arguments():
    base = audiocodec_amd.AudioCodec(48000, N0)
    data, index = torch.zeros(64, dtype=torch.uint8), torch.zeros((1, 1, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"with_bitrate\(\)"):
        base.route_packed_rows([(data, index)], [[0]])
    cbr = base.with_bitrate(64000)
    with pytest.raises(ValueError, match="at least one source"):
        cbr.route_packed_rows([], [[0]])
    with pytest.raises(ValueError, match="at least one output"):
        cbr.route_packed_rows([(data, index)], [])
    for bad in ([[0, 0]], [[]], [[0], [0, None]]):                         # ragged: not S entries
        with pytest.raises(ValueError, match="entries"):
            cbr.route_packed_rows([(data, index)], bad)
    for bad in ([[1.0]], [[True]], [["3"]], [[0], [False]]):
        with pytest.raises(TypeError, match="gain"):
            cbr.route_packed_rows([(data, index)], bad)
    for bad in ([[255]], [[-255]], [[0], [MUTE]]):
        with pytest.raises(ValueError, match="gain"):
            cbr.route_packed_rows([(data, index)], bad)
    with pytest.raises(TypeError):
        cbr.route_packed_rows([(data, index)], [0])                         # a route is a sequence
    for bad in ((data.to(torch.int8), index), (data, index.to(torch.int32)), (data.view(8, 8), index), (data, index[0]),
                (data, index)):                               # the last: host tensors
        with pytest.raises(ValueError):
            cbr.route_packed_rows([bad], [[0]])
    with pytest.raises(TypeError):
        cbr.route_packed_rows([(data.numpy(), index)], [[0]])
    with pytest.raises(NotImplementedError, match="float32"):
        audiocodec_amd.AudioCodec(48000, N0, compute_dtype=torch.float64).route_packed_rows([(data, index)], [[0]])
    with pytest.raises(TypeError):
        cbr.route_packed_rows_launches(2, sources_n=2)                      # both counts are required, by keyword
    with pytest.raises(TypeError):
        cbr.route_packed_rows_launches(2, None, 2, 2)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
class _nofuse:
    """AC_ROUTE_NOFUSE=1 (read per call) around a block."""

    def __enter__(self):
        os.environ["AC_ROUTE_NOFUSE"] = "1"

    def __exit__(self, *exc):
        del os.environ["AC_ROUTE_NOFUSE"]
        return False


def _composition(codec, sources, routes, active=None, return_offset=True):
    C = sources[0][1].shape[2]
    with _nofuse():
        assert codec.route_packed_rows_launches(C, sources_n=len(sources), outputs_n=len(routes)) == \
            len(routes) * codec.mix_packed_rows_launches(C, sources_n=len(sources))
        return codec.route_packed_rows(sources, routes, active, return_offset)


def _three_ways(dst, sources, rows, off, routes, active=None, what="", ref=None):
    """numpy, the composition and the one launch on the same sources: returns the reference."""
    if ref is None:
        ref = route_rows(rows, off, dst.row_bits, routes, None if active is None else active.cpu().numpy())
    comp = _composition(dst, sources, routes, active)
    C, S, O = sources[0][1].shape[2], len(sources), len(routes)
    one = S <= _lib.AC_ROUTE_MAX_SOURCES and O <= _lib.AC_ROUTE_MAX_OUTPUTS   # else the default is the composition too
    assert dst.route_packed_rows_launches(C, sources_n=S, outputs_n=O) == (1 if one else O * dst.mix_packed_rows_launches(C, sources_n=S))
    fused = dst.route_packed_rows(sources, routes, active, True)
    assert fused[0].shape == (O, sources[0][1].numel() * dst.row_bytes) and fused[2].shape == (O,) + tuple(sources[0][1].shape)
    assert fused[2].dtype == torch.bool and fused[3].dtype == torch.int16 and fused[3].shape == fused[2].shape
    for name, g, c, r in zip(("data", "index", "fits", "offset"), fused, comp, ref):
        np.testing.assert_array_equal(c.cpu().numpy(), r, err_msg="%s %s" % (name, what))
        assert torch.equal(g, c), (name, what, _where(g, c))
    return ref


def _conditions(rows, off, routes, refs):
    """What numpy alone must show before a kernel is asked: in one call at least 3 distinct offsets across its outputs; a
    row that fits only above offset 0; a band of a row whose s0 differs between two outputs."""
    assert any(len(np.unique(r[3])) >= 3 for r in refs), [np.unique(r[3]).tolist() for r in refs]
    assert any(int(((r[3] > 0) & r[2]).sum()) >= 1 for r in refs), "no row that fits only at k > 0"
    s0 = [mix_spectrum([rows[i] for i in heard(rt)], off, [rt[i] for i in heard(rt)])[1] for rt in routes if heard(rt)]
    assert any(int((s0[a] != s0[b]).sum()) >= 1 for a in range(len(s0)) for b in range(a)), "s0 is the same for every output"


@gpu
@pytest.mark.parametrize("S,O", SO)
@pytest.mark.parametrize("B,K,C", SHAPES)
def test_route_fused_composition_numpy(B, K, C, S, O):
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    sources = _sources(base, B, K, C, S, C + 2 * B + K + 1)
    rows = _unpacked(sources, off)
    routes = _routes(S, O)
    assert base.mix_minus_routes(S, routes[1][0:1] + routes[0][1:]) == routes if S == O and S > 1 else True
    refs = {R: route_rows(rows, off, R, routes) for R in BUDGETS}
    for R in BUDGETS:
        print("S = %d, O = %d to %d: %d rows, offsets %s, %d unfit" % (S, O, R, refs[R][3][0].size, np.unique(refs[R][3]).tolist(),
                                                                       int((~refs[R][2]).sum())))
    if S >= 2 and O >= 2 and B * (K + 1) * C >= 16:
        _conditions(rows, off, routes, [refs[R] for R in BUDGETS])
    for R in BUDGETS:
        dst = base.with_row_budget(R)
        _three_ways(dst, sources, rows, off, routes, None, "S = %d, O = %d at %d" % (S, O, R), refs[R])
        assert len(dst.route_packed_rows(sources, routes)) == 3


@gpu
def test_the_longest_staged_row():
    """A dense source whose 64 bands are all 16 bits wide -- 17 216 bits, every word of a staged slice and the loop behind the
    batched loads -- beside rows at 2730 bits, into three outputs."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    B, K, C = 2, 3, 2
    rng = np.random.default_rng(5)
    codes = rng.integers(-32768, 32768, (B, K + 1, N0, C)).astype(np.int16)
    codes[:, :, off[:-1], :] = -32768                                        # every band holds a 16-bit code
    sf = rng.integers(-60, -20, (B, K + 1, M0, C)).astype(np.int8)
    data, index = np_pack(codes, sf, off)
    assert (np_row_bits(codes, sf, off) == 16 * N0 + 13 * M0).all()
    sources = [_upload(data, index)] + _sources(base, B, K, C, 2, 3)
    rows = _unpacked(sources, off)
    routes = [[0, None, 2], [None, 1, -1], [-6, 0, None]]
    for R in (1365, CAP):
        ref = _three_ways(base.with_row_budget(R), sources, rows, off, routes, None, "to %d" % R)
        assert int(ref[3].max()) > 0


@gpu
def test_route_kinds():
    """Mix-minus, the identity, an output that hears all, one that hears nothing, one source at +254, -254 and a clamping
    gain in different outputs, duplicate outputs and a permutation of the outputs: consequences (a) .. (d) on the device."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    B, K, C, S = 2, 3, 2, 3
    sources = _sources(base, B, K, C, S, 29)
    rows = _unpacked(sources, off)
    dst = base.with_row_budget(1365)
    g0 = mix_spectrum(rows, off)[2]
    hi = int(g0[0].max())
    gains = [2, -3, 5]
    table = base.mix_minus_routes(S, gains) + [[0 if i == o else None for i in range(S)] for o in range(S)] + \
        [gains, [None] * S, [254, None, 0], [-254, 0, None], [128 - hi, None, 1], gains, [None] * S]
    first, second = table[:8], table[5:]
    for part in (first, second):
        ref = _three_ways(dst, sources, rows, off, part, None, "kinds")
        assert len(np.unique(ref[3])) >= 3
    fused = dst.route_packed_rows(sources, first, None, True)
    for o in range(S):                                                      # (b) the identity: the transrating call
        t = dst.transrate_packed_rows(*sources[o], True)
        assert torch.equal(fused[0][3 + o], t[0]) and torch.equal(fused[2][3 + o], t[2]) and torch.equal(fused[3][3 + o], t[3])
    m = dst.mix_packed_rows(sources, gains, None, True)                     # (a) hears all: the mix
    assert torch.equal(fused[0][6], m[0]) and torch.equal(fused[1], m[1]) and torch.equal(fused[2][6], m[2]) and torch.equal(fused[3][6], m[3])
    assert not bool(fused[0][7].any()) and bool(fused[2][7].all()) and not bool(fused[3][7].any())   # hears nothing
    two = dst.route_packed_rows(sources[:2], base.mix_minus_routes(2), None, True)                  # (c)
    for o in range(2):
        t = dst.transrate_packed_rows(*sources[1 - o], True)
        assert torch.equal(two[0][o], t[0]) and torch.equal(two[3][o], t[3])
    perm = [4, 0, 7, 2, 6, 1, 5, 3]                                         # (d)
    got = dst.route_packed_rows(sources, [first[p] for p in perm], None, True)
    for k in (0, 2, 3):
        assert torch.equal(got[k], fused[k][perm])
    dup = dst.route_packed_rows(sources, second, None, True)                # duplicates: outputs 1 and 6 of `second`, 2 and 7
    assert second[1] == second[6] and second[2] == second[7]
    assert torch.equal(dup[0][1], dup[0][6]) and torch.equal(dup[0][2], dup[0][7]) and torch.equal(dup[3][1], dup[3][6])
    assert not torch.equal(dup[0][3], dup[0][4]) and not torch.equal(dup[0][3], dup[0][5])    # +254, -254, the clamp


@gpu
def test_active_patterns():
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    B, K, C, S = 2, 3, 2, 3
    F = K + 1
    sources = _sources(base, B, K, C, S, 23)
    rows = _unpacked(sources, off)
    routes = [[None, -3, 5], [2, None, 5], [2, -3, None], [None, None, 5]]   # source 0 is heard by ... two; see below
    dst = base.with_row_budget(1365)
    none = torch.zeros((S, B, F, C), dtype=torch.uint8, device="cuda")
    ref = _three_ways(dst, sources, rows, off, routes, none, "all off")
    assert not ref[0].any() and ref[2].all() and not ref[3].any()
    b, f, c = np.meshgrid(np.arange(B), np.arange(F), np.arange(C), indexing="ij")
    board = _dev(np.stack([((b + f + c + i) % 2).astype(np.uint8) for i in range(S)]))
    ref = _three_ways(dst, sources, rows, off, routes, board, "checkerboard")
    assert int(ref[3].max()) > 0
    got = dst.route_packed_rows(sources, routes, board.bool(), True)        # as bool, and with values other than 1
    assert torch.equal(got[0], _dev(ref[0])) and torch.equal(dst.route_packed_rows(sources, routes, board * 200)[0], got[0])
    # a source that a single output hears, active only in every third row: elsewhere that output is the mix without it
    only = [[7, 1, None], [None, 1, 4], [None, None, 4]]
    act = torch.ones((S, B, F, C), dtype=torch.uint8, device="cuda")
    act[0] = (torch.arange(B * F * C, device="cuda") % 3 == 0).view(B, F, C)
    ref = _three_ways(dst, sources, rows, off, only, act, "one listener")
    # ... and where it is inactive, or unheard, it is never read: its data may be anything, its index out of range
    junk = (torch.full_like(sources[0][0], 0xFF), torch.full_like(sources[0][1], 1 << 45))
    off0 = act.clone()
    off0[0] = 0
    a = dst.route_packed_rows([junk] + sources[1:], only, off0, True)
    bb = dst.route_packed_rows([junk] + sources[1:], [[None, 1, None], [None, 1, 4], [None, None, 4]], None, True)
    for x, y in zip(a, bb):
        assert torch.equal(x, y)


@gpu
def test_isolation():
    """A hostile source -- -128 bands, marked rows, random and truncated data, row starts that are negative, past the end or
    off the 4-byte phase -- spoils exactly the outputs that hear it: the others equal the call without that source."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    B, K, C = 3, 5, 2
    good = _sources(base, B, K, C, 2, 61)
    rows_good = _unpacked(good, off)
    assert sum(int((r[1] == -128).sum()) for r in rows_good) >= 1              # the NaN / Inf frames arrived as -128 bands
    dst = base.with_row_budget(1365)
    routes = [[0, 1, None], [None, 1, -2], [3, None, None], [0, 1, -2]]       # source 2 is the hostile one: outputs 1 and 3 hear it
    without = dst.route_packed_rows(good, [r[:2] for r in routes], None, True)
    data, index = (t.cpu().numpy() for t in base.with_row_budget(2730).encode_packed_rows(_x(B, K, C, 64))[:2])
    rng = np.random.default_rng(8)
    odd = index.copy()
    odd[0, 0, 0], odd[0, 1, 1], odd[0, 2, 0], odd[0, 3, 1], odd[0, 4, 0] = -7, len(data) + 1000, index[0, 2, 0] + 1, -(1 << 50), len(data) - 3
    odd[0, 5, 0], odd[1, 0, 0], odd[1, 0, 1] = (1 << 40), index[1, 0, 0] + 2, index[1, 0, 1] + 3
    small = base.with_row_budget(320).encode_packed_rows(_x(B, K, C, 62))
    assert int((~small[2]).sum()) >= 1
    all_bad = np_pack(np.zeros((B, K + 1, N0, C), np.int16), np.full((B, K + 1, M0, C), -128, np.int8), off)
    cases = [("random bytes", rng.integers(0, 256, data.shape).astype(np.uint8), index),
             ("truncated", data[:int(index[2, 3, 0]) + 13], index), ("odd row starts", data, odd),
             ("marked rows", small[0].cpu().numpy(), small[1].cpu().numpy()), ("-128 bands", all_bad[0], all_bad[1])]
    for what, d, i in cases:
        hostile = np_unpack(d, i, off, N0)
        ref = _three_ways(dst, good + [_upload(d, i)], rows_good + [hostile], off, routes, None, what)
        for o in (0, 2):                                                    # unheard there: the call without it
            for k in (0, 2, 3):
                np.testing.assert_array_equal(ref[k][o], without[k][o].cpu().numpy(), err_msg="%s, output %d" % (what, o))
        for o in (1, 3):                                                    # (the 320-bit rows hold no code, and are marked
            # where the good sources hold -128 bands already: the same input frames)
            assert what == "marked rows" or not np.array_equal(ref[0][o], without[0][o].cpu().numpy()), (what, o)
    rb = dst.row_bytes                                                      # every band bad: the marked-looking row, fits 1
    np.testing.assert_array_equal(ref[0][1][:rb], marked_row(M0, 1365))
    assert ref[2][1].all()


@gpu
def test_heterogeneous_sources():
    """A dense encode_packed result, 2730-bit fixed-stride rows, protected slots and a permuted index, routed together."""
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
    routes = base.mix_minus_routes(4, [0, -2, 4, 1])
    refs = [_three_ways(base.with_row_budget(R), sources, rows, off, routes, None, "to %d" % R) for R in (1365, 682)]
    assert len(np.unique(np.concatenate([r[3].ravel() for r in refs]))) >= 3 and int(refs[0][3].max()) > 0


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
    sources = [src.encode_packed_rows(x)[:2], src.encode_packed_rows((0.5 * x.flip(1)).contiguous())[:2],
               src.encode_packed_rows((0.25 * x.roll(N0, 1)).contiguous())[:2]]
    rows = _unpacked(sources, off)
    for R in (1365, 400):
        ref = _three_ways(base.with_row_budget(R), sources, rows, off, base.mix_minus_routes(3, [0, 3, -2]), None, "to %d" % R)
        assert int((ref[3] > 0).sum()) >= 1 and len(np.unique(ref[3])) >= 2


@gpu
@pytest.mark.parametrize("sr,N,M,C", [(48000, 2048, 64, 2), (48000, 960, 64, 1), (44100, 1024, 48, 2)])
def test_the_composition_serves_other_sizes(sr, N, M, C):
    base = audiocodec_amd.AudioCodec(sr, N, bark_bands_n=M)
    off = base.psy.scale_band_offsets
    rng = np.random.default_rng(N + M + C)
    packed = [np_pack(*_random_rows(rng, off, 2, 3, C), off) for _ in range(3)]
    routes = [[None, 4, -4], [1, None, None], [None, None, None]]
    dst = base.with_row_budget(1365)
    assert dst.route_packed_rows_launches(C, sources_n=3, outputs_n=3) == 3 * dst.mix_packed_rows_launches(C, sources_n=3) == 24
    got = dst.route_packed_rows([_upload(d, i) for d, i in packed], routes, None, True)
    _eq([g.cpu().numpy() for g in got], np_route(packed, off, N, 1365, routes)[:4], "composition")


@gpu
@pytest.mark.parametrize("S,O", [(9, 2), (2, 9)])
def test_nine_sources_or_outputs_run_the_composition(S, O):
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    dst = base.with_row_budget(1365)
    sources = _sources(base, 2, 2, 1, S, 70)
    routes = [[None if (i + o) % 3 == 0 else (i - o) for i in range(S)] for o in range(O)]
    assert dst.route_packed_rows_launches(1, sources_n=S, outputs_n=O) == O * dst.mix_packed_rows_launches(1, sources_n=S)
    assert dst.route_packed_rows_launches(1, sources_n=min(S, 4), outputs_n=min(O, 8)) == 1
    got = dst.route_packed_rows(sources, routes, None, True)
    ref = route_rows(_unpacked(sources, off), off, 1365, routes)
    _eq([g.cpu().numpy() for g in got], ref[:4], "S = %d, O = %d" % (S, O))
    assert int(ref[3].max()) > 0


@gpu
def test_launch_table(monkeypatch):
    base = audiocodec_amd.AudioCodec(48000, N0)
    assert base.route_packed_rows_launches(2, sources_n=2, outputs_n=2) == 0   # no budget
    lib = _lib.load()
    plan = base.with_row_budget(1365).psy._plan(torch.device("cuda", torch.cuda.current_device()))
    for bad in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (2, -1, 2), (2, 2, -1)):
        assert lib.ac_route_launches(plan, *bad) == 0
    for C in (1, 2, 3, 7):
        for R in (320, 1365, CAP):
            cbr = base.with_row_budget(R)
            for S, O in ((1, 1), (2, 2), (4, 4), (4, 8), (1, 8)):
                assert cbr.route_packed_rows_launches(C, sources_n=S, outputs_n=O) == 1, (C, R, S, O)
            assert cbr.route_packed_rows_launches(C, sources_n=9, outputs_n=2) == 40   # 2 (2 * 9 + 2)
            assert cbr.route_packed_rows_launches(C, sources_n=5, outputs_n=5) == 5    # five fused mixes: section 8i, measured
            assert cbr.route_packed_rows_launches(C, sources_n=8, outputs_n=8) == 8
            assert cbr.route_packed_rows_launches(C, sources_n=2, outputs_n=9) == 9    # nine fused mixes
    assert base.with_row_budget(CAP + 32).route_packed_rows_launches(2, sources_n=2, outputs_n=3) == 18
    for N, M in ((2048, 64), (960, 64), (1024, 32)):
        assert audiocodec_amd.AudioCodec(48000, N, bark_bands_n=M).with_row_budget(1365).route_packed_rows_launches(2, sources_n=3, outputs_n=2) == 16
    cbr = base.with_row_budget(1365)
    monkeypatch.setenv("AC_ROUTE_NOFUSE", "1")
    for S, O in ((1, 1), (2, 2), (4, 8), (8, 8), (9, 3), (3, 9)):
        assert cbr.route_packed_rows_launches(2, sources_n=S, outputs_n=O) == O * cbr.mix_packed_rows_launches(2, sources_n=S)
    monkeypatch.setenv("AC_MIX_NOFUSE", "1")
    assert cbr.route_packed_rows_launches(2, sources_n=3, outputs_n=3) == 24
    monkeypatch.delenv("AC_ROUTE_NOFUSE")
    assert cbr.route_packed_rows_launches(2, sources_n=3, outputs_n=3) == 24   # fused where the mixing launch is
    monkeypatch.delenv("AC_MIX_NOFUSE")
    assert cbr.route_packed_rows_launches(2, sources_n=3, outputs_n=3) == 1


@gpu
def test_chip_filling():
    """4112 row positions -- 2056 workgroups of two waves -- of seeded noise at many levels, mix-minus of three, against the
    composition."""
    B, K, C, S = 8, 256, 2, 3
    base = audiocodec_amd.AudioCodec(48000, N0)
    g = torch.Generator(device="cuda").manual_seed(1234)
    src = base.with_row_budget(2730)
    sources = []
    for i in range(S):
        x = torch.rand((B, K * N0, C), generator=g, device="cuda") * 2 - 1
        x *= torch.logspace(-3, 0, B, device="cuda")[:, None, None] * torch.linspace(0.05, 1, K * N0, device="cuda")[None, :, None]
        x[i] = 0.0                                                          # 514 all-zero rows in each source
        sources.append(src.encode_packed_rows(x if i != 1 else x.flip(0).contiguous())[:2])
    dst = base.with_row_budget(1365)
    routes = base.mix_minus_routes(S, [0, 2, -1])
    assert sources[0][1].numel() == 4112 and dst.route_packed_rows_launches(C, sources_n=S, outputs_n=S) == 1
    fused = dst.route_packed_rows(sources, routes, None, True)
    comp = _composition(dst, sources, routes)
    for name, a, b in zip(("data", "index", "fits", "offset"), fused, comp):
        assert torch.equal(a, b), (name, _where(a, b))
    off = comp[3]
    assert int((off > 0).sum()) >= 1000 and len(torch.unique(off)) >= 3 and bool(comp[2].all()) and int(fused[0].max()) > 0
    assert not torch.equal(fused[0][0], fused[0][1]) and not torch.equal(fused[0][1], fused[0][2])


def _route_abi(codec, sources, routes, out, fits, rb, active=None, flags=None, X=None, t=None, thr=None, offset=None, B=None,
               src=True, dst=True, S=None, O=None, null_source=False, null_src=False, null_gain=False, raw=None):
    lib = _lib.load()
    dev = out.device
    n, m = len(sources), len(routes)
    arr = (_lib.PackedRows * n)(*[_lib.PackedRows(d.data_ptr(), d.numel(), i.data_ptr()) for d, i in sources])
    if null_source:
        arr[n - 1].index = None
    flat = [MUTE if g is None else g for r in routes for g in r] if raw is None else raw
    gain = (ctypes.c_int32 * len(flat))(*flat)
    route = _lib.RouteRows(n if S is None else S, m if O is None else O, None if null_src else arr, None if null_gain else gain,
                           active.data_ptr() if active is not None else None)
    po = _lib.PackedOut(out.data_ptr(), rb, fits.data_ptr())
    index = sources[0][1]

    def p(v):
        return ctypes.c_void_p(v.data_ptr()) if v is not None else None
    st = lib.ac_encode_fused_ex(codec.mdct._plan(dev), codec.psy._plan(dev), ctypes.addressof(route) if src else None, p(X), p(t),
                                p(thr), 0.0, (_lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED | _lib.AC_IN_ROUTE) if flags is None else flags,
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
    routes = [[6, None], [None, -9], [6, -9]]
    O = len(routes)
    rows, rb = sources[0][1].numel(), dst.row_bytes
    out = torch.full((O * rows * rb,), 0xA5, dtype=torch.uint8, device="cuda")
    fits = torch.full((O * rows,), 7, dtype=torch.uint8, device="cuda")
    offset = torch.full((O * rows,), -3, dtype=torch.int16, device="cuda")
    spare = torch.zeros((3, 6, N0, 2), device="cuda")
    refused = (out.clone(), fits.clone(), offset.clone())
    IN, EMIT, ROUTE = _lib.AC_IN_PACKED, _lib.AC_EMIT_PACKED, _lib.AC_IN_ROUTE
    for flags in (ROUTE, ROUTE | IN, ROUTE | EMIT, ROUTE | IN | EMIT | _lib.AC_IN_PCM16, ROUTE | IN | EMIT | _lib.AC_EMIT_REDUNDANT,
                  ROUTE | IN | EMIT | _lib.AC_EMIT_CARRY, ROUTE | IN | EMIT | _lib.AC_EMIT_CODES, ROUTE | IN | EMIT | _lib.AC_IN_MIX,
                  ROUTE | IN | EMIT | 128, ROUTE | IN | EMIT | 4096):
        assert _route_abi(dst, sources, routes, out, fits, rb, flags=flags, offset=offset) == _lib.AC_EINVAL, flags
        assert lib.ac_last_error()
    for kw in ({"X": spare}, {"t": spare}, {"thr": spare}, {"src": False}, {"dst": False}, {"S": 0}, {"S": -1}, {"O": 0}, {"O": -1},
               {"null_src": True}, {"null_source": True}, {"null_gain": True}, {"raw": [6, MUTE, MUTE, -9, 255, -9]},
               {"raw": [6, MUTE, MUTE, -9, 6, -255]}, {"raw": [6, MUTE, MUTE, -9, 6, MUTE + 1]}):
        assert _route_abi(dst, sources, routes, out, fits, rb, offset=offset, **kw) == _lib.AC_EINVAL, kw
    assert _route_abi(dst, sources, routes, out, fits, rb + 4, offset=offset) == _lib.AC_EINVAL
    assert b"row_bytes" in lib.ac_last_error()
    assert _route_abi(base, sources, routes, out, fits, rb, offset=offset) == _lib.AC_EINVAL and b"row budget" in lib.ac_last_error()
    wide = audiocodec_amd.AudioCodec(48000, 2048).with_row_budget(1365)
    assert _route_abi(wide, sources, routes, out, fits, rb, offset=offset) == _lib.AC_EUNSUPPORTED
    assert b"composition" in lib.ac_last_error()
    with _nofuse():
        assert _route_abi(dst, sources, routes, out, fits, rb, offset=offset) == _lib.AC_EUNSUPPORTED
    five = sources * 2 + sources[:1]
    assert _route_abi(dst, five, [[0] * 5], out, fits, rb, offset=offset) == _lib.AC_EUNSUPPORTED
    assert _route_abi(dst, sources[:1], [[0]] * 9, out, fits, rb, offset=offset) == _lib.AC_EUNSUPPORTED
    for got, want in zip((out, fits, offset), refused):                   # the refused calls wrote nothing
        assert torch.equal(got, want)
    assert _route_abi(dst, sources, routes, out, fits, rb, offset=offset, B=0) == _lib.AC_OK
    assert torch.equal(out, refused[0])
    active = (torch.arange(2 * rows, device="cuda") % 5 != 0).to(torch.uint8).view(2, 3, 6, 2)
    assert _route_abi(dst, sources, routes, out, fits, rb, active, offset=offset) == _lib.AC_OK, lib.ac_last_error()
    ref = _composition(dst, sources, routes, active)
    assert torch.equal(out.view(O, -1), ref[0]) and torch.equal(fits.view(O, 3, 6, 2), ref[2].to(torch.uint8))
    assert torch.equal(offset.view(O, 3, 6, 2), ref[3])
    out.fill_(0xA5)
    assert _route_abi(dst, sources, routes, out, fits, rb) == _lib.AC_OK   # active and out1 may be NULL
    assert torch.equal(out.view(O, -1), _composition(dst, sources, routes)[0])


@gpu
def test_python_interface_validates_device_tensors():
    cbr = audiocodec_amd.AudioCodec(48000, N0).with_row_budget(1365)
    data = torch.zeros(64, dtype=torch.uint8, device="cuda")
    index = torch.zeros((1, 2, 2), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="shape"):
        cbr.route_packed_rows([(data, index), (data, index[:, :1])], [[0, 0]])
    for bad in (torch.ones((1, 1, 2, 2), dtype=torch.uint8, device="cuda"), torch.ones((2, 1, 2), dtype=torch.uint8, device="cuda"),
                torch.ones((2, 1, 2, 2), dtype=torch.int32, device="cuda"), torch.ones((2, 1, 2, 2), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="active"):
            cbr.route_packed_rows([(data, index), (data, index)], [[0, None]], active=bad)
    for shape in ((0, 3, 2), (2, 0, 2)):                                    # an empty batch gives empty results
        empty = torch.zeros(shape, dtype=torch.int64, device="cuda")
        got = cbr.route_packed_rows([(data, empty), (data, empty)], [[1, 2], [None, 0], [None, None]], None, True)
        assert got[0].shape == (3, 0) and got[1].shape == shape and got[2].shape == (3,) + shape and got[2].dtype == torch.bool
        assert got[3].shape == (3,) + shape and got[3].dtype == torch.int16


@pytest.fixture(scope="module")
def harness():
    from stream_order import Harness
    return Harness()


ROUTES3 = [[None, -3, 1], [2, None, 1], [2, -3, None]]


def _flat_call(dst, route):
    def fused(da, ia, db, ib, dc, ic, act):
        return dst.route_packed_rows([(da, ia), (db, ib), (dc, ic)], ROUTES3, act, True)

    def comp(da, ia, db, ib, dc, ic, act):
        return _composition(dst, [(da, ia), (db, ib), (dc, ic)], ROUTES3, act)
    return fused if route == "fused" else comp


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
@pytest.mark.parametrize("check", ["delayed_producer", "busy_default"])
def test_stream_contract(harness, check, route):
    base = audiocodec_amd.AudioCodec(48000, N0)
    dst = base.with_row_budget(1365)
    src = base.with_row_budget(2730)
    pairs = [src.encode_packed_rows(_pcm(N0, 2, 4, 20, seed=77 + i, inject=False))[:2] for i in range(3)]
    ia = pairs[0][1]
    act = (torch.arange(3 * ia.numel(), device="cuda") % 7 != 0).to(torch.uint8).view((3,) + tuple(ia.shape))
    torch.cuda.synchronize()
    assert dst.route_packed_rows_launches(2, sources_n=3, outputs_n=3) == 1
    getattr(harness, check)("cbr.route_packed_rows[1024-2,%s]" % route, ([t for p in pairs for t in p] + [act], _flat_call(dst, route)))


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
def test_graph_capture(route):
    """One eager call (plans, allocator, the band table), then a linear capture on one stream, replayed on new contents."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    call = _flat_call(dst, route)
    pairs = [src.encode_packed_rows(_x(3, 5, 2, 5 + i))[:2] for i in range(3)]
    args = [t for p in pairs for t in p]
    act = torch.ones((3,) + tuple(pairs[0][1].shape), dtype=torch.uint8, device="cuda")
    call(*args, act)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(*args, act)
    for seed in (6, 7):
        for i in range(3):
            pairs[i][0].copy_(src.encode_packed_rows(_x(3, 5, 2, seed + 20 * i, flip=bool(i & 1)))[0])
        act.copy_((torch.arange(act.numel(), device="cuda") % (seed + 1) != 0).view(act.shape))
        g.replay()
        torch.cuda.synchronize()
        ref = call(*[t.clone() for t in args], act.clone())
        assert int((ref[3] > 0).sum()) >= 1 and int(ref[0].max()) > 0
        for got, want in zip(out, ref):
            assert torch.equal(got, want), (seed, _where(got, want))


@gpu
def test_chunks_of_three_streams_route_to_the_one_shot_rows():
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    B, K, C = 3, 5, 2
    xs = [_x(B, K, C, 31), _x(B, K, C, 32, flip=True), _x(B, K, C, 33)]
    whole = dst.route_packed_rows([src.encode_packed_rows(x)[:2] for x in xs], ROUTES3, None, True)
    rb = dst.row_bytes
    rows = whole[0].view(3, B, K + 1, C, rb)
    sts = [src.stream(B, C) for _ in xs]
    a = 0
    for k in (2, 1, 2):
        chunks = [st.encode_packed_rows_chunk(x[:, a * N0:(a + k) * N0].contiguous())[:2] for st, x in zip(sts, xs)]
        got = dst.route_packed_rows(chunks, ROUTES3, None, True)
        assert torch.equal(got[0].view(3, B, k, C, rb), rows[:, :, a:a + k]), (a, k)
        assert torch.equal(got[2], whole[2][:, :, a:a + k]) and torch.equal(got[3], whole[3][:, :, a:a + k])
        a += k
    assert int((whole[3] > 0).sum()) >= 1


@gpu
@pytest.mark.parametrize("pcm16", [False, True])
def test_end_to_end(pcm16):
    """Every output is a packed-rows pair as it is: decode_packed(data'[o], index') equals decode_quantized(*unpack(...))."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    sources = [src.encode_packed_rows(_pcm(N0, 2, 3, 5, seed=32 + i, inject=False))[:2] for i in range(3)]
    out, idx, fits, offset = dst.route_packed_rows(sources, ROUTES3, None, True)
    assert bool(fits.all()) and int(offset.max()) > 0
    for o in range(3):
        codes, sf = dst.psy.unpack(out[o], idx)
        got = dst.decode_packed(out[o], idx, pcm16)
        ref = dst.decode_quantized(codes, sf, pcm16)
        assert int(codes.abs().max()) > 0 and _same(got, ref), (o, _where(got, ref))
