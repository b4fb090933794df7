"""The level of packed rows without decoding, and the selector of the N loudest sources:
``AudioCodec.packed_rows_level`` (the ``AC_IN_PACKED | AC_EMIT_LEVEL`` form of ``ac_encode_fused_ex``, k_level_p at filters_n =
1024), ``PsychoacousticModel.level`` (the composition), and ``AudioCodec.select_loudest`` (``AC_SELECT_ACTIVE``,
k_select_loudest).

Every GPU comparison is ``torch.equal``: the one launch against the composition -- ``unpack``, int64 squares summed per band,
the float32 product with the table of w, the fold tree as tensor adds -- which runs everywhere while ``AC_LEVEL_NOFUSE=1`` is
set, and the composition against the numpy restatement of ``level_reference.py``; the selector's kernel against numpy and, at
65 sources, against the tensor loop.  Before any kernel result is compared, numpy alone must show that the input can tell
wrong kernels apart (``_level_conditions``, ``_select_conditions``).

Seeded defects (scratch builds, not committed), each run once against the 48 GPU cases of this file; no CPU test fails (the
CPU tests hold the numpy restatement and the interface, not the kernel):
* band sums kept in 32 bits (the low word of Q_j): 16 cases fail, all on the ``torch.equal`` of the one launch against the
  composition or on the float64 bound -- the 4 of test_level_fused_composition_numpy, test_level_of_hostile_input, the 10 of
  test_level_at_band_layouts (each carries the hand-made full-scale rows) and test_level_within_the_float64_bound.
  test_level_chip_filling passes: seeded noise at 2730 bits holds no band with Q >= 2^32, which is why the hand-made rows exist.
* the fold tree replaced by a sum in band order: 18 cases fail -- the same 15 comparisons, test_level_chip_filling, test_c_abi
  and test_end_to_end_bridge_of_four (on the energies against numpy's); test_level_within_the_float64_bound passes, as it
  must: the order of the adds does not leave the bound.
The selector's cases, the sizes that run the composition and the tests that compare a route with itself pass in both.
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
import level_reference as lr
from pack_reference import np_pack, np_unpack
from test_encode_quantized_fused import _pcm, _where
from test_mix import _dev, _sources, _upload, _x
from test_quantizer import np_offsets
from test_transrate import _random_rows

gpu = pytest.mark.gpu
F32 = np.float32
N0, M0 = 1024, 64
CAP = _lib.AC_PACK_ROWS_MAX_BITS
HEADER = os.path.join(ROOT, "include", "audiocodec_amd.h")
SHAPES = [(1, 1, 1), (2, 3, 2), (3, 5, 1), (2, 2, 3)]          # (B, K, C): 2, 16, 18 (tail waves in the last workgroup), 18 rows
SEL_SHAPES = [(1, 1, 1), (3, 5, 2), (2, 37, 3)]                # (B, F, C): one frame, a batch and a tail, ten batches of frames

# the worked example of section 8j: four bands of two bins, the last one bad
EX_OFF = np.array([0, 2, 4, 6, 8])
EX_CODES = np.array([3, -4, 1, 0, 100, -200, 7, 7], np.int16).reshape(1, 1, 8, 1)
EX_SF = np.array([0, 5, -3, -128], np.int8).reshape(1, 1, 4, 1)
# ... and of the selector: three sources, five frames, n = 1, release 0.5, gate 1
EX_ENERGY = np.array([[8, 0, 0, 0, 0], [4, 4, 0, 3, 0], [0, 0, 0, 0.5, 9]], F32).reshape(3, 1, 5, 1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _hand_made(rng, off, rows=2):
    """Full-scale rows at width 16 in every band: codes of 30000 and more in magnitude (and the code -32768), so that a band of
    four bins or more has Q >= 2^32; moderate scale factors of every residue mod 4."""
    N, M = int(off[-1]), len(off) - 1
    codes = (rng.integers(30000, 32768, (1, rows, N, 1)) * rng.choice([-1, 1], (1, rows, N, 1))).astype(np.int16)
    codes[0, 0, :2, 0] = [-32768, 32767]
    sf = (rng.integers(-20, 21, (1, rows, M, 1)) // 4 * 4 + np.arange(M)[None, None, :, None] % 4).astype(np.int8)
    return codes, sf


def _level_conditions(codes, sf, off):
    """What numpy alone must show of unpacked rows before a kernel is asked."""
    Q, bad = lr.band_squares(codes, sf, off)
    assert int((Q >= 1 << 32).sum()) >= 1, "no band with Q >= 2^32"
    inexact = (Q >= 1 << 24) & (Q.astype(F32).astype(np.float64) != Q.astype(np.float64))
    assert int(inexact.sum()) >= 1, "no band whose Q is rounded by the conversion to float32"
    good = ~bad & (Q > 0)
    assert set(np.unique(np.asarray(sf).astype(np.int32)[good] & 3).tolist()) == {0, 1, 2, 3}, "not every residue of sf mod 4"
    assert int(bad.any(axis=2).sum()) >= 1, "no row with a bad band"
    e = lr.band_energy(Q, sf, bad)
    assert int((_bits(lr.fold(e)) != _bits(lr.in_band_order(e))).sum()) >= 1, "no row whose fold tree differs from the band-order sum"


def _select_conditions(energy, n, valid, release, gate, state=None):
    """What numpy alone must show of a selector input."""
    active, _, sel, P = lr.np_select(energy, n, valid, release, gate, state)
    now = lr.np_peaks(energy, valid, 0.0, None)                             # the level of the frame alone
    S = P.shape[0]
    tie = any(((P[s] == P[t]) & (P[s] > F32(gate)) & sel[s] & ~sel[t]).any() for s in range(S) for t in range(s + 1, S))
    assert tie, "no tie broken by the index"
    assert int((sel & (now < P)).sum()) >= 1, "no source held only by its release"
    top = P.max(axis=0)
    assert int(((top > 0) & (top <= F32(gate))).sum()) >= 1, "no frame whose loudest source is under the gate"
    assert int(((P > F32(gate)).sum(axis=0) > n).sum()) >= 1, "n is never smaller than the number of sources above the gate"
    return active


def _sel_energy(S, B, F, C, seed):
    """Levels from a few values a factor of four apart (ties, also after a release of 0.5), mostly silence, with a NaN, a
    negative value, -0 and +Inf where the shape has room."""
    rng = np.random.default_rng(seed)
    e = rng.choice(np.array([0, 0, 0, 0, 0.25, 1, 1, 4, 16], F32), (S, B, F, C)).astype(F32)
    e *= (rng.random((S, B, F, 1)) < 0.25)                                   # a source talks in a quarter of the frames
    flat = e.reshape(-1)
    if flat.size >= 16:
        at = rng.choice(flat.size, 4, replace=False)
        flat[at] = [np.nan, -1.0, -0.0, np.inf]
    return e


def _checker(S, B, F, C):
    s, b, f, c = np.ix_(np.arange(S), np.arange(B), np.arange(F), np.arange(C))
    return ((s + b + f + c) % 2).astype(np.uint8)


# ---- CPU: the definition ----------------------------------------------------------------------------------------------
def test_worked_example_row():
    Q, bad = lr.band_squares(EX_CODES, EX_SF, EX_OFF)
    assert Q.ravel().tolist() == [25, 1, 50000, 0] and bad.ravel().tolist() == [False, False, False, True]
    w = lr.weight(np.array([0, 5, -3]))
    assert [float(v).hex() for v in w] == ["0x1.0000000000000p+0", "0x1.6a09e40000000p+2", "0x1.6a09e40000000p-2"]
    e = lr.band_energy(Q, EX_SF, bad)
    assert [float(v).hex() for v in e.ravel()] == ["0x1.9000000000000p+4", "0x1.6a09e40000000p+2", "0x1.1436ac0000000p+14", "0x0.0p+0"]
    E, b = lr.level_of_codes(EX_CODES, EX_SF, EX_OFF)
    # the fold tree at P = 4: (e0 + e2) + (e1 + e3)
    assert float(E[0, 0, 0]).hex() == "0x1.14b14c0000000p+14" and int(b[0, 0, 0]) == 1
    assert float(E[0, 0, 0]) == float(F32(F32(e.ravel()[0] + e.ravel()[2]) + F32(e.ravel()[1] + e.ravel()[3])))
    data, index = np_pack(EX_CODES, EX_SF, EX_OFF)
    E2, b2 = lr.np_level(data, index, EX_OFF, 8)                            # (unpack zeroes the bad band's codes: the same level)
    assert _bits(E2) == _bits(E) and b2 == b


def test_worked_example_selector():
    active, state, sel, P = lr.np_select(EX_ENERGY, 1, None, 0.5, 1.0)
    assert P[:, 0].tolist() == [[8, 4, 2, 1, 0.5], [4, 4, 2, 3, 1.5], [0, 0, 0, 0.5, 9]]
    # frame 1 and 2: a tie, the lower index wins, held by its release alone; frame 3: source 0 sits at the gate, not above it
    assert sel[:, 0].astype(int).tolist() == [[1, 1, 1, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 1]]
    assert state.ravel().tolist() == [0.5, 1.5, 9.0] and np.array_equal(active[..., 0], sel.astype(np.uint8))
    # four silent frames more: every peak falls under the gate, and nobody is selected
    longer = np.concatenate([EX_ENERGY, np.zeros((3, 1, 4, 1), F32)], axis=2)
    _select_conditions(longer, 1, None, 0.5, 1.0)
    assert not lr.np_select(longer, 1, None, 0.5, 1.0)[0][:, :, 8].any()


@pytest.mark.parametrize("sr,N,M", [(44100, 256, 48), (48000, 128, 64)])
def test_consequences_of_the_level(sr, N, M):
    off = np_offsets(sr, N, M)
    rng = np.random.default_rng(N)
    codes, sf = _random_rows(rng, off, 2, 3, 2)                              # non-canonical, with -128 bands and junk codes in them
    hc, hs = _hand_made(rng, off, 6)
    codes = np.concatenate([codes, hc.reshape(2, 3, N, 1).repeat(2, axis=3)], axis=0)
    sf = np.concatenate([sf, hs.reshape(2, 3, M, 1).repeat(2, axis=3)], axis=0)
    _level_conditions(codes, sf, off)
    data, index = np_pack(codes, sf, off)
    E, bad = lr.np_level(data, index, off, N)
    E0, bad0 = lr.level_of_codes(codes, sf, off)                             # packing loses nothing the level needs
    assert np.array_equal(_bits(E), _bits(E0)) and np.array_equal(bad, bad0)
    assert E.dtype == F32 and bad.dtype == np.uint8 and np.isfinite(E).all() and (E >= 0).all() and not np.signbit(E).any()
    assert np.array_equal(bad, (sf == -128).any(axis=2).astype(np.uint8)) and 0 < int(bad.sum()) < bad.size
    # (a) within 2^-20 relative of the float64 sum over the good bands: at most 11 roundings of 2^-24
    ref = lr.exact_energy(*np_unpack(data, index, off, N), off)
    assert (np.abs(E.astype(np.float64) - ref) <= 2.0 ** -20 * ref).all()
    # (b) a row of zero bytes
    Ez, bz = lr.np_level(np.zeros(64, np.uint8), np.zeros((1, 1, 1), np.int64), off, N)
    assert _bits(Ez).tolist() == [[[0]]] and bz.tolist() == [[[0]]]
    # (c) every sf + 4 quadruples E exactly, while no sf clamps
    room = np.where(sf == -128, -128, np.clip(sf, -127, 100)).astype(np.int8)
    up = np.where(room == -128, -128, room + 4).astype(np.int8)
    Ea, Eb = lr.level_of_codes(codes, room, off)[0], lr.level_of_codes(codes, up, off)[0]
    assert np.array_equal(_bits(Eb), _bits(Ea * F32(4))) and (Ea > 0).any()
    # (d) a slice and a permutation of the index, and rows moved behind other bytes, row for row
    E1, b1 = lr.np_level(data, index[:, 1:], off, N)
    assert np.array_equal(_bits(E1), _bits(E[:, 1:])) and np.array_equal(b1, bad[:, 1:])
    E2, _ = lr.np_level(np.concatenate([np.full(12, 0xFF, np.uint8), data]), index[::-1] + 12, off, N)
    assert np.array_equal(_bits(E2), _bits(E[::-1]))


def test_consequences_of_the_selector():
    S, B, F, C = 4, 3, 37, 2
    e = _sel_energy(S, B, F, C, 3)
    valid = (np.random.default_rng(4).random((S, B, F, C)) < 0.8).astype(np.uint8)
    _select_conditions(e, 2, valid, 0.5, 0.5)
    assert not lr.np_select(e, 0, valid)[0].any()                                               # n = 0
    everyone, _, _, P = lr.np_select(e, S, valid, 0.5, 0.0)                                     # n >= S with gate 0
    assert np.array_equal(everyone, ((P > 0)[..., None] & (valid != 0)).astype(np.uint8))
    for n in (1, 2, 3):
        active, _, sel, _ = lr.np_select(e, n, valid, 0.5, 0.5)
        assert int(sel.sum(axis=0).max()) == n and (active <= valid).all()
    # permuting sources with distinct peaks permutes active
    rng = np.random.default_rng(5)
    d = rng.random((S, B, F, C)).astype(F32) + F32(0.01)
    perm = np.array([2, 0, 3, 1])
    seen = valid.copy()
    seen[:, :, 0, 0] = 1                                                     # (no two sources silent from the start: no tie at 0)
    a, _, _, P = lr.np_select(d, 2, seen, 0.5, 0.1)
    assert all(len(np.unique(P[:, b, f])) == S for b in range(B) for f in range(F))
    assert np.array_equal(lr.np_select(d[perm], 2, seen[perm], 0.5, 0.1)[0], a[perm])
    # release = 0 has no memory: every frame alone gives its frame of the whole
    whole = lr.np_select(e, 2, valid, 0.0, 0.5)[0]
    for f in (0, 7, F - 1):
        assert np.array_equal(lr.np_select(e[:, :, f:f + 1], 2, valid[:, :, f:f + 1], 0.0, 0.5)[0], whole[:, :, f:f + 1])
    # any split of F with state carried equals the one-shot call, bit for bit
    one, st1, _, _ = lr.np_select(e, 2, valid, 0.5, 0.5)
    for cuts in ((1, 36), (18, 19), (5, 1, 30, 1)):
        state, a0, parts = None, 0, []
        for k in cuts:
            act, state, _, _ = lr.np_select(e[:, :, a0:a0 + k], 2, valid[:, :, a0:a0 + k], 0.5, 0.5, state)
            parts.append(act)
            a0 += k
        assert np.array_equal(np.concatenate(parts, axis=2), one) and np.array_equal(_bits(state), _bits(st1))


# ---- CPU: header, library, Python validation ------------------------------------------------------------------------------
def test_header_declares_the_flags_the_struct_and_the_query():
    text = open(HEADER).read()
    assert re.search(r"\bAC_EMIT_LEVEL\s*=\s*4096\b", text) and re.search(r"\bAC_SELECT_ACTIVE\s*=\s*8192\b", text)
    assert re.search(r"#define\s+AC_SELECT_MAX_SOURCES\s+64\b", text)
    m = re.search(r"typedef\s+struct\s+ac_select_rows\s*\{(.*?)\}\s*ac_select_rows\s*;", text, flags=re.S)
    assert m, "ac_select_rows is not declared"
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["int32_t sources_n", "const float* energy", "const uint8_t* valid", "int32_t n", "float release", "float gate",
                      "float* state"], fields
    m = re.search(r"AC_API\s+int\s+ac_level_launches\s*\(([^;]*)\)\s*;", text)
    assert m and "stream" not in m.group(1) and m.group(1).count(",") == 1, m and m.group(1)
    assert re.search(r"#define\s+AC_VERSION\s+171\b", text)
    said = " ".join(text[text.index("Library launches of the level"):text.index("ac_level_launches(const")].replace("*", " ").split())
    for words in ("1 = ac_encode_fused_ex with AC_IN_PACKED | AC_EMIT_LEVEL serves it", "0 = the library has no launch of its own",
                  "AC_LEVEL_NOFUSE=1", "NULL plan or C < 1"):
        assert words in said, words


def test_library_exports_the_query():
    lib = _lib.load()
    assert "ac_level_launches" in _lib.PROTOTYPES and callable(lib.ac_level_launches)
    assert lib.ac_level_launches(None, 2) == 0
    assert lib.ac_version() == 171
    assert _lib.AC_EMIT_LEVEL == 4096 and _lib.AC_SELECT_ACTIVE == 8192 and _lib.AC_SELECT_MAX_SOURCES == 64


def test_ctypes_mirror_has_the_headers_layout():
    Q = _lib.SelectRows
    assert [f[0] for f in Q._fields_] == ["sources_n", "energy", "valid", "n", "release", "gate", "state"]
    assert (Q.sources_n.offset, Q.energy.offset, Q.valid.offset, Q.n.offset, Q.release.offset, Q.gate.offset, Q.state.offset) == \
        (0, 8, 16, 24, 28, 32, 40) and ctypes.sizeof(Q) == 48


def test_python_interface_validates_its_arguments():
    codec = audiocodec_amd.AudioCodec(48000, N0)
    data, index = torch.zeros(64, dtype=torch.uint8), torch.zeros((1, 1, 2), dtype=torch.int64)
    for bad in ((data.to(torch.int8), index), (data, index.to(torch.int32)), (data.view(8, 8), index), (data, index[0]), (data, index)):
        with pytest.raises(ValueError):                       # the last: host tensors
            codec.packed_rows_level(*bad)
    with pytest.raises(TypeError):
        codec.packed_rows_level(data.numpy(), index)
    with pytest.raises(NotImplementedError, match="float32"):
        audiocodec_amd.AudioCodec(48000, N0, compute_dtype=torch.float64).packed_rows_level(data, index)
    e = torch.zeros((3, 1, 2, 2))
    with pytest.raises(ValueError, match="energy"):
        codec.select_loudest([], 0)
    with pytest.raises(ValueError, match="energy"):
        codec.select_loudest(e[0], 1)                          # three dimensions: not a stacked tensor
    for bad in (1.0, True, None, "2"):
        with pytest.raises(TypeError, match="n must"):
            codec.select_loudest(e, bad)
    for bad in (-1, 4):
        with pytest.raises(ValueError, match=r"n \("):
            codec.select_loudest(e, bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="release"):
            codec.select_loudest(e, 1, release=bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="gate"):
            codec.select_loudest(e, 1, gate=bad)
    for name in ("release", "gate"):
        with pytest.raises(TypeError, match=name):
            codec.select_loudest(e, 1, **{name: "0.5"})
    with pytest.raises(ValueError, match="energy"):           # host tensors
        codec.select_loudest(e, 1)
    with pytest.raises(ValueError, match="energy of source 0"):
        codec.select_loudest([e[0].double(), e[1]], 1)
    assert "slow" in codec.select_loudest.__doc__


# ---- GPU ------------------------------------------------------------------------------------------------------------------
class _nofuse:
    """AC_LEVEL_NOFUSE=1 (read per call) around a block."""

    def __enter__(self):
        os.environ["AC_LEVEL_NOFUSE"] = "1"

    def __exit__(self, *exc):
        del os.environ["AC_LEVEL_NOFUSE"]
        return False


def _composition(codec, data, index):
    with _nofuse():
        assert codec.packed_rows_level_launches(index.shape[2]) == 0
        return codec.packed_rows_level(data, index, True)


def _three_ways(codec, data, index, off, what="", N=N0):
    """numpy, the composition and the one launch on the same rows: returns numpy's (energy, bad)."""
    ref = lr.np_level(data.cpu().numpy(), index.cpu().numpy(), off, N)
    comp = _composition(codec, data, index)
    assert codec.packed_rows_level_launches(index.shape[2]) == 1
    fused = codec.packed_rows_level(data, index, True)
    assert torch.equal(codec.packed_rows_level(data, index), fused[0])
    for name, g, c, r in zip(("energy", "bad"), fused, comp, ref):
        assert g.dtype == c.dtype == torch.from_numpy(r).dtype and g.shape == index.shape
        assert torch.equal(c.cpu(), torch.from_numpy(r)), (name, what, _where(c.cpu(), torch.from_numpy(r)))
        assert torch.equal(g, c), (name, what, _where(g, c))
    return ref


def _with_hand_made(data, index, off, seed):
    """The rows with their last two replaced by hand-made full-scale rows appended to data: (data', index') on the device."""
    hd, hi = np_pack(*_hand_made(np.random.default_rng(seed), off), off)
    d, i = data.cpu().numpy(), index.cpu().numpy().copy()
    flat = i.reshape(-1)
    flat[-2:] = len(d) + hi.reshape(-1)[:2]
    return _upload(np.concatenate([d, hd]), i)


@gpu
@pytest.mark.parametrize("B,K,C", SHAPES)
def test_level_fused_composition_numpy(B, K, C):
    """Dense rows, fixed-stride rows at four budgets, protected slots, a permuted and a sliced index; consequence (d)."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    x = _x(B, K, C, 40 + B)
    held = base.with_row_budget(2730).encode_packed_rows(x)[:2]
    data, index = _with_hand_made(*held, off, B)
    if B >= 3:                                                               # (the shape whose input carries NaN and Inf)
        _level_conditions(*np_unpack(data.cpu().numpy(), index.cpu().numpy(), off, N0), off)
    ref = _three_ways(base, data, index, off, "2730 and hand-made")
    assert float(ref[0].max()) > 0
    _three_ways(base, *base.encode_packed(x), off, "dense")
    for R in (1365, 320, CAP):
        cbr = base.with_row_budget(R)
        d, i = cbr.encode_packed_rows(x)[:2]
        e = _three_ways(cbr, d, i, off, "fixed stride at %d" % R)
        if R == 1365:                                                        # protected slots: the primary part is the transrated row
            t = cbr.transrate_packed_rows(*held)
            p = cbr.protect_packed_rows(*held, 400)
            et, ep = _three_ways(cbr, t[0], t[1], off, "transrated"), _three_ways(cbr, p[0], p[1], off, "protected")
            assert np.array_equal(_bits(et[0]), _bits(ep[0])) and np.array_equal(et[1], ep[1])
    perm = index.flip(0, 1, 2)[:, ::2].contiguous()                              # permuted and sliced: row for row
    got = _three_ways(base, data, perm, off, "permuted")
    want = np.ascontiguousarray(ref[0][::-1, ::-1, ::-1][:, ::2])
    assert np.array_equal(_bits(got[0]), _bits(want))


@gpu
def test_level_of_a_streams_chunks():
    base = audiocodec_amd.AudioCodec(48000, N0)
    src = base.with_row_budget(2730)
    B, K, C = 3, 5, 2
    x = _x(B, K, C, 31)
    whole = base.packed_rows_level(*src.encode_packed_rows(x)[:2], return_bad=True)
    st, a = src.stream(B, C), 0
    for k in (2, 1, 2):
        d, i = st.encode_packed_rows_chunk(x[:, a * N0:(a + k) * N0].contiguous())[:2]
        e, bad = base.packed_rows_level(d, i, True)
        assert torch.equal(e, whole[0][:, a:a + k]) and torch.equal(bad, whole[1][:, a:a + k]), (a, k)
        a += k
    assert float(whole[0].max()) > 0


@gpu
def test_level_of_hostile_input():
    """Damaged, random and truncated data; row starts that are negative, past the end and off the 4-byte phase; marked rows;
    all-zero rows; the NaN / Inf-carrying input of test_encode_cbr._input (in _x at this shape)."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    B, K, C = 3, 5, 2
    d, i = base.with_row_budget(2730).encode_packed_rows(_x(B, K, C, 61))[:2]
    ref = _three_ways(base, d, i, off, "as encoded")
    assert int(ref[1].sum()) >= 1 and int((ref[1] == 0).sum()) >= 1          # the NaN / Inf frames arrived as bad rows
    data, index = d.cpu().numpy(), i.cpu().numpy()
    bits = np.unpackbits(data, bitorder="little")
    start = int(index[0, 2, 0]) * 8
    for j, wv in ((3, 17), (10, 30), (40, 23)):                              # widths 17 .. 30 read as 31
        bits[start + 5 * j:start + 5 * j + 5] = [(wv >> k) & 1 for k in range(5)]
    start = int(index[1, 1, 1]) * 8 + 5 * M0
    bits[start:start + 8] = [0, 0, 0, 0, 0, 0, 0, 1]                         # a stored scale-factor byte of -128
    dam = _three_ways(base, *_upload(np.packbits(bits, bitorder="little"), index), off, "damaged")
    assert dam[1][0, 2, 0] == 1 and dam[1][1, 1, 1] == 1
    rng = np.random.default_rng(8)
    _three_ways(base, *_upload(rng.integers(0, 256, data.shape).astype(np.uint8), index), off, "random bytes")
    for cut in (int(index[2, 5, 1]) + 100, int(index[2, 5, 1]) + 13, int(index[2, 3, 0]) + 2):
        _three_ways(base, *_upload(data[:cut], index), off, "truncated at %d" % cut)
    odd = index.copy()
    odd[0, 0, 0], odd[0, 1, 1], odd[0, 2, 0], odd[0, 3, 1], odd[0, 4, 0] = -7, len(data) + 1000, index[0, 2, 0] + 1, -(1 << 50), len(data) - 3
    odd[0, 5, 0], odd[1, 0, 0], odd[1, 0, 1] = (1 << 40), index[1, 0, 0] + 2, index[1, 0, 1] + 3
    got = _three_ways(base, *_upload(data, odd), off, "odd row starts")
    assert _bits(got[0][0, 1, 1]) == 0 and got[1][0, 1, 1] == 0              # a row past the end: +0, not bad
    small = base.with_row_budget(320).encode_packed_rows(_x(B, K, C, 62))    # marked rows: what the 320-bit budget cannot hold
    assert int((~small[2]).sum()) >= 1
    got = _three_ways(base, small[0], small[1], off, "marked rows")
    unfit = ~small[2].cpu().numpy()
    assert (got[1][unfit] == 1).all() and (_bits(got[0][unfit]) == 0).all()
    zero = _three_ways(base, torch.zeros(4096, dtype=torch.uint8, device="cuda"), i[:1].clamp(max=2048).contiguous(), off, "zero bytes")
    assert not _bits(zero[0]).any() and not zero[1].any()


@gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("layout", fl.LAYOUTS, ids=fl.LAYOUT_IDS)
def test_level_at_band_layouts(layout, C):
    """One-bin bands, granules that straddle bands and empty bands (fused_layouts.LAYOUTS), on its ``tonal`` input."""
    sr, alpha = fl.resolve(layout)
    base = audiocodec_amd.AudioCodec(sr, N0, alpha=alpha)
    off = base.psy.scale_band_offsets
    d, i = base.with_row_budget(2730).encode_packed_rows(torch.from_numpy(fl.tonal(C)).cuda())[:2]
    ref = _three_ways(base, *_with_hand_made(d, i, off, 3), off, layout[0])
    assert float(ref[0].max()) > 0


@gpu
@pytest.mark.parametrize("sr,N,M,C", [(48000, 2048, 64, 2), (48000, 960, 64, 1), (44100, 256, 48, 3)])
def test_the_composition_at_other_sizes(sr, N, M, C):
    """PsychoacousticModel.level serves every plan the quantiser serves: random non-canonical rows and hand-made full-scale ones
    against numpy, from codes and through packed_rows_level (the query is 0)."""
    base = audiocodec_amd.AudioCodec(sr, N, bark_bands_n=M)
    off = base.psy.scale_band_offsets
    rng = np.random.default_rng(N + C)
    codes, sf = _random_rows(rng, off, 2, 3, C)
    hc, hs = _hand_made(rng, off, 3)
    codes[1, :, :, 0], sf[1, :, :, 0] = hc[0, :, :, 0], hs[0, :, :, 0]
    _level_conditions(codes, sf, off)
    want = lr.level_of_codes(codes, sf, off)
    got = base.psy.level(_dev(codes), _dev(sf))
    assert torch.equal(got[0].cpu(), torch.from_numpy(want[0])) and torch.equal(got[1].cpu(), torch.from_numpy(want[1]))
    assert base.packed_rows_level_launches(C) == 0
    data, index = np_pack(codes, sf, off)
    got = base.packed_rows_level(*_upload(data, index), return_bad=True)
    want = lr.np_level(data, index, off, N)
    assert torch.equal(got[0].cpu(), torch.from_numpy(want[0])) and torch.equal(got[1].cpu(), torch.from_numpy(want[1]))


@gpu
def test_level_launch_table(monkeypatch):
    base = audiocodec_amd.AudioCodec(48000, N0)
    lib = _lib.load()
    plan = base.psy._plan(torch.device("cuda", torch.cuda.current_device()))
    assert lib.ac_level_launches(plan, 0) == 0 and lib.ac_level_launches(plan, -1) == 0 and lib.ac_level_launches(None, 2) == 0
    for C in (1, 2, 3, 7):
        assert base.packed_rows_level_launches(C) == 1                       # no row budget needed
        for R in (320, 1365, CAP, CAP + 32):
            assert base.with_row_budget(R).packed_rows_level_launches(C) == 1, (C, R)
    for N, M in ((2048, 64), (960, 64), (1024, 32)):
        assert audiocodec_amd.AudioCodec(48000, N, bark_bands_n=M).packed_rows_level_launches(2) == 0
    monkeypatch.setenv("AC_LEVEL_NOFUSE", "1")
    assert base.packed_rows_level_launches(2) == 0
    monkeypatch.delenv("AC_LEVEL_NOFUSE")
    assert base.packed_rows_level_launches(2) == 1
    monkeypatch.setenv("AC_TRANSRATE_NOFUSE", "1")                           # a switch of its own
    assert base.packed_rows_level_launches(2) == 1


@gpu
def test_level_chip_filling():
    """8224 rows -- 2056 workgroups of four waves -- of seeded noise at many levels against the composition, and the float64
    bound of consequence (a) on them."""
    B, K, C = 16, 256, 2
    base = audiocodec_amd.AudioCodec(48000, N0)
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.rand((B, K * N0, C), generator=g, device="cuda") * 2 - 1
    x *= torch.logspace(-3, 0, B, device="cuda")[:, None, None] * torch.linspace(0.05, 1, K * N0, device="cuda")[None, :, None]
    x[3] = 0.0                                                               # 514 all-zero rows
    d, i = base.with_row_budget(2730).encode_packed_rows(x)[:2]
    assert i.numel() == 8224 and base.packed_rows_level_launches(C) == 1
    fused = base.packed_rows_level(d, i, True)
    comp = _composition(base, d, i)
    for name, a, b in zip(("energy", "bad"), fused, comp):
        assert torch.equal(a, b), (name, _where(a, b))
    e = fused[0]
    assert int((e[3] == 0).sum()) == 514 and int((e > 0).sum()) >= 4000 and not bool(fused[1].any())
    codes, sf = base.psy.unpack(d, i)
    X = base.psy.dequantize(codes, sf).double()
    ref = (X * X).sum(dim=2)
    assert bool(((e.double() - ref).abs() <= 2.0 ** -20 * ref).all())


@gpu
def test_level_within_the_float64_bound():
    """Consequence (a) on full-scale and damaged rows: the good bands' float64 sum of dequantize(unpack(row))^2."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    d, i = base.with_row_budget(2730).encode_packed_rows(_x(3, 5, 2, 61))[:2]
    data, index = _with_hand_made(d, i, off, 9)
    e, bad = base.packed_rows_level(data, index, True)
    codes, sf = np_unpack(data.cpu().numpy(), index.cpu().numpy(), off, N0)
    _level_conditions(codes, sf, off)
    ref = lr.exact_energy(codes, sf, off)
    err = np.abs(e.cpu().numpy().astype(np.float64) - ref)
    assert (err <= 2.0 ** -20 * ref).all(), float((err / np.maximum(ref, 1e-300)).max())
    assert int(bad.sum()) >= 1 and float(ref.max()) >= 2.0 ** 36


def _select_numpy(codec, e, n, valid, release, gate, state=None, what=""):
    """select_loudest on the device against numpy: active and the state left behind."""
    st = None if state is None else _dev(state)
    got = codec.select_loudest(_dev(e), n, None if valid is None else _dev(valid), release, gate, st)
    want, st_want, _, _ = lr.np_select(e, n, valid, release, gate, state)
    assert got.dtype == torch.uint8 and got.shape == e.shape
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (what, _where(got.cpu(), torch.from_numpy(want)))
    if st is not None:
        assert torch.equal(st.cpu().view(torch.int32), torch.from_numpy(st_want).view(torch.int32)), what
    return got


@gpu
@pytest.mark.parametrize("B,F,C", SEL_SHAPES)
@pytest.mark.parametrize("S", [1, 2, 3, 8, 64])
def test_select_kernel_against_numpy(S, B, F, C):
    codec = audiocodec_amd.AudioCodec(48000, N0)
    e = _sel_energy(S, B, F, C, 100 * S + F)
    rng = np.random.default_rng(S)
    state = rng.choice(np.array([0, 0.5, 2, 32], F32), (S, B)).astype(F32)
    masks = {"all": None, "off": np.zeros(e.shape, np.uint8), "checkerboard": _checker(S, B, F, C),
             "bool": (rng.random(e.shape) < 0.8)}
    for n in sorted({0, 1, min(2, S), S}):
        for release in (0.0, 0.5, 1.0):
            for gate in (0.0, 0.5):
                for name, valid in masks.items():
                    what = (n, release, gate, name)
                    got = _select_numpy(codec, e, n, valid, release, gate, None, what)
                    assert int(got.any(dim=3).sum(dim=0).max()) <= n, what
                _select_numpy(codec, e, n, masks["checkerboard"], release, gate, state, (n, release, gate, "state"))
    a = codec.select_loudest([_dev(e[s]) for s in range(S)], min(1, S))      # a list of sources is the stacked tensor
    assert torch.equal(a, codec.select_loudest(_dev(e), min(1, S)))


@gpu
def test_select_conditions_and_splits():
    """On an input that numpy shows to hold a tie, a held source, a gated one and more candidates than n: three splits of F
    with state carried against the one-shot call."""
    codec = audiocodec_amd.AudioCodec(48000, N0)
    S, B, F, C = 4, 3, 37, 2
    e = _sel_energy(S, B, F, C, 3)
    valid = (np.random.default_rng(4).random((S, B, F, C)) < 0.8).astype(np.uint8)
    _select_conditions(e, 2, valid, 0.5, 0.5)
    st1 = torch.zeros((S, B), device="cuda")
    one = _select_numpy(codec, e, 2, valid, 0.5, 0.5, np.zeros((S, B), F32))
    de, dv = _dev(e), _dev(valid)
    assert torch.equal(codec.select_loudest(de, 2, dv, 0.5, 0.5, st1), one)
    for cuts in ((1, 36), (18, 19), (5, 1, 30, 1)):
        state, a0, parts = torch.zeros((S, B), device="cuda"), 0, []
        for k in cuts:
            parts.append(codec.select_loudest(de[:, :, a0:a0 + k].contiguous(), 2, dv[:, :, a0:a0 + k].contiguous(), 0.5, 0.5, state))
            a0 += k
        assert torch.equal(torch.cat(parts, dim=2), one), cuts
        assert torch.equal(state.view(torch.int32), st1.view(torch.int32)), cuts


@gpu
def test_select_65_sources_run_the_loop():
    codec = audiocodec_amd.AudioCodec(48000, N0)
    S, B, F, C = 65, 2, 7, 2
    e = _sel_energy(S, B, F, C, 65)
    state = np.random.default_rng(65).choice(np.array([0, 0.5, 2], F32), (S, B)).astype(F32)
    for n, release, gate, valid in ((2, 0.5, 0.5, _checker(S, B, F, C)), (65, 1.0, 0.0, None), (0, 0.0, 0.0, None), (7, 0.0, 0.25, None)):
        _select_numpy(codec, e, n, valid, release, gate, state.copy(), (n, release, gate))
    lib = _lib.load()
    de, out = _dev(e), torch.full(e.shape, 0xA5, dtype=torch.uint8, device="cuda")
    assert _select_abi(codec, de, out, 2) == _lib.AC_EUNSUPPORTED and b"AC_SELECT_MAX_SOURCES" in lib.ac_last_error()
    assert bool((out == 0xA5).all())
    # ... and the loop gives the kernel's bits where both serve
    e64 = _sel_energy(64, B, F, C, 64)
    pad = np.concatenate([e64, np.zeros((1, B, F, C), F32)])
    got = codec.select_loudest(_dev(pad), 3, None, 0.5, 0.25)
    assert torch.equal(got[:64], codec.select_loudest(_dev(e64), 3, None, 0.5, 0.25)) and not bool(got[64].any())


def _p(v):
    return ctypes.c_void_p(v.data_ptr()) if v is not None else None


def _level_abi(codec, data, index, energy, bad=None, flags=None, X=None, t=None, thr=None, src=True, B=None, nbytes=None, null_index=False):
    lib = _lib.load()
    dev = index.device
    rows = _lib.PackedRows(data.data_ptr(), data.numel() if nbytes is None else nbytes, None if null_index else index.data_ptr())
    st = lib.ac_encode_fused_ex(codec.mdct._plan(dev), codec.psy._plan(dev), ctypes.addressof(rows) if src else None, _p(X), _p(t),
                                _p(thr), 0.0, (_lib.AC_IN_PACKED | _lib.AC_EMIT_LEVEL) if flags is None else flags, _p(energy),
                                _p(bad), 0, index.shape[0] if B is None else B, index.shape[1] - 1, index.shape[2], None)
    torch.cuda.synchronize()
    return st


def _select_abi(codec, energy, active, n, valid=None, release=0.5, gate=0.0, state=None, flags=None, X=None, t=None, thr=None,
                out1=None, src=True, S=None, null_energy=False, B=None):
    lib = _lib.load()
    dev = energy.device
    sel = _lib.SelectRows(energy.shape[0] if S is None else S, None if null_energy else energy.data_ptr(),
                          valid.data_ptr() if valid is not None else None, n, release, gate,
                          state.data_ptr() if state is not None else None)
    st = lib.ac_encode_fused_ex(codec.mdct._plan(dev), codec.psy._plan(dev), ctypes.addressof(sel) if src else None, _p(X), _p(t),
                                _p(thr), 0.0, _lib.AC_SELECT_ACTIVE if flags is None else flags, _p(active), _p(out1), 0,
                                energy.shape[1] if B is None else B, energy.shape[2] - 1, energy.shape[3], None)
    torch.cuda.synchronize()
    return st


@gpu
def test_c_abi():
    lib = _lib.load()
    base = audiocodec_amd.AudioCodec(48000, N0)
    d, i = base.with_row_budget(2730).encode_packed_rows(_x(3, 5, 2, 17))[:2]
    energy = torch.full((3, 6, 2), -7.0, device="cuda")
    bad = torch.full((3, 6, 2), 0xA5, dtype=torch.uint8, device="cuda")
    spare = torch.zeros((3, 6, N0, 2), device="cuda")
    refused = (energy.clone(), bad.clone())
    IN, EMIT, LEVEL, SEL = _lib.AC_IN_PACKED, _lib.AC_EMIT_PACKED, _lib.AC_EMIT_LEVEL, _lib.AC_SELECT_ACTIVE
    for flags in (LEVEL, LEVEL | EMIT, LEVEL | IN | EMIT, LEVEL | IN | _lib.AC_IN_MIX, LEVEL | IN | _lib.AC_IN_ROUTE, LEVEL | IN | SEL,
                  LEVEL | IN | _lib.AC_IN_PCM16, LEVEL | IN | _lib.AC_EMIT_CODES, LEVEL | IN | 128, LEVEL | IN | 16384):
        assert _level_abi(base, d, i, energy, bad, flags=flags) == _lib.AC_EINVAL, flags
        assert lib.ac_last_error()
    for kw in ({"X": spare}, {"t": spare}, {"thr": spare}, {"src": False}, {"nbytes": -1}, {"null_index": True}):
        assert _level_abi(base, d, i, energy, bad, **kw) == _lib.AC_EINVAL, kw
    assert _level_abi(base, d, i, None, bad) == _lib.AC_EINVAL
    wide = audiocodec_amd.AudioCodec(48000, 2048)
    assert _level_abi(wide, d, i, energy, bad) == _lib.AC_EUNSUPPORTED and b"composition" in lib.ac_last_error()
    with _nofuse():
        assert _level_abi(base, d, i, energy, bad) == _lib.AC_EUNSUPPORTED
    for got, want in zip((energy, bad), refused):                            # the refused calls wrote nothing
        assert torch.equal(got, want)
    assert _level_abi(base, d, i, energy, bad, B=0) == _lib.AC_OK and torch.equal(energy, refused[0])
    assert _level_abi(base, d, i, energy, bad) == _lib.AC_OK, lib.ac_last_error()
    ref = _composition(base, d, i)
    assert torch.equal(energy, ref[0]) and torch.equal(bad, ref[1])
    energy.fill_(-7.0)
    assert _level_abi(base.with_row_budget(1365), d, i, energy) == _lib.AC_OK and torch.equal(energy, ref[0])   # out1 may be NULL

    S = 3
    e = _dev(_sel_energy(S, 3, 6, 2, 1))
    valid = _dev(_checker(S, 3, 6, 2))
    active = torch.full((S, 3, 6, 2), 0xA5, dtype=torch.uint8, device="cuda")
    state = torch.full((S, 3), 2.0, device="cuda")
    for flags in (SEL | IN, SEL | EMIT, SEL | IN | EMIT, SEL | _lib.AC_IN_MIX, SEL | _lib.AC_EMIT_NOISY, SEL | 16384):
        assert _select_abi(base, e, active, 2, valid, state=state, flags=flags) == _lib.AC_EINVAL, flags
    for kw in ({"X": spare}, {"t": spare}, {"thr": spare}, {"out1": spare}, {"src": False}, {"S": 0}, {"S": -1}, {"null_energy": True},
               {"release": -0.5}, {"release": 1.5}, {"release": float("nan")}, {"gate": -1.0}, {"gate": float("nan")}):
        assert _select_abi(base, e, active, 2, valid, state=state, **kw) == _lib.AC_EINVAL, kw
        assert lib.ac_last_error()
    for n in (-1, S + 1):
        assert _select_abi(base, e, active, n, valid, state=state) == _lib.AC_EINVAL
    assert _select_abi(base, e, None, 2, valid, state=state) == _lib.AC_EINVAL
    assert _select_abi(base, e, active, 2, valid, state=state, S=65) == _lib.AC_EUNSUPPORTED
    assert bool((active == 0xA5).all()) and bool((state == 2.0).all())       # the refused calls wrote nothing
    assert _select_abi(base, e, active, 2, valid, state=state, B=0) == _lib.AC_OK and bool((active == 0xA5).all())
    assert _select_abi(base, e, active, 2, valid, 0.5, 0.25, state) == _lib.AC_OK, lib.ac_last_error()
    want, st_want, _, _ = lr.np_select(e.cpu().numpy(), 2, valid.cpu().numpy(), 0.5, 0.25, np.full((S, 3), 2.0, F32))
    assert torch.equal(active.cpu(), torch.from_numpy(want)) and torch.equal(state.cpu(), torch.from_numpy(st_want))
    assert _select_abi(base, e, active, 1) == _lib.AC_OK                     # valid and state may be NULL
    assert torch.equal(active.cpu(), torch.from_numpy(lr.np_select(e.cpu().numpy(), 1)[0]))
    # the refusals other tests assert of the older forms still hold with the new bits beside them
    assert _level_abi(base.with_row_budget(1365), d, i, energy, bad, flags=_lib.AC_IN_ROUTE | IN | EMIT | LEVEL) == _lib.AC_EINVAL


@gpu
def test_python_interface_validates_device_tensors():
    codec = audiocodec_amd.AudioCodec(48000, N0)
    e = torch.zeros((3, 1, 2, 2), device="cuda")
    with pytest.raises(ValueError, match="energy of source 1"):
        codec.select_loudest([e[0], e[1, :, :1]], 1)
    for bad in (torch.ones((3, 1, 2, 1), dtype=torch.uint8, device="cuda"), torch.ones((3, 1, 2, 2), dtype=torch.int32, device="cuda"),
                torch.ones((3, 1, 2, 2), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="valid"):
            codec.select_loudest(e, 1, valid=bad)
    with pytest.raises(TypeError, match="valid"):
        codec.select_loudest(e, 1, valid=np.ones((3, 1, 2, 2), np.uint8))
    for bad in (torch.zeros((3, 2), device="cuda"), torch.zeros((3, 1), dtype=torch.float64, device="cuda"), torch.zeros((3, 1)),
                torch.zeros((3, 2), device="cuda")[:, :1]):
        with pytest.raises(ValueError, match="state"):
            codec.select_loudest(e, 1, state=bad)
    with pytest.raises(TypeError, match="state"):
        codec.select_loudest(e, 1, state=np.zeros((3, 1), F32))
    for shape in ((0, 3, 2), (2, 0, 2)):                                     # empty shapes give empty results
        idx = torch.zeros(shape, dtype=torch.int64, device="cuda")
        got = codec.packed_rows_level(torch.zeros(64, dtype=torch.uint8, device="cuda"), idx, True)
        assert got[0].shape == shape and got[0].dtype == torch.float32 and got[1].shape == shape and got[1].dtype == torch.uint8
        assert codec.select_loudest(torch.zeros((2,) + shape, device="cuda"), 1).shape == (2,) + shape


@pytest.fixture(scope="module")
def harness():
    from stream_order import Harness
    return Harness()


def _calls(codec, route):
    def level(d, i):
        return codec.packed_rows_level(d, i, True) if route == "fused" else _composition(codec, d, i)

    def select(e, v, st0):
        st = st0.clone()                                                     # (the call updates its state in place)
        return codec.select_loudest(e, 2, v, 0.5, 0.25, st), st
    return level, select


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
@pytest.mark.parametrize("check", ["delayed_producer", "busy_default"])
def test_stream_contract(harness, check, route):
    base = audiocodec_amd.AudioCodec(48000, N0)
    d, i = base.with_row_budget(2730).encode_packed_rows(_pcm(N0, 2, 4, 20, seed=77, inject=False))[:2]
    level, select = _calls(base, route)
    torch.cuda.synchronize()
    getattr(harness, check)("codec.packed_rows_level[1024-2,%s]" % route, ([d, i], level))
    if route == "fused":
        e, v = _dev(_sel_energy(4, 64, 256, 2, 9)), _dev(_checker(4, 64, 256, 2))
        st0 = torch.full((4, 64), 2.0, device="cuda")
        torch.cuda.synchronize()
        getattr(harness, check)("codec.select_loudest[4]", ([e, v, st0], select))


@gpu
@pytest.mark.parametrize("route", ["fused", "composition"])
def test_graph_capture(route):
    """One eager call (plans, allocator, the band table), then a linear capture on one stream, replayed on new contents."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    src = base.with_row_budget(2730)
    level, select = _calls(base, route)
    d, i = src.encode_packed_rows(_x(3, 5, 2, 5))[:2]
    e, v, st0 = _dev(_sel_energy(3, 3, 6, 2, 5)), _dev(_checker(3, 3, 6, 2)), torch.zeros((3, 3), device="cuda")
    level(d, i), select(e, v, st0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = level(d, i) + select(e, v, st0)
    for seed in (6, 7):
        d.copy_(src.encode_packed_rows(_x(3, 5, 2, seed))[0])
        e.copy_(_dev(_sel_energy(3, 3, 6, 2, seed)))
        st0.fill_(float(seed))
        g.replay()
        torch.cuda.synchronize()
        ref = level(d.clone(), i) + select(e.clone(), v, st0.clone())
        assert float(ref[0].max()) > 0 and bool(ref[2].any())
        for got, want in zip(out, ref):
            assert torch.equal(got, want), (seed, _where(got, want))


@gpu
def test_end_to_end_bridge_of_four():
    """Four sources -> levels -> select_loudest(n = 2) -> route_packed_rows(mix_minus_routes(4), active=): byte for byte the
    route under numpy's active, and no output hears more than two sources in a frame."""
    base = audiocodec_amd.AudioCodec(48000, N0)
    off = base.psy.scale_band_offsets
    dst = base.with_row_budget(1365)
    B, K, C, S = 3, 5, 2, 4
    sources = _sources(base, B, K, C, S, 90)
    levels = [base.packed_rows_level(d, i, True) for d, i in sources]
    energy = torch.stack([e for e, _ in levels])
    valid = torch.stack([bad == 0 for _, bad in levels])
    active = base.select_loudest([e for e, _ in levels], 2, valid, 0.5, 1e-6)
    np_levels = [lr.np_level(d.cpu().numpy(), i.cpu().numpy(), off, N0) for d, i in sources]
    want = lr.np_select(np.stack([e for e, _ in np_levels]), 2, np.stack([b == 0 for _, b in np_levels]), 0.5, 1e-6)
    assert torch.equal(energy.cpu(), torch.from_numpy(np.stack([e for e, _ in np_levels])))
    assert torch.equal(active.cpu(), torch.from_numpy(want[0]))
    heard = active.any(dim=3).sum(dim=0)
    assert int(heard.max()) == 2 and int((want[3] > F32(1e-6)).sum(axis=0).max()) > 2 and int((~valid).sum()) >= 1
    routes = base.mix_minus_routes(S)
    got = dst.route_packed_rows(sources, routes, active, True)
    ref = dst.route_packed_rows(sources, routes, _dev(want[0]), True)
    everyone = dst.route_packed_rows(sources, routes, None, True)
    for name, a, b in zip(("data", "index", "fits", "offset"), got, ref):
        assert torch.equal(a, b), (name, _where(a, b))
    assert not torch.equal(got[0], everyone[0])
    for o in range(S):                                                       # output o hears the active sources but o: at most two
        assert int(torch.stack([active[s] for s in range(S) if s != o]).any(dim=3).sum(dim=0).max()) <= 2
