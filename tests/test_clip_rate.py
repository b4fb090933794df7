"""Rate control per clip: one bit budget shared by the rows of a clip.

``clip_rate_reference.py`` restates rules 1-5 in numpy, with a scan of every offset and the bisection the kernels use; the
CPU tests pin the two to each other, to the worked example of the section and to the consequences the section lists; the
GPU tests check ``quantize_to_clip_budget`` against the restatement bit for bit and, at sizes numpy cannot reach, against
``quantize_to_budget``.
"""

import ctypes

import numpy as np
import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib
from clip_rate_reference import (ClipStats, floor_bits, padded, quantize_clip_budget, search_bisect, search_scan)
from rate_reference import K_MAX
from test_quantizer import np_offsets, np_quantize
from test_rate_control import EX_OFF, EX_THR, EX_X, adversarial, unlimited

# the C entry points of this feature: a library without them fails this whole file where it is collected
ENTRY_POINTS = {name: _lib.PROTOTYPES[name] for name in ("ac_quantize_clip_budget", "ac_clip_budget_scratch_bytes")}


def clip_unlimited(F, C, N, M):
    """A budget every clip meets at any offset: every row at its longest, padded."""
    return F * C * 32 * ((16 * N + 13 * M + 31) // 32)


def example():
    """The worked example of DESIGN.md section 8d: one clip of two frames and two channels on the bands of section 8c's
    example.  Rows in r order: the row of section 8c, the same a quarter as loud, its mirror image twice as loud, silence."""
    x0, t0 = EX_X.ravel(), EX_THR.ravel()
    X = np.zeros((1, 2, 8, 2), np.float32)
    X[0, 0, :, 0], X[0, 0, :, 1], X[0, 1, :, 0] = x0, x0 / 4, x0[::-1] * 2
    thr = np.broadcast_to(t0[None, None, :, None], X.shape).copy()
    return X, thr


def clips(rng, off, B, F, C):
    """B >= 4 clips of adversarial() rows: clip 0 holds the rows that saturate at every offset (it meets no tight budget),
    clip 1 the NaN / Inf bands and the scale factors at both clamp limits, the others ordinary rows at many levels."""
    assert B >= 4 and F >= 2
    return adversarial(rng, off, B, F, C)


def budgets(rng, st, kmin, M):
    """Per-clip budgets [B] that mix: clip 0 unmeetable (below what its saturated row takes at offset 254), clip 2 never
    binding, clip 3 exactly the floor, every other clip a share of its length at kmin, not a multiple of 32."""
    top, least = st.total(kmin), st.total(K_MAX)
    floor = floor_bits(st.F, st.C, M)
    T = np.maximum(floor + 40, (top * rng.uniform(0.3, 0.95, st.B)).astype(np.int64) | 5)
    T = np.maximum(np.minimum(T, top - 1), floor)
    T[0] = least[0] - 32 if kmin else -5          # (entries of a budget tensor are not checked)
    T[2] = top[2] + 1000
    T[3] = floor
    return T


# ---- CPU -----------------------------------------------------------------------------------------------------------
def test_worked_example():
    X, thr = example()
    st = ClipStats(X, thr, EX_OFF)
    np.testing.assert_array_equal(st.bits(0)[0], [100, 84, 115, 20])
    np.testing.assert_array_equal(padded(st.bits(0))[0], [128, 96, 128, 32])
    np.testing.assert_array_equal([st.total(k)[0] for k in (0, 2, 3, 8, 9, 11, 12, 17, 18, 20, 22, 26)],
                                  [384, 384, 352, 352, 320, 320, 288, 288, 256, 224, 192, 160])
    assert floor_bits(2, 2, 4) == 128
    # budget: (k_b, p_b, offsets, row bits, clip bits)
    table = {
        512: (0, 0, [0, 0, 0, 0], [100, 84, 115, 20], 384),           # never binding: quantize()
        384: (0, 0, [0, 0, 0, 0], [100, 84, 115, 20], 384),
        352: (3, 0, [3, 3, 3, 3], [94, 78, 110, 20], 352),            # d = [32, 0, 0, 0]: the first row's step does not fit
        340: (9, 2, [8, 8, 9, 9], [84, 68, 96, 20], 320),             # d = [0, 0, 32, 0], 20 bits left: two rows at k_b - 1
        300: (12, 1, [11, 12, 12, 12], [78, 62, 91, 20], 288),        # d = [0, 32, 0, 0], 12 bits left
        128: (52, 2, [51, 51, 52, 52], [20, 20, 20, 20], 128),        # the floor
        127: (K_MAX, 0, [K_MAX] * 4, [20, 20, 20, 20], 128),          # not met: clip_bits_out > T
    }
    for T, (kb, p, offs, bits, clip) in table.items():
        for search in (search_scan, search_bisect):
            codes, sf, offset, row_bits, clip_offset, clip_bits, more = quantize_clip_budget(X, thr, EX_OFF, T, 0, search)
            assert clip_offset[0] == kb and more["p"][0] == p and clip_bits[0] == clip, (T, search.__name__)
            np.testing.assert_array_equal(offset.ravel(), offs)
            np.testing.assert_array_equal(row_bits.ravel(), bits)
        if T == 512:
            codes0, sf0 = np_quantize(X, thr, EX_OFF)
            np.testing.assert_array_equal(codes, codes0)
            np.testing.assert_array_equal(sf, sf0)
        if T == 340:
            np.testing.assert_array_equal(more["d"][0], [0, 0, 32, 0])
            np.testing.assert_array_equal(sf[0, :, :, 0], [[0, -22, -14, -36], [0, -21, -13, -35]])
    # kmin bounds the search from below, and a clip at kmin is not filled
    _, _, offset, _, clip_offset, clip_bits, more = quantize_clip_budget(X, thr, EX_OFF, 512, 5)
    assert clip_offset[0] == 5 and more["p"][0] == 0 and clip_bits[0] == 352 and np.all(offset == 5)
    _, _, offset, _, clip_offset, _, _ = quantize_clip_budget(X, thr, EX_OFF, 360, -3)
    assert clip_offset[0] == 3 and np.all(offset == 3)


CPU_CASES = [(44100, 256, 48, -254), (48000, 64, 64, -40), (48000, 1024, 64, 0), (48000, 128, 64, 12)]


@pytest.mark.parametrize("sr,N,M,kmin", CPU_CASES)
def test_scan_equals_bisection_and_the_consequences_hold(sr, N, M, kmin):
    off = np_offsets(sr, N, M)
    rng = np.random.default_rng(N + M)
    B, F, C = 6, 3, 2
    X, thr = clips(rng, off, B, F, C)
    st = ClipStats(X, thr, off)
    T = budgets(rng, st, kmin, M)
    kb_scan, totals = search_scan(st, T, kmin)
    kb, evaluations = search_bisect(st, T, kmin)
    np.testing.assert_array_equal(kb, kb_scan)
    assert evaluations <= 9
    a = quantize_clip_budget(X, thr, off, T, kmin, search_scan, st)
    b = quantize_clip_budget(X, thr, off, T, kmin, search_bisect, st)
    for u, v in zip(a[:6], b[:6]):
        np.testing.assert_array_equal(u, v)
    codes, sf, offset, row_bits, clip_offset, clip_bits, more = b
    p, d, total = more["p"], more["d"], more["total"]
    # rule 1: the total does not grow with k
    assert np.all(np.diff(totals, axis=0) <= 0)
    # rule 2: k_b is minimal; clip 0 cannot meet its budget, clip 2 is not bound by it
    met = clip_bits <= T
    np.testing.assert_array_equal(met, totals[-1] <= T)
    assert not met[0] and clip_offset[0] == K_MAX and clip_offset[2] == kmin and met[1:].all()
    above = clip_offset > kmin
    assert np.all(totals[clip_offset[above] - kmin - 1, above.nonzero()[0]] > T[above])
    assert np.all(total[met] <= T[met])
    # rule 3: the fill runs where the budget is met above kmin; p_b is maximal and below F C; one row's step at most is
    # left unused
    ran = met & above
    assert ran.sum() >= 4 and np.all(p[~ran] == 0) and np.all(p < F * C)
    for c in ran.nonzero()[0]:
        prefix = np.cumsum(d[c])
        left = T[c] - total[c]
        assert (p[c] == 0 or prefix[p[c] - 1] <= left) and prefix[p[c]] > left
        assert clip_bits[c] == total[c] + (prefix[p[c] - 1] if p[c] else 0)
        assert 0 <= T[c] - clip_bits[c] < d[c, p[c]]
    # rule 4: k_b - 1 on a prefix, k_b after it
    flat = offset.reshape(B, -1).astype(np.int64)
    for c in range(B):
        np.testing.assert_array_equal(flat[c], [clip_offset[c] - 1] * p[c] + [clip_offset[c]] * (F * C - p[c]))
    # rule 5: the clip's bits are those of its padded rows
    np.testing.assert_array_equal(clip_bits, padded(row_bits).reshape(B, -1).sum(axis=1))


@pytest.mark.parametrize("sr,N,M", [(44100, 256, 48), (48000, 1024, 64)])
def test_unlimited_budget_is_quantize(sr, N, M):
    off = np_offsets(sr, N, M)
    rng = np.random.default_rng(5)
    B, F, C = 4, 2, 2
    X, thr = clips(rng, off, B, F, C)
    codes0, sf0 = np_quantize(X, thr, off)
    assert clip_unlimited(F, C, N, M) == F * C * 32 * -(-(16 * N + 13 * M) // 32)
    codes, sf, offset, _, clip_offset, clip_bits, _ = quantize_clip_budget(X, thr, off, clip_unlimited(F, C, N, M), 0)
    np.testing.assert_array_equal(codes, codes0)
    np.testing.assert_array_equal(sf, sf0)
    assert not offset.any() and not clip_offset.any() and np.all(clip_bits <= clip_unlimited(F, C, N, M))


def test_a_larger_budget_never_raises_an_offset():
    off = np_offsets(48000, 256, 64)
    rng = np.random.default_rng(9)
    X, thr = clips(rng, off, 5, 4, 2)
    st = ClipStats(X, thr, off)
    for kmin in (-20, 0):
        lo, hi = floor_bits(4, 2, 64), int(st.total(kmin)[1:].max())
        last = None
        for T in np.unique(np.linspace(lo, hi + 64, 40).astype(np.int64)):
            offset = quantize_clip_budget(X, thr, off, int(T), kmin, st=st)[2]
            if last is not None:
                assert np.all(offset <= last), T
            last = offset
        assert np.all(last[1:] == kmin)


def test_library_exports_the_clip_budget_entry_points():
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)
    assert lib.ac_version() == 171
    args = [None, None, None, 10 ** 9, None, 0] + [None] * 7 + [1, 1, 1, None]
    assert lib.ac_quantize_clip_budget(*args) == _lib.AC_EINVAL
    assert "plan" in lib.ac_last_error().decode()
    assert callable(audiocodec_amd.PsychoacousticModel.quantize_to_clip_budget)
    for name in ("clip_bits_for_bitrate", "encode_quantized_clip_budget", "encode_packed_clip_budget"):
        assert callable(getattr(audiocodec_amd.AudioCodec, name))
    codec = audiocodec_amd.AudioCodec(48000, 1024)
    assert codec.row_bits_for_bitrate(64000) == 1365
    assert codec.clip_bits_for_bitrate(64000, 469, 2) == 469 * 2 * 1344         # 32 floor(1365 / 32)
    assert codec.clip_bits_for_bitrate(128000, 10, 1) == 10 * 2720
    assert codec.clip_bits_for_bitrate(64000, 0, 2) == 0
    with pytest.raises(ValueError):
        codec.clip_bits_for_bitrate(0, 10, 2)
    with pytest.raises(ValueError):
        codec.clip_bits_for_bitrate(64000, -1, 2)
    with pytest.raises(TypeError):
        codec.clip_bits_for_bitrate(64000, 10.0, 2)


def scratch_bytes(M, B, F, C):
    """12 M bytes of statistics per row, 8 of row bits, the totals of nine bisection steps per clip and two sums per split
    of a clip, each part rounded up to 256 bytes.  A clip is cut into splits of at least 16 rows, at most 256 of them, as
    many as bring the launch to 2048 workgroups."""
    def up(v):
        return (v + 255) // 256 * 256
    R = F * C
    rows_per_split = max(16, -(-R // min(256, -(-2048 // B))))
    return up(12 * M * B * R) + up(8 * 9 * B) + up(16 * B * -(-R // rows_per_split)) + up(8 * B * R)


def test_scratch_bytes_helper_and_no_plan():
    """The helper the GPU test holds the library to, on sizes worked out by hand; without a plan (a plan lives on a device, so
    the library's own arithmetic is checked in the GPU test_scratch_bytes) the entry point answers 0."""
    assert scratch_bytes(64, 1, 1, 1) == 768 + 256 + 256 + 256
    assert scratch_bytes(64, 256, 469, 2) == 12 * 64 * 256 * 938 + 72 * 256 + 16 * 256 * 8 + 8 * 256 * 938
    assert scratch_bytes(64, 1, 30000, 2) >= 12 * 64 * 60000 + 16 * 256
    assert _lib.load().ac_clip_budget_scratch_bytes(None, 4, 4, 2) == 0           # (a plan lives on a device: GPU test below)


# ---- GPU -----------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(psy, Xd, td, st, T, kmin):
    """quantize_to_clip_budget against the numpy restatement, bit for bit; returns the reference."""
    off = psy.scale_band_offsets
    Td = _dev(np.asarray(T, dtype=np.int64)) if isinstance(T, np.ndarray) else T
    codes, sf, offset, row_bits, clip_bits = psy.quantize_to_clip_budget(Xd, td, Td, min_offset=kmin)
    ref = quantize_clip_budget(st.X, None, off, T, kmin, st=st)
    B, F, C = st.B, st.F, st.C
    assert codes.dtype == torch.int16 and sf.dtype == torch.int8 and offset.dtype == torch.int16
    assert row_bits.dtype == torch.int32 and clip_bits.dtype == torch.int64
    assert offset.shape == (B, F, C) and row_bits.shape == (B, F, C) and clip_bits.shape == (B,)
    np.testing.assert_array_equal(offset.cpu().numpy(), ref[2])
    np.testing.assert_array_equal(row_bits.cpu().numpy(), ref[3])
    np.testing.assert_array_equal(clip_bits.cpu().numpy(), ref[5])
    np.testing.assert_array_equal(sf.cpu().numpy(), ref[1])
    np.testing.assert_array_equal(codes.cpu().numpy(), ref[0])
    return ref


def _filled_share(ref, T, kmin):
    """The share of clips whose budget the reference meets above kmin: the clips whose fill step runs."""
    return float(np.mean((ref[4] > kmin) & (ref[5] <= np.broadcast_to(T, ref[5].shape))))


@gpu
def test_scratch_bytes():
    lib = _lib.load()
    for sr, N, M in ((48000, 1024, 64), (44100, 256, 48)):
        psy = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M)      # (owns the plan: keep it alive)
        plan = psy._plan(torch.device("cuda", 0))
        for B, F, C in [(1, 1, 1), (256, 469, 2), (1, 30000, 2), (3000, 1, 2), (7, 33, 6)]:
            assert lib.ac_clip_budget_scratch_bytes(plan, B, F, C) == scratch_bytes(M, B, F, C), (M, B, F, C)
        assert lib.ac_clip_budget_scratch_bytes(plan, 0, 4, 2) == 0
        assert lib.ac_clip_budget_scratch_bytes(plan, 4, -1, 2) == 0


@gpu
@pytest.mark.parametrize("sr,N,M,C", [(48000, 1024, 64, 2), (48000, 1024, 64, 1), (48000, 960, 64, 6), (48000, 2048, 64, 1),
                                      (48000, 64, 64, 2), (44100, 256, 48, 2),
                                      # more than one channel group: groups of 4 and 3 channels; one channel each
                                      # although C = 2
                                      (48000, 1024, 600, 7), (48000, 256, 1400, 2)])
def test_quantize_to_clip_budget_bit_exact(sr, N, M, C):
    """Per-clip budget tensors that mix never-binding, binding, exactly-the-floor and unmeetable budgets, on clips with
    NaN / Inf bands and saturated rows, from min_offset below, at and above 0; then a scalar budget.  At least three
    quarters of the clips of every run take the fill step (asserted on the reference)."""
    psy = audiocodec_amd.PsychoacousticModel(sr, filter_bands_n=N, bark_bands_n=M)
    off = psy.scale_band_offsets
    rng = np.random.default_rng(N * 7 + M + C)
    B, F = 12, 9
    X, thr = clips(rng, off, B, F, C)
    st = ClipStats(X, thr, off)
    Xd, td = _dev(X), _dev(thr)
    seen, filled = set(), 0
    for kmin in (-30, 0, 17):
        T = budgets(rng, st, kmin, M)
        ref = _check(psy, Xd, td, st, T, kmin)
        assert _filled_share(ref, T, kmin) >= 0.75
        assert ref[5][0] > T[0] and ref[4][0] == K_MAX and ref[4][2] == kmin and ref[5][3] == T[3] == floor_bits(F, C, M)
        seen.update(np.unique(ref[2]).tolist())
        filled += int((ref[6]["p"] > 0).sum())
    assert K_MAX in seen and len(seen) > 8 and filled >= 12
    assert (st.sf0 == -128).any()
    # a scalar budget: the median clip's length at offset 0 halved (clip 0 cannot meet it)
    scalar = int(max(floor_bits(F, C, M), np.median(st.total(0)) // 2))
    ref = _check(psy, Xd, td, st, scalar, 0)
    assert _filled_share(ref, scalar, 0) >= 0.75


@gpu
@pytest.mark.parametrize("B,F,C,N", [(1, 300, 2, 1024), (1, 4500, 2, 64), (300, 1, 2, 1024), (2100, 1, 1, 64)])
def test_one_long_clip_and_many_one_frame_clips_bit_exact(B, F, C, N):
    """B = 1: the clip's rows are cut into 38 (600 rows) and 250 (9000 rows) splits, one workgroup each, and the search and
    the scan run across them; F = 1: a clip is one or two rows, and more clips than the launch has workgroups to split."""
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=N, bark_bands_n=64)
    off = psy.scale_band_offsets
    rng = np.random.default_rng(B + F + N)
    X = (rng.standard_normal((B, F, N, C)) * 10.0 ** rng.uniform(-4, 0, (B, F, 1, C))).astype(np.float32)
    thr = (np.abs(rng.standard_normal((B, F, N, C))) * 10.0 ** rng.uniform(-5, -2, (B, F, 1, C)) + 1e-8).astype(np.float32)
    st = ClipStats(X, thr, off)
    Xd, td = _dev(X), _dev(thr)
    for kmin in (0, -12):
        top = st.total(kmin)
        T = np.minimum(np.maximum(floor_bits(F, C, 64) + 40, (top * rng.uniform(0.3, 0.95, B)).astype(np.int64) | 3), top - 1)
        if B > 1:
            T[B // 2] = top[B // 2] + 64                       # never binding
            T[B - 1] = floor_bits(F, C, 64) - 1                 # unmeetable
        ref = _check(psy, Xd, td, st, T, kmin)
        assert _filled_share(ref, T, kmin) >= 0.75
        if B == 1:
            assert 0 < ref[6]["p"][0] < F * C
        else:
            assert ref[4][B - 1] == K_MAX and ref[4][B // 2] == kmin


def _against_the_row_kernel(psy, X, thr, T, kmin):
    """quantize_to_clip_budget against quantize_to_budget (section 8c), at sizes numpy is too slow for.  T int64 [B] on
    the device.  Returns (offset, clip_bits_out, the clips whose fill ran)."""
    B, F, N, C = X.shape
    M = psy.bark_bands_n
    R = F * C
    codes, sf, offset, row_bits, clip_bits = psy.quantize_to_clip_budget(X, thr, T, min_offset=kmin)
    flat = offset.reshape(B, R).long()
    kb = flat[:, -1]                                                # p_b < F C: the last row is at k_b
    # rule 4: k_b - 1 on a prefix, k_b after it
    assert bool(((flat == kb[:, None]) | (flat == kb[:, None] - 1)).all())
    assert bool((flat[:, 1:] >= flat[:, :-1]).all())
    p = (flat < kb[:, None]).sum(dim=1)
    assert int(kb.min()) >= kmin and int(kb.max()) <= K_MAX

    def pad(bits):
        return (bits.long() + 31) // 32 * 32

    # every row equals the row kernel's at the row's offset; the row kernel's bits at every k_b and k_b - 1
    bits_at = {}
    need = set(torch.unique(flat).tolist()) | set((torch.unique(kb[kb > kmin]) - 1).tolist())
    for v in sorted(need):
        rc, rs, ro, rb = psy.quantize_to_budget(X, thr, unlimited(N, M), min_offset=int(v))
        assert bool((ro == v).all())
        bits_at[v] = rb.reshape(B, R)
        rows = offset == v
        if bool(rows.any()):
            assert torch.equal(row_bits[rows], rb[rows]), v
            assert torch.equal(sf.transpose(2, 3)[rows], rs.transpose(2, 3)[rows]), v
            assert torch.equal(codes.transpose(2, 3)[rows], rc.transpose(2, 3)[rows]), v
    at = torch.stack([pad(bits_at[int(k)][b]) for b, k in enumerate(kb.tolist())])
    under = torch.stack([pad(bits_at[int(k) - 1][b]) if k > kmin else at[b] for b, k in enumerate(kb.tolist())])
    total, d = at.sum(dim=1), under - at
    met = total <= T
    ran = met & (kb > kmin)
    # rule 2: k_b is minimal
    assert bool((kb[~met] == K_MAX).all())
    assert bool((under.sum(dim=1)[kb > kmin] > T[kb > kmin]).all())
    # rule 3: p_b is maximal; at most one row's step is left unused
    assert bool((p[~ran] == 0).all()) and bool((p < R).all())
    prefix = torch.cat([torch.zeros_like(total)[:, None], d.cumsum(dim=1)], dim=1)       # [B, R + 1], exclusive
    used = prefix.gather(1, p[:, None])[:, 0]
    np.testing.assert_array_equal(clip_bits.cpu().numpy(), (total + used).cpu().numpy())
    assert bool((clip_bits[met] <= T[met]).all())
    slack = (T - clip_bits)[ran]
    assert bool((slack >= 0).all()) and bool((slack < d.gather(1, p[:, None])[:, 0][ran]).all())
    np.testing.assert_array_equal(clip_bits.cpu().numpy(), pad(row_bits).reshape(B, R).sum(dim=1).cpu().numpy())
    return offset, clip_bits, ran


@gpu
def test_chip_filling_launch_against_the_row_kernel():
    """B = 256 stereo clips of 3 s at N = 1024: 36 096 row workgroups, and 256 x 8 = 2048 workgroups in the clip search, the
    fill and the scan.  Three clips in four get a share of their own length at offset 0 (binding by construction), the
    others 24 ... 160 kbit/s per channel; a few budgets never bind, sit at the floor or below it."""
    from chip_scale_inputs import MIN_WORKGROUPS, structured
    N, C, B, K = 1024, 2, 256, 140
    F = K + 1
    codec = audiocodec_amd.AudioCodec(48000, N)
    M = codec.psy.bark_bands_n
    rps = max(16, -(-F * C // min(256, -(-2048 // B))))
    assert B * -(-F * C // rps) >= MIN_WORKGROUPS and B * F >= MIN_WORKGROUPS
    X, _, thr = codec.encode(structured(B, K, N, C, seed=31))
    rng = np.random.default_rng(31)
    T = np.array([codec.clip_bits_for_bitrate(float(r), F, C) for r in rng.uniform(24000, 160000, B)], dtype=np.int64)
    natural = codec.psy.quantize_to_budget(X, thr, unlimited(N, M))[3]
    top = ((natural.long() + 31) // 32 * 32).reshape(B, -1).sum(dim=1).cpu().numpy()
    share = np.maximum(floor_bits(F, C, M), (top * rng.uniform(0.3, 0.95, B)).astype(np.int64))
    T = np.where(np.arange(B) % 4 == 3, T, share) + rng.integers(0, 32, B)       # (not multiples of 32)
    T[5::40] = clip_unlimited(F, C, N, M)
    T[7::50] = floor_bits(F, C, M)
    T[9::60] = floor_bits(F, C, M) - 1
    offset, clip_bits, ran = _against_the_row_kernel(codec.psy, X, thr, _dev(T), 0)
    assert float(ran.double().mean()) >= 0.5 and len(torch.unique(offset)) > 8
    assert bool((offset.reshape(B, -1)[9::60] == K_MAX).all())


@gpu
def test_splits_longer_than_a_workgroup_against_the_row_kernel():
    """More clips than workgroups to spare: every clip is one split of 400 rows, scanned by its workgroup of 256 threads
    in two rounds with a carry."""
    N, C, B, F = 64, 2, 2100, 200
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=N, bark_bands_n=64)
    g = torch.Generator(device="cuda").manual_seed(4)
    gain = 10.0 ** (-3.0 * torch.rand((B, F, 1, C), device="cuda", generator=g))
    X = torch.randn((B, F, N, C), device="cuda", generator=g) * gain
    thr = torch.rand((B, F, N, C), device="cuda", generator=g) * 0.01 * gain + 1e-7
    natural = psy.quantize_to_budget(X, thr, unlimited(N, 64))[3]
    top = ((natural.long() + 31) // 32 * 32).reshape(B, -1).sum(dim=1)
    share = 0.4 + 0.59 * torch.rand((B,), device="cuda", generator=g).double()
    T = torch.maximum((top.double() * share).long() | 1, torch.full_like(top, floor_bits(F, C, 64)))
    offset, _, ran = _against_the_row_kernel(psy, X, thr, T, 0)
    assert float(ran.double().mean()) >= 0.75
    # the prefix ends in the second round of the scan in some clips and in the first in others
    p = (offset.reshape(B, -1) < offset.reshape(B, -1)[:, -1:]).sum(dim=1)
    assert bool((p > 256).any()) and bool(((p > 0) & (p < 256)).any())


@gpu
@pytest.mark.parametrize("N,C,bps", [(1024, 2, 64000), (1024, 1, 32000), (2048, 2, 128000), (960, 6, 48000)])
def test_encode_packed_clip_budget_at_a_bitrate(N, C, bps):
    """End to end: each clip's bytes in data are clip_bits_out / 8 and at most T / 8; the stream decodes to decode_quantized
    of the budgeted codes, bit for bit."""
    codec = audiocodec_amd.AudioCodec(48000, N)
    rng = np.random.default_rng(N + C)
    B, K = 3, 11
    x = (rng.uniform(-1, 1, (B, K * N, C)) * np.linspace(0.01, 1, K * N)[None, :, None]).astype(np.float32)
    x[1] *= 0.05
    xd = _dev(x)
    T = codec.clip_bits_for_bitrate(bps, K + 1, C)
    assert T == (K + 1) * C * 32 * ((bps * N // 48000) // 32)
    data, index, offset = codec.encode_packed_clip_budget(xd, T)
    codes, sf, offset2, row_bits, clip_bits = codec.encode_quantized_clip_budget(xd, T)
    assert torch.equal(offset, offset2)
    starts = index[:, 0, 0].cpu().numpy()
    clip_bytes = np.diff(np.concatenate([starts, [data.numel()]]))
    np.testing.assert_array_equal(clip_bytes * 8, clip_bits.cpu().numpy())
    assert np.all(clip_bytes * 8 <= T) and T % 8 == 0
    # a clip the budget binds leaves less than one row's step, which no row's longest padded length exceeds
    bound = offset.reshape(B, -1)[:, -1].cpu().numpy() > 0
    assert bound.any() and np.all(T - clip_bytes[bound] * 8 < 32 * ((16 * N + 13 * 64 + 31) // 32))
    for pcm16 in (False, True) if C <= 2 else (False,):
        a = codec.decode_packed(data, index, pcm16=pcm16)
        b = codec.decode_quantized(codes, sf, pcm16=pcm16)
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.int32) if not pcm16 else a, b.view(torch.int32) if not pcm16 else b)


@gpu
def test_side_stream():
    codec = audiocodec_amd.AudioCodec(48000, 1024)
    rng = np.random.default_rng(8)
    x = _dev(rng.uniform(-1, 1, (4, 20 * 1024, 2)).astype(np.float32))
    X, _, thr = codec.encode(x)
    T = codec.clip_bits_for_bitrate(48000, 21, 2)
    ref = codec.psy.quantize_to_clip_budget(X, thr, T)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = codec.psy.quantize_to_clip_budget(X, thr, T)
    torch.cuda.current_stream().wait_stream(s)
    for a, b in zip(out, ref):
        assert torch.equal(a, b)
    assert int(ref[2].max()) > 0


@gpu
def test_error_paths():
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=1024, bark_bands_n=64)
    rng = np.random.default_rng(1)
    X, thr = adversarial(rng, psy.scale_band_offsets, 2, 2, 2)
    Xd, td = _dev(X), _dev(thr)
    floor = floor_bits(2, 2, 64)
    assert floor == 4 * 320
    T = torch.full((2,), 9000, dtype=torch.int64, device=Xd.device)
    with pytest.raises(ValueError):
        psy.quantize_to_clip_budget(Xd.double(), td.double(), 9000)
    with pytest.raises(ValueError):
        psy.quantize_to_clip_budget(Xd, td[:, :1], 9000)
    with pytest.raises(ValueError):
        psy.quantize_to_clip_budget(Xd, td, T.int())
    with pytest.raises(ValueError):
        psy.quantize_to_clip_budget(Xd, td, T[:1])
    with pytest.raises(ValueError):
        psy.quantize_to_clip_budget(Xd, td, T.cpu())
    with pytest.raises(ValueError):
        psy.quantize_to_clip_budget(Xd, td, floor - 1)
    with pytest.raises(ValueError):
        psy.quantize_to_clip_budget(Xd, td, 9000, min_offset=255)
    with pytest.raises(ValueError):
        psy.quantize_to_clip_budget(Xd, td, 9000, min_offset=-255)
    with pytest.raises(TypeError):
        psy.quantize_to_clip_budget(Xd, td, 9000.0)
    with pytest.raises(TypeError):
        psy.quantize_to_clip_budget(Xd, td, 9000, min_offset=1.0)
    with pytest.raises(ValueError, match="add_noise"):
        psy.quantize_to_clip_budget(Xd.clone().requires_grad_(), td, 9000)
    codec = audiocodec_amd.AudioCodec(48000, 1024)
    with pytest.raises(ValueError, match="add_noise"):
        codec.encode_quantized_clip_budget(_dev(np.zeros((1, 2048, 2), np.float32)).requires_grad_(), 9000)
    other = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=1024, bark_bands_n=64, compute_dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="float32"):
        other.quantize_to_clip_budget(Xd.double(), td.double(), 9000)
    assert psy.quantize_to_clip_budget(Xd, td, floor)[4].shape == (2,)           # the floor itself is accepted
    # the C ABI refuses what the Python layer refuses, with a message
    lib = _lib.load()
    plan = psy._plan(Xd.device)
    out = [torch.empty(s, dtype=d, device=Xd.device)
           for s, d in (((2, 2, 1024, 2), torch.int16), ((2, 2, 64, 2), torch.int8), ((2, 2, 2), torch.int16),
                        ((2, 2, 2), torch.int32), ((2,), torch.int16), ((2,), torch.int64))]
    scratch = torch.empty((lib.ac_clip_budget_scratch_bytes(plan, 2, 2, 2),), dtype=torch.uint8, device=Xd.device)
    p = [ctypes.c_void_p(t.data_ptr()) for t in [Xd, td] + out + [scratch]]

    def call(T, Tclip, kmin, optional=(5, 6, 7), scr=p[8]):
        o = [p[i] if i in optional else None for i in (5, 6, 7)]
        return lib.ac_quantize_clip_budget(plan, p[0], p[1], T, Tclip, kmin, p[2], p[3], p[4], o[0], o[1], o[2], scr, 2, 2, 2,
                                           None)

    assert call(9000, None, 255) == _lib.AC_EINVAL and "kmin" in lib.ac_last_error().decode()
    assert call(9000, None, -255) == _lib.AC_EINVAL
    assert call(floor - 1, None, 0) == _lib.AC_EINVAL and "clip_bits" in lib.ac_last_error().decode()
    assert call(9000, None, 0, scr=None) == _lib.AC_EINVAL and "scratch" in lib.ac_last_error().decode()
    assert lib.ac_quantize_clip_budget(plan, p[0], p[1], 9000, None, 0, p[2], p[3], None, None, None, None, p[8], 2, 2, 2,
                                       None) == _lib.AC_EINVAL and "NULL" in lib.ac_last_error().decode()
    assert call(0, ctypes.c_void_p(T.data_ptr()), 0) == _lib.AC_OK        # per-clip budgets: the scalar is not read
    torch.cuda.synchronize()
    ref = psy.quantize_to_clip_budget(Xd, td, T)
    for got, want in zip(out[:4] + out[5:], ref):
        assert torch.equal(got, want)
    assert torch.equal(out[4].long(), ref[2].reshape(2, -1)[:, -1].long())    # clip_offset = k_b, the last row's offset
    # row_bits_out, clip_offset and clip_bits_out may be NULL
    for t in out:
        t.zero_()
    assert call(9000, None, 0, optional=()) == _lib.AC_OK
    torch.cuda.synchronize()
    ref = psy.quantize_to_clip_budget(Xd, td, 9000)
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]) and torch.equal(out[2], ref[2])
    assert not out[3].any() and not out[4].any() and not out[5].any()
