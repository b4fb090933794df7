"""GPU (MI355X): every kernel tier at a launch that fills the chip, held frame by frame to an independent result.

The parity tests elsewhere run grids of a few dozen workgroups; the kernels earn their keep at thousands of workgroups,
several resident per CU, many rounds of waves -- the shape at which round 4's first run-structured masking model returned
wrong values in 0.5 - 2 % of the frames while passing every small test.  Each case here launches at least 2048 workgroups
(8 per CU; the grid is stated in the case id) on at least 96 clips of 144 000 samples of structured input
(chip_scale_inputs.structured) and compares frame by frame:

  * float32 / 2-byte filter bank and masking model against the float64 kernels (k_*_generic<double>: plain O(N^2) code that
    shares no device function with the wave-level, LDS-FFT, team or run-structured kernels) on the same input cast up; the
    float64 result itself against the CPU oracle on the first and the last clip (1e-12 class bars);
  * the quantiser family bit for bit against the numpy restatements (test_quantizer, pack_reference, rate_reference).

A failure names the worst (clip, frame, channel) and how many frames exceed the bar.  test_chip_scale_table.py (CPU) holds
the case table to the paths it must cover.
"""

import math

import numpy as np
import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _lib
from chip_scale_inputs import (MIN_WORKGROUPS, abs_ratio, blocks, blocks_per_clip, clip_l2_ratio, clips_for,
                               frame_peak_ratio, rel_elem_ratio, structured, tonality_ratio, worst)
from emulate_runs import granule_registers, runs_image
from oracle.audiocodec_oracle import MDCTOracle, PsychoOracle

pytestmark = pytest.mark.gpu

TOL = 1e-4                      # coefficients, thresholds (test_gpu_parity.TOL)
LSB = 1.0 / 32768.0             # PCM
SPREAD_TOL = {"f32": TOL, "bf16x2_mfma": TOL, "bf16_mfma": 5e-3}   # (test_gpu_parity.SPREAD_TOL)
PCM16_SIZES = (1024, 2048, 960, 1920, 480)
F64_FWD_MAX, F64_INV_MAX = 8192, 4096


def _tpw(N):
    """(frame, channel pair) tasks one workgroup takes at most, for sizing B: a frame per workgroup above 1024 (two / four /
    eight waves on one frame), several frames per wave below -- 8192 / N, at most 32."""
    return max(1, min(32, 8192 // N))


# Clips per case beyond clips_for's estimate, measured (a kernel trace of this module's first run: 2048 / the fewest
# workgroups any kernel under test launched there, + 2 %): the wave-level kernels take 16 frames per workgroup, the
# inverse and team kernels of the LDS-FFT tier several, so the base clip count left some launches below 2048 workgroups.
# Keyed by (first path, N, C); 2-byte cases by "<dtype>:<path>".
GRID_SCALE = {
    ('tier3', 1024, 2): 2.02,
    ('tier3', 1024, 1): 2.02,
    ('tier3', 2048, 2): 4.02,
    ('tier3', 2048, 1): 4.02,
    ('tier2', 480, 2): 1.43,
    ('tier2', 960, 2): 1.5,
    ('tier2', 4096, 2): 1.41,
    ('tier2', 8192, 1): 9.16,
    ('tier2_frame_offsets', 1152, 2): 2.29,
    ('tier2', 3600, 2): 1.49,
    ('tier2', 7680, 1): 2.76,
    ('tier1', 250, 2): 1.52,
    ('tier1', 810, 1): 1.57,
    ('team', 960, 6): 4.35,
    ('team', 1024, 3): 9.67,
    ('strided_pairs', 1024, 3): 1.36,
    ('tier2_f32', 1024, 2): 2.02,
    ('tier2_bf16_mfma', 1024, 2): 2.02,
    ('tier2_bf16x2_mfma', 1024, 1): 2.02,
    ('tier2_bf16x2_mfma', 2048, 2): 4.02,
    ('tier2_f32', 2048, 1): 4.02,
    ('runs_R1', 128, 2): 2.47,
    ('runs_R2', 256, 1): 2.02,
    ('runs_R4', 512, 2): 2.02,
    ('runs_R16', 2048, 2): 4.02,
    ('runs_R32', 4096, 1): 1.53,
    ('runs_team', 960, 6): 1.15,
    ('runs_team', 2048, 3): 1.23,
    ('band_walk', 1024, 2): 2.02,
    ('tier0', 1024, 2): 2.46,
    ('fused_wave', 64, 2): 2.47,
    ('fused_wave', 128, 1): 4.02,
    ('fused_wave', 256, 2): 3.96,
    ('fused_wave', 512, 1): 3.96,
    ('fused_wave', 512, 2): 3.96,
    ('fused_wave', 1024, 1): 2.02,
    ('fused_wave', 1024, 2): 2.02,
    ('wave_two_launch', 2048, 1): 4.02,
    ('fused_wave', 2048, 2): 4.02,
    ('fused_lds', 960, 2): 1.5,
    ('multichannel', 1024, 3): 9.67,
    ('duplex', 1024, 2): 1.36,
    ('lds_chain', 960, 2): 5.44,
    ('one_launch', 1024, 2): 1.23,
    ('two_launches', 960, 2): 4.58,
    ('f16:lds', 960, 2): 1.52,
    ('f16:wave', 1024, 2): 2.03,
    ('f16:lds', 4096, 1): 1.83,
    ('bf16:wave', 1024, 2): 2.02,
    ('bf16:wave', 1024, 1): 2.02,
    ('bf16:wave', 2048, 2): 4.02,
    ('bf16:lds', 960, 2): 2.03,
}


def _case(area, covers, **kw):
    """One row of the case table.  ``covers``: the (entry point, path) pairs it exercises; the id names the path and the
    launch (clips x blocks; the grid it gives is >= MIN_WORKGROUPS workgroups by construction, see clips_for)."""
    N, C = kw["N"], kw["C"]
    K = blocks_per_clip(N)
    B = kw.pop("B", None) or clips_for(N, C, kw.pop("tpw", _tpw(N)))
    key = (("%s:" % kw["tag"]) if kw.get("dtype") else "") + covers[0][1]
    B = int(math.ceil(B * GRID_SCALE.get((key, N, C), 1.0)))
    kw.update(area=area, covers=tuple(covers), K=K, B=B)
    tag = kw.get("tag", "")
    kw["id"] = "%s-N%d-C%d-B%dxK%d%s" % (covers[0][1], N, C, B, kw.get("K_stream", K), ("-" + tag) if tag else "")
    return kw


FB, PSY, ENC, TWO, STREAM, QUANT, RATE, DECQ = ("filter_bank", "masking", "encode", "two_byte", "stream", "quantiser",
                                                "rate", "decode_quantized")
FWD, INV = "mdct.transform", "mdct.inverse_transform"
TON, THR = "psy.tonality", "psy.global_masking_threshold"

CASES = [
    # ---- filter bank, float32 ----------------------------------------------------------------------------------------
    _case(FB, [(FWD, "tier3"), (INV, "tier3")], N=1024, C=2, tier=3),
    _case(FB, [(FWD, "tier3"), (INV, "tier3")], N=1024, C=1, tier=3),
    _case(FB, [(FWD, "tier3"), (INV, "tier3")], N=2048, C=2, tier=3),
    _case(FB, [(FWD, "tier3"), (INV, "tier3")], N=2048, C=1, tier=3),
    _case(FB, [(FWD, "tier2"), (INV, "tier2")], N=480, C=2, tier=2),
    _case(FB, [(FWD, "tier2"), (INV, "tier2")], N=960, C=2, tier=2),
    _case(FB, [(FWD, "tier2"), (INV, "tier2")], N=1920, C=1, tier=2),
    _case(FB, [(FWD, "tier2"), (INV, "tier2")], N=4096, C=2, tier=2),
    _case(FB, [(FWD, "tier2"), (INV, "tier2_vs_oracle")], N=8192, C=1, tier=2),
    _case(FB, [(FWD, "tier2_frame_offsets"), (INV, "tier2")], N=1152, C=2, tier=2),
    _case(FB, [(FWD, "tier2_frame_offsets"), (INV, "tier2_frame_offsets")], N=2304, C=1, tier=2),
    _case(FB, [(FWD, "tier2"), (INV, "tier2")], N=3600, C=2, tier=2),
    _case(FB, [(FWD, "tier2"), (INV, "tier2_frame_offsets_vs_oracle")], N=7680, C=1, tier=2),
    _case(FB, [(FWD, "tier1"), (INV, "tier1")], N=250, C=2, tier=1),
    _case(FB, [(FWD, "tier1"), (INV, "tier1")], N=810, C=1, tier=1),
    _case(FB, [(FWD, "tier0"), (INV, "tier0")], N=1022, C=2, tier=0, tpw=1),
    _case(FB, [(FWD, "team"), (INV, "team")], N=960, C=6, tier=2, noteam="2", tag="NOTEAM2"),
    _case(FB, [(FWD, "team"), (INV, "team")], N=1024, C=3, tier=2, noteam="2", tag="NOTEAM2"),
    _case(FB, [(FWD, "strided_pairs"), (INV, "strided_pairs")], N=512, C=5, tier=2, noteam="1", tag="NOTEAM1"),
    _case(FB, [(FWD, "strided_pairs"), (INV, "strided_pairs")], N=1024, C=3, tier=2, noteam="1", tag="NOTEAM1"),
    # ---- masking model ------------------------------------------------------------------------------------------------
    _case(PSY, [(TON, "tier2_f32"), (THR, "tier2_f32")], N=1024, C=2, psy_tier=2, spreading="f32"),
    _case(PSY, [(TON, "tier2_bf16_mfma"), (THR, "tier2_bf16_mfma")], N=1024, C=2, psy_tier=2, spreading="bf16_mfma"),
    _case(PSY, [(TON, "tier2_bf16x2_mfma"), (THR, "tier2_bf16x2_mfma")], N=1024, C=1, psy_tier=2, spreading="bf16x2_mfma",
          drown=0.3, tag="drown"),
    _case(PSY, [(TON, "tier2_bf16x2_mfma"), (THR, "tier2_bf16x2_mfma")], N=2048, C=2, psy_tier=2, spreading="bf16x2_mfma"),
    _case(PSY, [(TON, "tier2_f32"), (THR, "tier2_f32")], N=2048, C=1, psy_tier=2, spreading="f32"),
    _case(PSY, [(TON, "runs_R1"), (THR, "runs_R1")], N=128, C=2, psy_tier=1, R=1),
    _case(PSY, [(TON, "runs_R2"), (THR, "runs_R2")], N=256, C=1, psy_tier=1, R=2),
    _case(PSY, [(TON, "runs_R4"), (THR, "runs_R4")], N=512, C=2, psy_tier=1, R=4, drown=0.3, tag="drown"),
    _case(PSY, [(TON, "runs_R8"), (THR, "runs_R8")], N=960, C=2, psy_tier=1, R=8),
    _case(PSY, [(TON, "runs_R16"), (THR, "runs_R16")], N=2048, C=2, M=48, psy_tier=1, R=16, tag="M48"),
    _case(PSY, [(TON, "runs_R32"), (THR, "runs_R32")], N=4096, C=1, psy_tier=1, R=32),
    _case(PSY, [(TON, "runs_team"), (THR, "runs_team")], N=960, C=6, psy_tier=1, R=8),
    _case(PSY, [(TON, "runs_team"), (THR, "runs_team")], N=640, C=8, psy_tier=1, R=8, drown=0.2, tag="drown"),
    _case(PSY, [(TON, "runs_team"), (THR, "runs_team")], N=2048, C=3, M=48, psy_tier=1, R=16, tag="M48"),
    _case(PSY, [(TON, "runs_team_R4"), (THR, "runs_team_R4")], N=512, C=3, psy_tier=1, R=4,
          env={"AC_PSY_TEAM_ALWAYS": "1"}, tag="TEAM_ALWAYS"),
    _case(PSY, [(TON, "runs_strided_pairs"), (THR, "runs_strided_pairs")], N=960, C=5, psy_tier=1, R=8,
          env={"AC_PSY_NOTEAM": "1"}, tag="NOTEAM"),
    _case(PSY, [(TON, "band_walk"), (THR, "band_walk")], N=1024, C=2, sr=8000, pre="float32", psy_tier=1, walk=True,
          drown=0.3, tag="8kHz-pre32"),
    _case(PSY, [(TON, "tier0"), (THR, "tier0")], N=1024, C=2, M=100, psy_tier=0, tpw=1, tag="M100"),
    # ---- fused encode (+ decode of its spectra) -----------------------------------------------------------------------
    *[_case(ENC, [("codec.encode", "fused_wave"), ("codec.decode", "after_fused")], N=N, C=C, launches=1)
      for N, C in ((64, 2), (128, 1), (256, 2), (512, 1), (512, 2), (1024, 1), (1024, 2), (2048, 2))],
    # (2048 mono is transform + masking model by design: ac_encode_launches)
    _case(ENC, [("codec.encode", "wave_two_launch"), ("codec.decode", "after_wave")], N=2048, C=1, launches=2),
    _case(ENC, [("codec.encode", "fused_lds"), ("codec.decode", "after_fused")], N=960, C=2, launches=1, drown=0.3, tag="drown"),
    _case(ENC, [("codec.encode", "fused_lds_frame_offsets")], N=2304, C=1, launches=1),
    _case(ENC, [("codec.encode", "fused_lds_frame_offsets")], N=3600, C=2, launches=1),
    _case(ENC, [("codec.encode", "fused_forced")], N=1920, C=2, launches=1, nofuse="2", tag="NOFUSE2"),
    _case(ENC, [("codec.encode", "two_launch")], N=960, C=2, launches=2, nofuse="1", tag="NOFUSE1"),
    _case(ENC, [("codec.encode", "multichannel"), ("codec.decode", "multichannel")], N=1024, C=3, launches=None),
    # ---- 2-byte dtypes ------------------------------------------------------------------------------------------------
    _case(TWO, [("bf16.encode", "wave"), ("bf16.decode", "wave")], N=1024, C=2, dtype="bfloat16", tier=3, drown=0.1, tag="bf16"),
    _case(TWO, [("bf16.encode", "wave"), ("bf16.decode", "wave")], N=1024, C=1, dtype="bfloat16", tier=3, tag="bf16"),
    _case(TWO, [("bf16.encode", "wave"), ("bf16.decode", "wave")], N=2048, C=2, dtype="bfloat16", tier=3, tag="bf16"),
    _case(TWO, [("bf16.encode", "lds"), ("bf16.decode", "lds")], N=960, C=2, dtype="bfloat16", tier=2, tag="bf16"),
    _case(TWO, [("f16.filter_bank", "lds")], N=960, C=2, dtype="float16", tier=2, tag="f16"),
    _case(TWO, [("f16.filter_bank", "wave")], N=1024, C=2, dtype="float16", tier=3, tag="f16"),
    _case(TWO, [("f16.filter_bank", "lds")], N=4096, C=1, dtype="float16", tier=2, tag="f16"),
    # ---- streaming ----------------------------------------------------------------------------------------------------
    _case(STREAM, [("stream.run", "duplex")], N=1024, C=2, B=256, k=32, K_stream=128, masking=True),
    _case(STREAM, [("stream.run", "lds_chain")], N=960, C=2, B=256, k=32, K_stream=128, masking=False),
    # ---- quantiser family ---------------------------------------------------------------------------------------------
    _case(QUANT, [("psy.quantize", "rows"), ("psy.dequantize", "rows"), ("psy.pack", "multi_tile_scan"),
                  ("psy.unpack", "multi_tile_scan")], N=1024, C=2, tpw=1),
    _case(QUANT, [("psy.quantize", "rows"), ("psy.dequantize", "rows"), ("psy.pack", "multi_tile_scan"),
                  ("psy.unpack", "multi_tile_scan")], N=960, C=3, tpw=1),
    _case(RATE, [("psy.quantize_to_budget", "register_scalar"), ("psy.quantize_to_budget", "register_per_row")],
          N=1024, C=2, tpw=1),
    _case(RATE, [("psy.quantize_to_budget", "reread_scalar"), ("psy.quantize_to_budget", "reread_per_row")],
          N=2048, C=2, tpw=1),
    _case(DECQ, [("codec.decode_quantized", "one_launch"), ("codec.decode_packed", "one_launch")], N=1024, C=2, launches=1,
          tpw=1),
    _case(DECQ, [("codec.decode_quantized", "two_launches"), ("codec.decode_packed", "two_launches")], N=960, C=2,
          launches=2, tpw=1),
]


def _params(area):
    return [pytest.param(c, id=c["id"]) for c in CASES if c["area"] == area]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X (run with -m gpu on the GPU box)"
    _lib.load().ac_set_force_generic(0)
    yield
    torch.cuda.empty_cache()


def _check(ratio, bar_name, what):
    v, msg = worst(ratio, bar_name, what)
    assert v <= 1.0, msg
    return v


def _slices(B, K, N, C, bytes_per=24):
    """clips per float64 pass: about 1.5 GiB of float64 work arrays"""
    step = max(1, int((3 << 29) // max(1, K * N * C * bytes_per)))
    return [slice(b, min(B, b + step)) for b in range(0, B, step)]


def _ends(B):
    return [0, B - 1]


def _np(t):
    return t.detach().cpu().numpy()


def _anchor_mdct(N, x_ends, X64_ends, X_ends=None, y64_ends=None):
    """the float64 kernels' results on the first and the last clip against the CPU oracle (1e-12 class bars of
    test_float64_filter_bank_vs_oracle)"""
    o = MDCTOracle(N, "vorbis", np.float64)
    Xo = o.transform(x_ends)
    err = float(np.max(np.abs(X64_ends - Xo)) / np.max(np.abs(Xo)))
    assert err <= 1e-12, ("float64 transform vs oracle", err)
    if y64_ends is not None:
        yo = o.inverse_transform(X_ends)
        err = float(np.max(np.abs(y64_ends - yo)))
        assert err <= 1e-12, ("float64 inverse_transform vs oracle", err)


def _anchor_psy(p64, sr, N, M, X_ends, t_in_ends, t64_ends, thr64_ends, drown):
    """the float64 masking model on the first and the last clip against the CPU oracle (bars of
    test_float64_masking_model_vs_oracle) -- on the plan's own tables, so that a float32-precomputed plan is anchored too"""
    o = PsychoOracle(sr, N, M, compute_dtype=np.float64)
    if p64.precompute_dtype != torch.float64:
        o.W, o.W_inv = p64.W.numpy(), p64.W_inv.numpy()
        o.spreading_matrix = p64.spreading_matrix.numpy()
        o.max_bark = np.float64(float(p64.max_bark))
        o.quiet_threshold_intensity = p64.quiet_threshold_intensity.numpy().reshape(np.shape(o.quiet_threshold_intensity))
    to = o.tonality(X_ends)
    err = float(np.max(np.abs(t64_ends - to)))
    assert err <= 1e-12, ("float64 tonality vs oracle", err)
    tho = o.global_masking_threshold(X_ends, t_in_ends, drown)
    err = float(np.max(np.abs(thr64_ends - tho) / tho))
    assert err <= 1e-10, ("float64 threshold vs oracle", err)


def _finite(*ts):
    for t in ts:
        assert bool(torch.isfinite(t).all()), "non-finite output on a finite input"


# ---- filter bank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _params(FB))
def test_filter_bank(case, monkeypatch):
    N, C, B, K = case["N"], case["C"], case["B"], case["K"]
    if "noteam" in case:
        monkeypatch.setenv("AC_LDS_WAVE_NOTEAM", case["noteam"])
    m = audiocodec_amd.MDCTransformer(N)
    assert m.tier(C) == case["tier"], (m.tier(C), case["tier"])
    x = structured(B, K, N, C, seed=10 * N + C)
    X = m.transform(x)
    y = m.inverse_transform(X)
    torch.cuda.synchronize()
    _finite(X, y)
    m64 = audiocodec_amd.MDCTransformer(N, compute_dtype=torch.float64)
    fx, fl, fy = [], [], []
    ends = {}
    for sl in _slices(B, K, N, C):
        X64 = m64.transform(x[sl].double())
        fx.append(frame_peak_ratio(X[sl], X64, TOL))
        fl.append(clip_l2_ratio(X[sl], X64, TOL))
        y64 = m64.inverse_transform(X[sl].double()) if N <= F64_INV_MAX else None
        if y64 is not None:
            fy.append(abs_ratio(blocks(y[sl], N), blocks(y64, N), LSB))
        for b in _ends(B):
            if sl.start <= b < sl.stop:
                ends[b] = (_np(X64[b - sl.start]), None if y64 is None else _np(y64[b - sl.start]))
        del X64, y64
    _check(torch.cat(fx), "max|dX| <= 1e-4 max|X64| per frame", "tier %d transform vs float64" % case["tier"])
    _check(torch.cat(fl), "rel-L2 <= 1e-4 per clip", "tier %d transform vs float64" % case["tier"])
    e = _ends(B)
    if N <= F64_INV_MAX:
        _check(torch.cat(fy), "1 LSB = 2^-15 per block", "tier %d inverse_transform vs float64" % case["tier"])
        _anchor_mdct(N, _np(x[e].double()), np.stack([ends[b][0] for b in e]), _np(X[e].double()),
                     np.stack([ends[b][1] for b in e]))
    else:
        # the float64 synthesis holds 2 N doubles of LDS (up to 4096): the first and the last clip against the CPU oracle
        _anchor_mdct(N, _np(x[e].double()), np.stack([ends[b][0] for b in e]))
        yo = MDCTOracle(N, "vorbis", np.float64).inverse_transform(_np(X[e].double()))
        err = torch.from_numpy(np.abs(_np(y[e].double()) - yo).reshape(len(e), -1, N, C).max(axis=2)) / LSB
        _check(err, "1 LSB per block", "tier %d inverse_transform vs the oracle (clips 0, B-1)" % case["tier"])


# ---- masking model -----------------------------------------------------------------------------------------------------
def _psy_pair(sr, N, M, pre, spreading=None):
    pre_t = torch.float32 if pre == "float32" else torch.float64
    psy = audiocodec_amd.PsychoacousticModel(sr, N, M, precompute_dtype=pre_t, spreading=spreading)
    p64 = audiocodec_amd.PsychoacousticModel(sr, N, M, compute_dtype=torch.float64, precompute_dtype=pre_t)
    return psy, p64


def _check_masking(p64, case, X, t, thr, drown, bar_thr, what, tbar=None):
    """t, thr (any dtype) against the float64 kernels on X (cast up): tonality from X, threshold from X and the kernel's own
    t -- each kernel on its own input.  tbar None: the tonality bar of SURVEY 8(c); else an absolute bar."""
    B, K = X.shape[0], X.shape[1]
    N, C = X.shape[2], X.shape[3]
    ft, fr = [], []
    ends = {}
    for sl in _slices(B, K, N, C, bytes_per=40):
        X64 = X[sl].double()
        t64 = p64.tonality(X64)
        thr64 = p64.global_masking_threshold(X64, t[sl].double(), drown)
        ft.append(tonality_ratio(t[sl], t64) if tbar is None else abs_ratio(t[sl], t64, tbar))
        fr.append(rel_elem_ratio(thr[sl], thr64, bar_thr))
        for b in _ends(B):
            if sl.start <= b < sl.stop:
                ends[b] = (_np(t64[b - sl.start]), _np(thr64[b - sl.start]))
        del X64, t64, thr64
    vt = _check(torch.cat(ft), "|dt| <= 1e-4 |t| + 1e-6" if tbar is None else "|dt| <= %g" % tbar, what + " tonality vs float64")
    vr = _check(torch.cat(fr), "|dthr| <= %g thr" % bar_thr, what + " threshold vs float64")
    e = _ends(B)
    _anchor_psy(p64, case.get("sr", 48000), N, case.get("M", 64), _np(X[e].double()), _np(t[e].double()),
                np.stack([ends[b][0] for b in e]), np.stack([ends[b][1] for b in e]), drown)
    return vt, vr


@pytest.mark.parametrize("case", _params(PSY))
def test_masking_model(case, monkeypatch):
    N, C, B, K = case["N"], case["C"], case["B"], case["K"]
    sr, M, drown = case.get("sr", 48000), case.get("M", 64), case.get("drown", 0.0)
    for k, v in case.get("env", {}).items():
        monkeypatch.setenv(k, v)
    psy, p64 = _psy_pair(sr, N, M, case.get("pre"), case.get("spreading"))
    assert psy.tier() == case["psy_tier"], (psy.tier(), case["psy_tier"])
    if "spreading" in case:
        assert psy.plan_spreading() == case["spreading"]
    img = runs_image(_lib.load(), N, M, sr, 0.6, precompute=0 if case.get("pre") == "float32" else 1)
    if case.get("walk"):
        assert img is None                                   # no runs image: the band walk (k_psy_mid)
    elif case["psy_tier"] == 1:
        assert img is not None and granule_registers(N) == case["R"]
    x = structured(B, K, N, C, seed=20 * N + C + M)
    X = audiocodec_amd.MDCTransformer(N).transform(x)
    del x
    t = psy.tonality(X)
    thr = psy.global_masking_threshold(X, t, drown)
    torch.cuda.synchronize()
    _finite(t, thr)
    bar = SPREAD_TOL[psy.plan_spreading()]
    if psy.plan_spreading() == "bf16_mfma":
        # bfloat16 operands of the spreading product round each factor by up to 2^-9, a product by up to 2^-8; the threshold
        # takes that sum of intensities to the power 1 / alpha (alpha = 0.6), which scales a relative error by 1 / alpha:
        # 2^-8 / 0.6 = 6.5e-3.  The 5e-3 of the small tests was measured on uniform noise; on this input the worst frame
        # is 5.95e-3 (983 of 66834 frames above 5e-3, in clips of every kind), bit-equal when its clip runs alone in a
        # one-clip launch: the data's conditioning, not the launch.
        bar = 2.0 ** -8 / 0.6
    _check_masking(p64, case, X, t, thr, drown, bar, "psy tier %d" % case["psy_tier"])


# ---- fused encode ------------------------------------------------------------------------------------------------------
def _check_decode(codec, m64, X, y, what, pcm16=None):
    """y = decode(X) against the float64 inverse of the same coefficients, per block (1 LSB); pcm16 = decode(X, pcm16=True)
    against the float64 result rounded (within 1 LSB)"""
    N = X.shape[2]
    B, K, C = X.shape[0], X.shape[1], X.shape[3]
    fy, fp = [], []
    for sl in _slices(B, K, N, C):
        y64 = m64.inverse_transform(X[sl].double())
        fy.append(abs_ratio(blocks(y[sl], N), blocks(y64, N), LSB))
        if pcm16 is not None:
            ref = torch.clamp(torch.round(y64 * 32768.0), -32768, 32767)
            fp.append(abs_ratio(blocks(pcm16[sl], N), blocks(ref, N), 1.0))
        del y64
    _check(torch.cat(fy), "1 LSB = 2^-15 per block", what + " decode vs float64")
    if pcm16 is not None:
        _check(torch.cat(fp), "1 LSB of int16 per block", what + " decode(pcm16) vs float64 rounded")


@pytest.mark.parametrize("case", _params(ENC))
def test_fused_encode(case, monkeypatch):
    N, C, B, K = case["N"], case["C"], case["B"], case["K"]
    drown = case.get("drown", 0.0)
    if "nofuse" in case:
        monkeypatch.setenv("AC_LDS_WAVE_NOFUSE", case["nofuse"])
    codec = audiocodec_amd.AudioCodec(48000, N)
    if case["launches"] is not None:
        assert codec.encode_launches(C) == case["launches"]
    else:
        assert codec.encode_launches(C) > 1                     # (C >= 3: transform + masking model)
    if case.get("nofuse") == "2":
        monkeypatch.delenv("AC_LDS_WAVE_NOFUSE")
        assert codec.encode_launches(C) == 2                    # (a size where fusing does not pay: forced above)
        monkeypatch.setenv("AC_LDS_WAVE_NOFUSE", "2")
    x = structured(B, K, N, C, seed=30 * N + C)
    X, t, thr = codec.encode(x, drown)
    torch.cuda.synchronize()
    _finite(X, t, thr)
    m64 = audiocodec_amd.MDCTransformer(N, compute_dtype=torch.float64)
    p64 = audiocodec_amd.PsychoacousticModel(48000, N, compute_dtype=torch.float64)
    fx, fl = [], []
    ends = {}
    for sl in _slices(B, K, N, C):
        X64 = m64.transform(x[sl].double())
        fx.append(frame_peak_ratio(X[sl], X64, TOL))
        fl.append(clip_l2_ratio(X[sl], X64, TOL))
        for b in _ends(B):
            if sl.start <= b < sl.stop:
                ends[b] = _np(X64[b - sl.start])
        del X64
    what = "encode (%s launches)" % case["launches"]
    _check(torch.cat(fx), "max|dX| <= 1e-4 max|X64| per frame", what + " X vs float64")
    _check(torch.cat(fl), "rel-L2 <= 1e-4 per clip", what + " X vs float64")
    e = _ends(B)
    _anchor_mdct(N, _np(x[e].double()), np.stack([ends[b] for b in e]))
    del x
    _check_masking(p64, case, X, t, thr, drown, SPREAD_TOL[codec.psy.plan_spreading()], what)
    if any(entry == "codec.decode" for entry, _ in case["covers"]):
        y = codec.decode(X)
        pcm = codec.decode(X, pcm16=True) if N in PCM16_SIZES and C <= 2 else None
        torch.cuda.synchronize()
        _finite(y)
        _check_decode(codec, m64, X, y, what, pcm)


# ---- 2-byte dtypes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _params(TWO))
def test_two_byte_dtypes(case):
    """bars of test_bfloat16_filter_bank / test_float16_filter_bank / test_bfloat16_fused_encode: X 4e-3 (bfloat16) /
    1e-3 (float16) of the frame peak, tonality 4e-3 absolute, threshold 6e-3 relative, synthesis 4e-3 / 1e-3 of
    max(1, peak) -- against the float64 kernels on the very 2-byte values the kernels read"""
    N, C, B, K = case["N"], case["C"], case["B"], case["K"]
    dt = getattr(torch, case["dtype"])
    xbar = 4e-3 if dt == torch.bfloat16 else 1e-3
    # float16 has subnormals below 2^-14, spaced 2^-24: a coefficient stored there is rounded by up to 2^-25 absolute
    # whatever the frame's peak.  The quiet clips of this input (gains down to 1e-4) have whole frames down there, where
    # 1e-3 of the peak is below the format's resolution (measured without the floor: up to 22.6x the bar, all in such
    # frames); the bar is 1e-3 of the peak plus that half spacing.  bfloat16 has float32's exponent range: no floor.
    xfloor = 2.0 ** -25 if dt == torch.float16 else 0.0
    drown = case.get("drown", 0.0)
    assert audiocodec_amd.MDCTransformer(N).tier(C) == case["tier"]
    x = structured(B, K, N, C, seed=40 * N + C, dtype=dt)
    m64 = audiocodec_amd.MDCTransformer(N, compute_dtype=torch.float64)
    if dt == torch.bfloat16:
        codec = audiocodec_amd.AudioCodec(48000, N, compute_dtype=dt)
        X, t, thr = codec.encode(x, drown)
        _finite(t, thr)
    else:
        codec = None
        X = audiocodec_amd.MDCTransformer(N, compute_dtype=dt).transform(x)
    y = (codec.decode(X) if codec is not None else audiocodec_amd.MDCTransformer(N, compute_dtype=dt).inverse_transform(X))
    torch.cuda.synchronize()
    assert X.dtype == dt and y.dtype == dt
    _finite(X, y)
    fx, fy = [], []
    ends = {}
    for sl in _slices(B, K, N, C):
        X64 = m64.transform(x[sl].double())
        fx.append(frame_peak_ratio(X[sl], X64, xbar, xfloor))
        y64 = m64.inverse_transform(X[sl].double())
        fy.append(abs_ratio(blocks(y[sl], N), blocks(y64, N), xbar * max(1.0, float(y64.abs().max()))))
        for b in _ends(B):
            if sl.start <= b < sl.stop:
                ends[b] = _np(X64[b - sl.start])
        del X64, y64
    what = "%s tier %d" % (case["dtype"], case["tier"])
    _check(torch.cat(fx), "max|dX| <= %g max|X64| + %g per frame" % (xbar, xfloor), what + " transform vs float64")
    _check(torch.cat(fy), "%g max(1, peak) per block" % xbar, what + " synthesis vs float64")
    e = _ends(B)
    _anchor_mdct(N, _np(x[e].double()), np.stack([ends[b] for b in e]))
    if codec is not None:
        p64 = audiocodec_amd.PsychoacousticModel(48000, N, compute_dtype=torch.float64)
        _check_masking(p64, case, X, t, thr, drown, 6e-3, what, tbar=4e-3)


# ---- streaming ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _params(STREAM))
def test_stream_run(case):
    """StreamingMDCT.run on B streams in chunks of k blocks (the duplex kernel at 1024 stereo: analysis of chunk i + 1 and
    synthesis of chunk i in one launch) against the one-shot float64 transform and inverse of the concatenated input"""
    N, C, B, k, K = case["N"], case["C"], case["B"], case["k"], case["K_stream"]
    masking = case["masking"]
    codec = audiocodec_amd.AudioCodec(48000, N)
    assert codec.mdct.tier(C) == (3 if N in (1024, 2048) else 2)
    x = structured(B, K, N, C, seed=50 * N + C)
    st = codec.stream(B, C)
    chunks = [x[:, i * k * N:(i + 1) * k * N].contiguous() for i in range(K // k)]
    Xl, tl, thrl, xhl = st.run(chunks, k, masking=masking, drown=0.0)
    torch.cuda.synchronize()
    X, xh = torch.cat(Xl, dim=1), torch.cat(xhl, dim=1)
    del chunks, Xl, xhl
    _finite(X, xh)
    m64 = audiocodec_amd.MDCTransformer(N, compute_dtype=torch.float64)
    fx, fy = [], []
    for sl in _slices(B, K, N, C):
        X64 = m64.transform(x[sl].double())[:, :K]
        fx.append(frame_peak_ratio(X[sl], X64, TOL))
        y64 = m64.inverse_transform(X64)[:, :K * N]
        fy.append(abs_ratio(blocks(xh[sl], N), blocks(y64, N), LSB))
        del X64, y64
    _check(torch.cat(fx), "max|dX| <= 1e-4 max|X64| per frame", "stream.run X vs one-shot float64")
    _check(torch.cat(fy), "1 LSB per block", "stream.run synthesis vs one-shot float64")
    if masking:
        t, thr = torch.cat(tl, dim=1), torch.cat(thrl, dim=1)
        _finite(t, thr)
        p64 = audiocodec_amd.PsychoacousticModel(48000, N, compute_dtype=torch.float64)
        _check_masking(p64, case, X, t, thr, 0.0, SPREAD_TOL[codec.psy.plan_spreading()], "stream.run")
    st.close()


# ---- quantiser family --------------------------------------------------------------------------------------------------
def _encoded(case):
    N, C, B, K = case["N"], case["C"], case["B"], case["K"]
    codec = audiocodec_amd.AudioCodec(48000, N)
    x = structured(B, K, N, C, seed=60 * N + C)
    X, _, thr = codec.encode(x)
    del x
    assert B * (K + 1) >= MIN_WORKGROUPS                       # one workgroup per (clip, frame) row at least
    return codec, X, thr


def _inject(X, thr, N, C):
    """the small tests' adversarial rows, in the last rows of the grid: zeros, 1e9-scaled bands, NaN and +-Inf"""
    X[-1, -1] = 0.0
    X[-1, -2, : N // 2] *= 1e9
    X[-1, -3, N // 3, 0] = np.nan
    thr[-1, -4, N - 1, C - 1] = np.inf
    X[-2, -1, 0, C - 1] = -np.inf
    X[-2, -2, N // 2, 0] = np.inf
    X[-1, -5, N // 4:, C - 1] = 0.0


def _rows_equal(a, b, what):
    """bit-equal arrays [B, F, ..., C]: on a mismatch the worst (clip, frame, channel) and the count of rows that differ"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        diff = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    else:
        diff = a != b
    rows = diff.any(axis=2)
    if rows.any():
        idx = np.argwhere(rows)
        raise AssertionError("%s: %d of %d (clip, frame, channel) rows differ, first at %s" % (
            what, len(idx), rows.size, tuple(int(v) for v in idx[0])))


@pytest.mark.parametrize("case", _params(QUANT))
def test_quantiser_and_pack(case):
    from pack_reference import np_canon, np_pack
    from test_quantizer import np_dequantize, np_quantize
    N, C = case["N"], case["C"]
    codec, X, thr = _encoded(case)
    psy = codec.psy
    off = psy.scale_band_offsets
    Xn, tn = _np(X), _np(thr)
    _inject(Xn, tn, N, C)
    codes, sf = psy.quantize(torch.from_numpy(Xn).cuda(), torch.from_numpy(tn).cuda())
    rc, rs = np_quantize(Xn, tn, off)
    _rows_equal(_np(sf), rs, "quantize sf")
    _rows_equal(_np(codes), rc, "quantize codes")
    assert (rs[-1] == -128).any() and (np.abs(rc[-1]) == 32767).any()
    Xh = _np(psy.dequantize(codes, sf))
    _rows_equal(Xh, np_dequantize(rc, rs, off), "dequantize")
    data, index = psy.pack(codes, sf)
    rd, ri = np_pack(rc, rs, off)
    np.testing.assert_array_equal(_np(index), ri)
    assert data.numel() == len(rd)
    dn = _np(data)
    if not np.array_equal(dn, rd):
        first = int(np.argmax(dn != rd))
        row = np.unravel_index(int(np.searchsorted(ri.reshape(-1), first, side="right") - 1), ri.shape)
        raise AssertionError("pack: %d bytes differ, first in row (clip, frame, channel) = %s" % (
            int((dn != rd).sum()), tuple(int(v) for v in row)))
    assert index.numel() >= 2 * 2048                           # (several 2048-row tiles of the index scan)
    c, s = psy.unpack(data, index)
    cc, cs = np_canon(rc, rs, off)
    _rows_equal(_np(s), cs, "unpack sf")
    _rows_equal(_np(c), cc, "unpack codes")


def _bisect_budget(X, thr, off, R, kmin):
    """rate_reference.quantize_budget with the scan over k replaced by a bisection (rule 2: bits_r(k) does not grow with
    k), so that a chip-sized grid is checked in seconds; _finish and fast_bits are the restatement's own"""
    from rate_reference import K_MAX, _finish, band_extremes, fast_bits
    from test_quantizer import np_quantize
    X = np.asarray(X, dtype=np.float32)
    _, sf0 = np_quantize(X, thr, off)
    xmax, xmin = band_extremes(X, off)
    B, F, N, C = X.shape
    Rb = np.broadcast_to(np.asarray(R, dtype=np.int64), (B, F, C))
    lo = np.full((B, F, C), kmin, dtype=np.int64)             # smallest k that may meet the budget
    hi = np.full((B, F, C), K_MAX, dtype=np.int64)            # K_MAX: met there or not at all
    while (lo < hi).any():
        act = lo < hi
        mid = (lo + hi) // 2
        met = fast_bits(sf0, xmax, xmin, off, mid[:, :, None, :]) <= Rb
        hi = np.where(act & met, mid, hi)
        lo = np.where(act & ~met, mid + 1, lo)
    return _finish(X, sf0, off, lo)


@pytest.mark.parametrize("case", _params(RATE))
def test_quantize_to_budget(case):
    from pack_reference import np_row_bits
    from rate_reference import quantize_budget
    from test_quantizer import np_quantize
    N, C = case["N"], case["C"]
    codec, X, thr = _encoded(case)
    psy = codec.psy
    off = psy.scale_band_offsets
    Xn, tn = _np(X), _np(thr)
    _inject(Xn, tn, N, C)
    Xd, td = torch.from_numpy(Xn).cuda(), torch.from_numpy(tn).cuda()
    natural = np_row_bits(*np_quantize(Xn, tn, off), off)
    rng = np.random.default_rng(N + C)
    per_row = np.maximum(5 * 64, natural * rng.uniform(0.05, 1.05, natural.shape)).astype(np.int32)
    scalar = codec.row_bits_for_bitrate(96000)
    # the bisection is the full scan of rate_reference on the first and the last two clips
    sub = [0, Xn.shape[0] - 2, Xn.shape[0] - 1]
    for R, kmin in ((scalar, 0), (per_row, -20)):
        Rs = R if np.isscalar(R) else R[sub]
        ref = _bisect_budget(Xn[sub], tn[sub], off, Rs, kmin)
        full = quantize_budget(Xn[sub], tn[sub], off, Rs, kmin)
        for a, b in zip(ref, full):
            np.testing.assert_array_equal(a, b)
    seen = set()
    for R, kmin in ((scalar, 0), (per_row, -20)):
        Rd = R if np.isscalar(R) else torch.from_numpy(R).cuda()
        codes, sf, offset, bits = psy.quantize_to_budget(Xd, td, Rd, min_offset=kmin)
        rc, rs, ro, rb = _bisect_budget(Xn, tn, off, R, kmin)
        _rows_equal(_np(offset)[:, :, None], ro[:, :, None], "quantize_to_budget offset")
        _rows_equal(_np(bits)[:, :, None], rb[:, :, None], "quantize_to_budget row_bits")
        _rows_equal(_np(sf), rs, "quantize_to_budget sf")
        _rows_equal(_np(codes), rc, "quantize_to_budget codes")
        seen.update(np.unique(ro).tolist())
    assert len(seen) > 3


@pytest.mark.parametrize("case", _params(DECQ))
def test_decode_quantized(case):
    """decode_quantized / decode_packed against the float64 inverse of np_dequantize(codes, sf), per block (1 LSB), and
    their pcm16 forms against it rounded"""
    from test_quantizer import np_dequantize
    N, C = case["N"], case["C"]
    codec, X, thr = _encoded(case)
    assert codec.decode_quantized_launches(C) == case["launches"]
    codes, sf = codec.psy.quantize(X, thr)
    del X, thr
    Xq = torch.from_numpy(np_dequantize(_np(codes), _np(sf), codec.psy.scale_band_offsets)).cuda()
    assert bool(torch.isfinite(Xq).all())
    m64 = audiocodec_amd.MDCTransformer(N, compute_dtype=torch.float64)
    y = codec.decode_quantized(codes, sf)
    p = codec.decode_quantized(codes, sf, pcm16=True)
    _check_decode(codec, m64, Xq, y, "decode_quantized (%d launches)" % case["launches"], p)
    data, index = codec.psy.pack(codes, sf)
    y2 = codec.decode_packed(data, index)
    p2 = codec.decode_packed(data, index, pcm16=True)
    _check_decode(codec, m64, Xq, y2, "decode_packed (%d launches)" % case["launches"], p2)
