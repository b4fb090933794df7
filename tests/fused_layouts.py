"""Shared pieces of tests/test_fused_layouts.py: the scale-band layouts the fused quantise / pack / decode kernels at
filters_n = 1024 are run on besides 48000 Hz, the facts that say why each layout is in the set, the ``tonal`` input whose
rows hold wide code fields, and the conditions a reference must show before anything is compared with it.

Nothing here touches a GPU except ``empty_rate`` where one is present (it asks the library for launch counts).
"""

import functools

import numpy as np

import audiocodec_amd
from oracle.audiocodec_oracle import MDCTOracle, PsychoOracle
from pack_reference import _rows, np_code_fields, np_widths
from test_quantizer import np_offsets, np_quantize

N0, M0 = 1024, 64
B0, K0 = 3, 5                                                    # five blocks: both edge frames; three mono clips: a half-empty pair
EMPTY_RATES = (120000, 118000, 122000, 116000, 124000)           # sample rates whose layout holds an empty scale band
EMPTY = "EMPTY"
# (id, sample rate, alpha); EMPTY resolves to one of EMPTY_RATES on the built library (empty_rate)
LAYOUTS = [("8000", 8000, 0.6), ("44100", 44100, 0.6), ("44100-alpha0.8", 44100, 0.8), ("96000", 96000, 0.6), (EMPTY, None, 0.6)]
LAYOUT_IDS = [l[0] for l in LAYOUTS]
# why each fixed layout is in the set, from np_offsets: (empty bands, one-bin bands, longest band, first six band lengths).
# 48000, the rate every other test uses, has (0, 1, 68, 2 2 1 2 2 2)
FACTS = {8000: (0, 0, 41, (6, 6, 7, 6, 6, 7)), 44100: (0, 0, 67, (2, 2, 2, 2, 2, 2)), 96000: (0, 11, 78, (1, 1, 1, 1, 1, 1))}


def host_offsets(sample_rate):
    """``psy.scale_band_offsets`` at (sample_rate, 1024, 64): a host call of the built library."""
    return audiocodec_amd.PsychoacousticModel(sample_rate, filter_bands_n=N0, bark_bands_n=M0).scale_band_offsets


def layout_counts(off):
    """(empty bands, one-bin bands, granules -- bins 2g, 2g + 1 -- whose bins lie in two bands)"""
    off = np.asarray(off, dtype=np.int64)
    L = np.diff(off)
    band = np.repeat(np.arange(len(L)), L)
    return int((L == 0).sum()), int((L == 1).sum()), int((band[0::2] != band[1::2]).sum())


def has_empty_band(off):
    return bool((np.diff(np.asarray(off, dtype=np.int64)) == 0).any())


@functools.lru_cache(maxsize=None)
def empty_rate():
    """The first of EMPTY_RATES whose host offsets show an empty band and, where a GPU is present, whose codec quantises in the
    fused encode's one launch for mono and stereo; None if there is none."""
    import torch
    for sr in EMPTY_RATES:
        if not has_empty_band(host_offsets(sr)):
            continue
        if torch.cuda.is_available():
            codec = audiocodec_amd.AudioCodec(sr, N0)
            if not all(codec.encode_quantized_launches(C) == 1 for C in (1, 2)):
                continue
        return sr
    return None


def resolve(layout):
    """(sample rate, alpha) of an entry of LAYOUTS."""
    name, sr, alpha = layout
    if name == EMPTY:
        sr = empty_rate()
        assert sr is not None, "no rate of %s has an empty scale band on the one-launch route" % (EMPTY_RATES,)
    return sr, alpha


# ---- inputs ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tonal(C):
    """float32 [B0, K0 N0, C], |x| <= 1: clip 0 ramped noise; clip 1 a noise floor of 1e-4 under four sinusoids at the centres
    of bins 40, 200, 520 and 900; clip 2 a quiet ramped noise and, in its last channel, a decaying harmonic comb (0.5 / h at
    7.5 h bins, h < 120).  Peaks and a low floor side by side: rows with many different code widths, up to 10 bits and more."""
    S = K0 * N0
    rng = np.random.default_rng(4242 + C)
    n = np.arange(S, dtype=np.float64)
    x = np.zeros((B0, S, C))
    x[0] = rng.uniform(-1, 1, (S, C)) * np.linspace(0.01, 1, S)[:, None]
    x[1] = 1e-4 * rng.uniform(-1, 1, (S, C))
    for c in range(C):
        for k, a in ((40.5, 0.3), (200.5, 0.25), (520.5, 0.2), (900.5, 0.25)):
            x[1, :, c] += a * np.sin(np.pi * k / N0 * n + 0.7 * c + k)
    x[2] = 0.01 * rng.uniform(-1, 1, (S, C)) * np.linspace(0.01, 1, S)[:, None]
    x[2, :, C - 1] = sum(0.5 / h * np.sin(np.pi * 7.5 * h / N0 * n + h) for h in range(1, 120))
    x /= max(1.0, np.abs(x).max())
    return x.astype(np.float32)


def tonal16(C):
    """int16 PCM of ``tonal``: rint(32767 x)."""
    return np.rint(32767.0 * tonal(C).astype(np.float64)).astype(np.int16)


def oracle_codes(x, sample_rate, alpha, off):
    """codes and sf of ``np_quantize`` on the float32 numpy oracle's spectra and thresholds of x: the reference alone."""
    X = MDCTOracle(N0, "vorbis", np.float32).transform(np.asarray(x, dtype=np.float32))
    psy = PsychoOracle(sample_rate, N0, M0, alpha=alpha, compute_dtype=np.float32)
    thr = psy.global_masking_threshold(X, psy.tonality(X))
    return np_quantize(X, thr, off)


# ---- what a reference must show ------------------------------------------------------------------------------------------
def width_facts(codes, sf, off):
    """Of reference codes: (histogram {width: bands} of the stored widths 1..16, rows that hold a code field of at least 9
    bits which crosses a 32-bit word boundary).  Rows start on word boundaries, so positions count from the row's start."""
    cr, sr = _rows(np.asarray(codes), np.asarray(sf))
    w = np_widths(cr[:, :, None], sr[:, :, None], off)[:, :, 0]
    stored = w[(w >= 1) & (w <= 16)]
    hist = {int(k): int(v) for k, v in zip(*np.unique(stored, return_counts=True))}
    pos, wb, keep = np_code_fields(w, off)
    crossing = keep & (wb >= 9) & ((pos % 32) + wb > 32)
    return hist, int(crossing.any(axis=1).sum())


def assert_wide(codes, sf, off):
    """The condition on ``tonal``, on a reference's codes: at least eight distinct stored widths, the largest at least 10, and
    a row with a code field of 9 bits or more across a word boundary.  Returns the histogram."""
    hist, crossing_rows = width_facts(codes, sf, off)
    assert len(hist) >= 8, "only %d distinct stored widths: %s" % (len(hist), hist)
    assert max(hist) >= 10, "largest stored width %d" % max(hist)
    assert crossing_rows >= 1, "no row with a field of >= 9 bits across a 32-bit word boundary"
    return hist
