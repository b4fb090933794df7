"""Inputs and per-frame comparisons for tests/test_chip_scale.py: launches that fill the MI355X (256 CUs, >= 8 workgroups
each, several rounds of waves), held frame by frame to the float64 kernels.

The input is deterministic (one seeded torch generator on the device) and mixes what the masking model reacts to: pure tones
and sweeps, noise, tone plus noise, per-clip gains over 1e-4 ... 1, runs of all-zero blocks, one full-scale clip, and
distinct content in the last clips and the last blocks (the tail of the grid and its last partial workgroup).
"""

import math

import numpy as np
import torch

CLIP_SAMPLES = 144000          # the clip length of test_fused_encode_at_launches_that_fill_the_chip (3 s at 48 kHz)
MIN_CLIPS = 96                 # ... and its clip count: no case here is smaller
CUS = 256
MIN_WORKGROUPS = 8 * CUS       # 2048


def blocks_per_clip(N):
    return max(2, CLIP_SAMPLES // N)


def clips_for(N, C, tasks_per_workgroup=8, rows_per_clip=None):
    """Clips for a launch of at least MIN_WORKGROUPS workgroups when a workgroup takes ``tasks_per_workgroup`` (frame,
    channel pair) tasks -- mono signals pair up two clips -- and never fewer than MIN_CLIPS."""
    F = rows_per_clip if rows_per_clip is not None else blocks_per_clip(N) + 1
    pairs = (C + 1) // 2 if C > 1 else 0.5
    need = math.ceil(MIN_WORKGROUPS * tasks_per_workgroup / (F * pairs))
    return max(MIN_CLIPS, need)


def structured(B, K, N, C, seed, dtype=torch.float32, device="cuda"):
    """[B, K N, C] test signal in -1 ... 1 (see the module docstring); built in float64 on the device, rounded once."""
    g = torch.Generator(device=device).manual_seed(seed)
    S = K * N
    n = torch.arange(S, device=device, dtype=torch.float64).view(1, S, 1)

    def u(*shape):
        return torch.rand(shape, generator=g, device=device, dtype=torch.float64)

    kind = torch.arange(B, device=device) % 4                          # 0 tones, 1 sweep, 2 noise, 3 tone + noise
    kind = kind.view(B, 1, 1)
    # three partials per clip and channel at 20 Hz ... 0.45 fs (in cycles per sample), random phases and weights
    f = (20.0 / 48000.0) * (0.45 * 48000.0 / 20.0) ** u(B, 3, C)
    ph = 2 * math.pi * u(B, 3, C)
    w = 0.2 + u(B, 3, C)
    w = w / w.sum(dim=1, keepdim=True)
    tone = torch.zeros(B, S, C, device=device, dtype=torch.float64)
    for p in range(3):
        tone += w[:, p:p + 1] * torch.sin(2 * math.pi * f[:, p:p + 1] * n + ph[:, p:p + 1])
    # exponential sweep from f0 to f1 over the clip
    f0 = (30.0 / 48000.0) * (1.0 + 9.0 * u(B, 1, C))
    f1 = 0.2 + 0.29 * u(B, 1, C)
    r = torch.log(f1 / f0)
    sweep = torch.sin(2 * math.pi * f0 * S / r * (torch.exp(r * n / S) - 1.0) + 2 * math.pi * u(B, 1, C))
    noise = 2 * u(B, S, C) - 1
    x = torch.where(kind == 0, tone, torch.where(kind == 1, sweep, torch.where(kind == 2, noise, 0.7 * tone + 0.3 * noise)))
    gain = 10.0 ** (-4.0 * u(B, 1, C))                                 # 1e-4 ... 1 per clip and channel
    gain[0] = 1.0
    x = x * gain
    # a few runs of all-zero blocks (three blocks: at least one all-zero frame), in every seventh clip
    for b in range(3, B, 7):
        k0 = (b * 5) % max(1, K - 3)
        x[b, k0 * N:(k0 + 3) * N] = 0.0
    # one full-scale clip: a tone clipped at +-1 (peaks exactly 1)
    fs = B // 2
    x[fs] = torch.clamp(1.6 * tone[fs], -1.0, 1.0)
    # the tail of the grid: the last clip a loud sweep up to 0.49 fs with an impulse train in its last block, the clip
    # before it quiet noise whose last two blocks are silent, the last block of every clip a tone burst of its own
    last = B - 1
    fl0, fl1 = 40.0 / 48000.0, 0.49
    rl = math.log(fl1 / fl0)
    x[last] = 0.9 * torch.sin(2 * math.pi * fl0 * S / rl * (torch.exp(rl * n[0] / S) - 1.0))
    x[last, S - N::max(1, N // 8)] = -1.0
    if B >= 2:
        x[B - 2] = 1e-3 * noise[B - 2]
        x[B - 2, S - min(2, K) * N:] = 0.0
    burst = torch.sin(2 * math.pi * (0.05 + 0.4 * u(B, 1, C)) * n[:, :N]) * torch.hann_window(N, device=device, dtype=torch.float64).view(1, N, 1)
    x[:B - 2, S - N:] = 0.5 * burst[:B - 2] * gain[:B - 2]
    return x.to(dtype)


# ---- comparisons ---------------------------------------------------------------------------------------------------
def worst(ratio, bar_name, what):
    """ratio [B, F, C] (error / bar per frame and channel; NaN counts as failing) -> (worst ratio, message).  The message
    names the worst (clip, frame, channel) and how many frames exceed the bar."""
    r = torch.nan_to_num(ratio.double(), nan=float("inf"))
    bad = int((r > 1.0).sum())
    i = int(torch.argmax(r.reshape(-1)))
    idx = np.unravel_index(i, tuple(r.shape))
    v = float(r.reshape(-1)[i])
    msg = "%s: worst %.3g of the bar (%s) at (clip, frame, channel) = %s; %d of %d frames over the bar" % (
        what, v, bar_name, tuple(int(a) for a in idx), bad, r.numel())
    return v, msg


def frame_peak_ratio(X, X64, bar, floor=0.0):
    """per-frame max|dX| / (bar max|X64| + floor) over the filters axis (2): [B, F, C]"""
    d = (X.double() - X64).abs().amax(dim=2)
    den = bar * X64.abs().amax(dim=2) + floor
    return torch.where(d == 0, torch.zeros_like(d), d / den.clamp_min(1e-300))


def clip_l2_ratio(X, X64, bar):
    """per-clip and channel rel-L2 [B, 1, C] in units of ``bar``"""
    d = (X.double() - X64).pow(2).sum(dim=(1, 2)).sqrt()
    den = X64.pow(2).sum(dim=(1, 2)).sqrt()
    return (torch.where(d == 0, torch.zeros_like(d), d / den.clamp_min(1e-300)) / bar).unsqueeze(1)


def tonality_ratio(t, t64):
    """conftest.tonality_err per frame: |t - t64| / (1e-4 |t64| + 1e-6), [B, F, C]"""
    return ((t.double() - t64).abs() / (1e-4 * t64.abs() + 1e-6)).amax(dim=2)


def abs_ratio(a, a64, bar, axis=2):
    """max |a - a64| / bar over ``axis``"""
    return (a.double() - a64).abs().amax(dim=axis) / bar


def rel_elem_ratio(thr, thr64, bar):
    """element-wise |thr - thr64| / thr64 per frame, in units of ``bar``: [B, F, C]"""
    return ((thr.double() - thr64).abs() / thr64).amax(dim=2) / bar


def blocks(y, N):
    """[B, K N, C] -> [B, K, N, C] (per-block views for per-frame reports of PCM)"""
    B, S, C = y.shape
    return y.reshape(B, S // N, N, C)
