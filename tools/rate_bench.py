"""Rate control at the bench workload (B = 256 clips, stereo, K = 468 blocks, filters_n 1024): quantize_to_budget at a tight
and a loose budget and quantize_to_clip_budget (one budget per clip) against quantize() on the same
tensors, timed with HIP events (every call allocates its results); then the packed size (bits per sample), the share of
rows that met their budget and the share of the budget used, per row and per clip, at a few bitrates.
python tools/rate_bench.py [--clips 256] [--blocks 468] [--filters 1024] [--steps 50] [--warmup 5]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audiocodec_amd  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=468)
    ap.add_argument("--filters", type=int, default=1024)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bitrates", default="32000,64000,128000", help="bits per second per channel, comma-separated")
    a = ap.parse_args()
    B, K, N, C = a.clips, a.blocks, a.filters, a.channels
    codec = audiocodec_amd.AudioCodec(48000, N)
    psy = codec.psy
    M = psy.bark_bands_n
    x = (torch.rand((B, K * N, C), device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
    X, _, thr = codec.encode(x)
    del x
    F = K + 1
    rows, nbin = B * F * C, B * F * N * C
    code_b, sf_b, row_b = nbin * 2, B * F * M * C, rows * (2 + 4)
    tight, loose = codec.row_bits_for_bitrate(32000), 16 * N + 13 * M
    clip_tight, clip_loose = codec.clip_bits_for_bitrate(32000, F, C), F * C * 32 * ((loose + 31) // 32)
    # the clip call, by the bytes its kernels request: X and thr read and the band statistics (12 M bytes per row) written;
    # the statistics read by each of the 8 search steps from kmin = 0 and by k_clip_rows, their meta words by k_clip_codes;
    # 8 bytes of row bits per row written and read; X read again.  (The repeated reads may be served from cache.)
    stat_b = rows * 12 * M
    clip_b = nbin * 12 + code_b + sf_b + row_b + stat_b * (1 + 8 + 1) + stat_b // 3 + rows * 16
    print("rate_bench: B=%d K=%d N=%d C=%d M=%d  tight budget %d bits/row (32 kbit/s), loose %d  %s"
          % (B, K, N, C, M, tight, loose, torch.cuda.get_device_name()))
    cases = [
        ("quantize", lambda: psy.quantize(X, thr), nbin * 8 + code_b + sf_b),
        ("quantize_to_budget tight", lambda: psy.quantize_to_budget(X, thr, tight), nbin * 8 + code_b + sf_b + row_b),
        ("quantize_to_budget loose", lambda: psy.quantize_to_budget(X, thr, loose), nbin * 8 + code_b + sf_b + row_b),
        ("quantize_to_clip_budget tight", lambda: psy.quantize_to_clip_budget(X, thr, clip_tight), clip_b),
        ("quantize_to_clip_budget loose", lambda: psy.quantize_to_clip_budget(X, thr, clip_loose), clip_b),
    ]
    res = {}
    for name, fn, nbytes in cases:
        ms = timed(fn, a.steps, a.warmup)
        res[name] = ms
        print("%-30s %8.3f ms  %6.3f GB requested  %6.2f TB/s" % (name, ms, nbytes / 1e9, nbytes / ms / 1e9))
    for name in ("quantize_to_budget tight", "quantize_to_budget loose"):
        print("%s / quantize = %.3f" % (name, res[name] / res["quantize"]))
    for name in ("tight", "loose"):
        print("quantize_to_clip_budget %s / quantize_to_budget %s = %.3f"
              % (name, name, res["quantize_to_clip_budget " + name] / res["quantize_to_budget " + name]))

    codes, sf = psy.quantize(X, thr)
    data, _ = psy.pack(codes, sf)
    print("no budget: %.3f bits per sample" % (8.0 * data.numel() / nbin))
    for bps in (int(v) for v in a.bitrates.split(",")):
        R = codec.row_bits_for_bitrate(bps)
        codes, sf, offset, row_bits = psy.quantize_to_budget(X, thr, R)
        data, _ = psy.pack(codes, sf)
        met = (row_bits <= R).double().mean().item()
        print("%6d bit/s per channel: budget %5d bits/row (%.3f bits per sample)  packed %.3f bits per sample  "
              "budget used %.4f  rows met %.4f  offset mean %.2f max %d"
              % (bps, R, R / N, 8.0 * data.numel() / nbin, 8.0 * data.numel() / (rows * R), met,
                 offset.double().mean().item(), int(offset.max().item())))
        T = codec.clip_bits_for_bitrate(bps, F, C)
        codes, sf, offset, row_bits, clip_bits = psy.quantize_to_clip_budget(X, thr, T)
        data, _ = psy.pack(codes, sf)
        assert 8 * data.numel() == int(clip_bits.sum().item())
        print("%6d bit/s, one budget per clip: %d bits/clip (%.3f bits per sample)  packed %.3f bits per sample  "
              "budget used %.4f (least %.4f)  clips met %.4f  offset mean %.2f max %d"
              % (bps, T, T / (F * C * N), 8.0 * data.numel() / nbin, clip_bits.sum().item() / (B * T),
                 clip_bits.min().item() / T, (clip_bits <= T).double().mean().item(), offset.double().mean().item(),
                 int(offset.max().item())))


if __name__ == "__main__":
    main()
