"""Quantiser at the bench workload (B = 256 clips, stereo, K = 468 blocks, filters_n 1024): quantize, the fused synthesis
from codes (float32 and 16-bit PCM out) and decode() -- all allocating their results -- on the same process's tensors, timed
with HIP events; decode_into() (a caller-owned output) for reference.  The quantising encode in its two forms -- encode() +
quantize() (AC_ENCODE_QUANT_NOFUSE=1, two launches) and the one launch of k_fwd_fast_q -- beside encode(): bytes = PCM in +
codes + sf out; then the two forms alternating over --rounds rounds, with the spread of the rounds.  Likewise at a row budget
(--row-bits): encode_quantized_budget() -- encode() + k_quantize_budget, two launches -- against
encode_quantized() of the codec with_row_budget(), the one launch of k_fwd_fast_qb.
--pcm16 (this section alone): encode_quantized on int16 PCM, plain and at the row budget -- the one launch of k_fwd_fast_q16 /
qb16, the two launches it replaces (AC_ENCODE_QUANT_NOFUSE=1: encode(int16) + the quantiser) and the float32 one launch on a
resident float32 tensor of the same samples, compared bit for bit, then alternating over --rounds rounds of --round-steps
(profiles/quant/quant_bench_pcm16.txt).
python tools/quant_bench.py [--clips 256] [--blocks 468] [--filters 1024] [--steps 50] [--warmup 5] [--rounds 7] [--row-bits 1365]
                            [--pcm16 [--round-steps 30]]"""
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


def pcm16_rows(a):
    B, K, N, C = a.clips, a.blocks, a.filters, a.channels
    plain = audiocodec_amd.AudioCodec(48000, N)
    x = (torch.rand((B, K * N, C), device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
    p = torch.round(x * 32767).to(torch.int16)
    x = p.to(torch.float32) / 32768
    print("quant_bench --pcm16: B=%d K=%d N=%d C=%d  %s" % (B, K, N, C, torch.cuda.get_device_name()))
    for label, codec in (("encode_quantized", plain), ("encode_quantized at %d bits" % a.row_bits, plain.with_row_budget(a.row_bits))):
        def two_launches():
            os.environ["AC_ENCODE_QUANT_NOFUSE"] = "1"   # (read per call)
            try:
                return codec.encode_quantized(p)
            finally:
                del os.environ["AC_ENCODE_QUANT_NOFUSE"]

        one, two, flt = codec.encode_quantized(p), two_launches(), codec.encode_quantized(x)
        assert all(torch.equal(g, r) for g, r in zip(one, two)) and all(torch.equal(g, r) for g, r in zip(one, flt)), "the forms differ"
        del one, two, flt
        forms = [("int16, %d launch" % codec.encode_quantized_launches(C, pcm16=True), lambda: codec.encode_quantized(p)),
                 ("int16, two launches (encode + quantiser)", two_launches),
                 ("float32 resident, %d launch" % codec.encode_quantized_launches(C), lambda: codec.encode_quantized(x))]
        print("%s: the three forms agree bit for bit" % label)
        runs = dict((n, []) for n, _ in forms)
        for _ in range(a.rounds):
            for n, fn in forms:
                runs[n].append(timed(fn, a.round_steps, 1))
        med = []
        for n, _ in forms:
            v = sorted(runs[n])
            med.append(v[len(v) // 2])
            print("  %-44s median %.3f ms  min %.3f  max %.3f  (%d alternating rounds of %d)" % (n, med[-1], v[0], v[-1], len(v), a.round_steps))
        print("  one launch / two launches = %.3f   int16 / float32 = %.3f" % (med[0] / med[1], med[0] / med[2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pcm16", action="store_true", help="only the int16 section")
    ap.add_argument("--round-steps", type=int, default=30)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=468)
    ap.add_argument("--filters", type=int, default=1024)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--row-bits", type=int, default=1365)
    a = ap.parse_args()
    if a.pcm16:
        return pcm16_rows(a)
    B, K, N, C = a.clips, a.blocks, a.filters, a.channels
    codec = audiocodec_amd.AudioCodec(48000, N)
    M = codec.psy.bark_bands_n
    cbr = codec.with_row_budget(a.row_bits)
    x = (torch.rand((B, K * N, C), device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
    X, _, thr = codec.encode(x)
    codes, sf = codec.psy.quantize(X, thr)
    F = K + 1
    nbin = B * F * N * C
    pcm_f32, pcm_i16 = B * (F + 1) * N * C * 4, B * (F + 1) * N * C * 2
    code_b, sf_b = nbin * 2, B * F * M * C
    out_f = torch.empty((B, (F + 1) * N, C), dtype=torch.float32, device="cuda")
    print("quant_bench: B=%d K=%d N=%d C=%d M=%d  decode_quantized launches=%d  %s"
          % (B, K, N, C, M, codec.decode_quantized_launches(C), torch.cuda.get_device_name()))
    enc_b = B * K * N * C * 4 + code_b + sf_b

    def two_launches():
        os.environ["AC_ENCODE_QUANT_NOFUSE"] = "1"   # (read per call)
        try:
            return codec.encode_quantized(x)
        finally:
            del os.environ["AC_ENCODE_QUANT_NOFUSE"]

    rows = [
        ("encode", lambda: codec.encode(x), enc_b),
        ("encode + quantize (two launches)", two_launches, enc_b),
        ("encode_quantized (one launch)", lambda: codec.encode_quantized(x), enc_b),
        ("encode_quantized_budget (two launches)", lambda: codec.encode_quantized_budget(x, a.row_bits), enc_b),
        ("cbr.encode_quantized (%d launch)" % cbr.encode_quantized_launches(C), lambda: cbr.encode_quantized(x), enc_b),
        ("quantize", lambda: codec.psy.quantize(X, thr), nbin * 8 + code_b + sf_b),
        ("decode_quantized f32", lambda: codec.decode_quantized(codes, sf), code_b + sf_b + pcm_f32),
        ("decode_quantized pcm16", lambda: codec.decode_quantized(codes, sf, pcm16=True), code_b + sf_b + pcm_i16),
        ("decode f32", lambda: codec.decode(X), nbin * 4 + pcm_f32),
        ("decode_into f32", lambda: codec.decode_into(X, out_f), nbin * 4 + pcm_f32),
        ("dequantize", lambda: codec.psy.dequantize(codes, sf), code_b + sf_b + nbin * 4),
    ]
    res = {}
    for name, fn, nbytes in rows:
        ms = timed(fn, a.steps, a.warmup)
        res[name] = ms
        print("%-40s %8.3f ms  %6.3f GB  %6.2f TB/s" % (name, ms, nbytes / 1e9, nbytes / ms / 1e9))
    print("decode_quantized f32 / decode f32 = %.3f" % (res["decode_quantized f32"] / res["decode f32"]))
    if a.rounds < 1:
        return
    # the two forms of the quantising encode and encode(), alternating in this process
    names = ("encode", "encode + quantize (two launches)", "encode_quantized (one launch)")
    fns = dict((n, f) for n, f, _ in rows[:5])

    def alternate(names):
        runs = dict((n, []) for n in names)
        for _ in range(a.rounds):
            for n in names:
                runs[n].append(timed(fns[n], a.steps, 1))
        med = {}
        for n in names:
            v = sorted(runs[n])
            med[n] = v[len(v) // 2]
            print("%-40s median %.3f ms  min %.3f  max %.3f  (%d alternating rounds of %d)" % (n, med[n], v[0], v[-1], len(v), a.steps))
        return med

    med = alternate(names)
    print("one launch / two launches = %.3f   one launch / encode = %.3f"
          % (med[names[2]] / med[names[1]], med[names[2]] / med[names[0]]))
    # ... and the two forms of the encode at a row budget
    names = tuple(n for n, _, _ in rows[3:5])
    med = alternate(names)
    print("row budget %d: cbr.encode_quantized / encode_quantized_budget = %.3f" % (a.row_bits, med[names[1]] / med[names[0]]))


if __name__ == "__main__":
    main()
