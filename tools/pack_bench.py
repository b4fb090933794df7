"""Packed bitstream at the bench workload (B = 256 clips, stereo, K = 468 blocks, filters_n 1024, uniform input in [-1, 1]):
pack_index + pack (the C ABI on caller-owned buffers, and psy.pack() with its read of the byte count), unpack, and
decode_packed against decode_quantized, timed with HIP events.  Algorithmic bytes: codes + sf + packed bytes, each once (pack_index alone:
codes + sf + the index; a decoder: its input + the PCM it writes).  Then decode_packed in its two forms -- the one launch of
k_inv_fast_p and unpack + decode_quantized (AC_DECODE_PACKED_NOFUSE=1, read per call) -- and decode_quantized, float32 and
16-bit PCM out, alternating over --rounds rounds of --round-steps calls with the spread of the rounds; the two forms'
outputs are compared bit for bit first.  Last, at a row budget: encode_packed, encode_packed_rows in its two forms (the one
launch of k_fwd_fast_qp; AC_ENCODE_PACKED_NOFUSE=1: the composition) and encode_quantized, alternating the same way
(packed_rows(); --only-rows runs this section alone).
--stream: packed rows chunk by chunk on a StreamingMDCT (stream_rows()): the chain of public calls a caller had before the
chunk methods existed -- encode_chunk, quantize_to_budget, the mask, ac_pack; unpack, dequantize, inverse_chunk -- against
encode_packed_rows_chunk / decode_packed_chunk where the package has them, so the same script times the baseline on an older
commit.  Two workloads: one stereo clip in chunks of 256 blocks (per-chunk latency) and --clips x --blocks as one chunk.
--pcm16: int16 PCM to packed rows (pcm16_rows()), one-shot at the bench workload and one stereo clip in chunks of 256 blocks:
the one launch on int16 (k_fwd_fast_qp16 / qps16), the conversion to(float32) / 32768 followed by the float32 one launch (what a
caller did before), and the float32 one launch on a resident float32 tensor; compared byte for byte, then alternating
(profiles/pack/pack_bench_pcm16.txt).
python tools/pack_bench.py [--clips 256] [--blocks 468] [--filters 1024] [--steps 50] [--warmup 5] [--rounds 7] [--round-steps 30]
                           [--row-bits 1365] [--only-rows] [--stream] [--pcm16] [--transrate [--targets 1365 682]] [--conceal] [--conceal-stream] [--protect] [--mix] [--route] [--level]
--transrate: rows at 2730 bits transrated to each of --targets (transrate_rows(); profiles/pack/pack_bench_transrate.txt).
--conceal: decode_packed with lost rows concealed -- none lost, and 1 % lost at random -- against decode_packed without `lost`
(conceal_rows(); profiles/pack/pack_bench_conceal.txt).
--conceal-stream: the same chunk by chunk on a StreamingMDCT, the last good row carried across chunks, against
decode_packed_chunk without `lost` (conceal_stream_rows(); profiles/pack/pack_bench_conceal_stream.txt).
--protect [--red-bits 341]: protect_packed_rows against its composition and transrate_packed_rows alone, then decode_packed with
redundant_at against without (protect_rows(); profiles/pack/pack_bench_protect.txt).
--protect-stream [--red-bits 341]: decode_packed_chunk with redundant_at chunk by chunk on a StreamingMDCT, against the concealing
chunk on the same `lost` and against its composition; then protect_chunk against the one-shot protect_packed_rows on the same rows
and against its composition (protect_stream_rows(); profiles/pack/pack_bench_protect_stream.txt).
--mix [--sources 2 4]: mix_packed_rows of S sources at 2730 bits to 1365 in its one launch, against its composition, the decode
route (S decode_packed, the adds, encode_packed_rows) and transrate_packed_rows of one source (mix_rows();
profiles/pack/pack_bench_mix.txt).
--route [--sources 2 3 4 8]: route_packed_rows as mix-minus of S = O parties at 2730 bits to 1365 in its one launch, against O calls
of mix_packed_rows and the decode route (S decode_packed, the adds, O encode_packed_rows) (route_rows();
profiles/pack/pack_bench_route.txt).
--level: packed_rows_level in its one launch against its composition, the decode route (decode_packed and a per-block energy pass)
and transrate_packed_rows of the same rows; select_loudest at S = 4 and 8; a bridge of four with everyone routed against levels +
select_loudest(n = 2) + route_packed_rows (level_rows(); profiles/pack/pack_bench_level.txt)."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audiocodec_amd  # noqa: E402
from audiocodec_amd import _lib  # noqa: E402


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


def packed_rows(a):
    """encode_packed_rows at a bitrate ("packed rows"): (a) encode_packed, dense, with its host read;
    (b) the composition of encode_packed_rows (AC_ENCODE_PACKED_NOFUSE=1, read per call); (c) its one launch; (d)
    encode_quantized -- k_fwd_fast_qb alone -- as the floor.  Alternating in this process, --rounds rounds of --round-steps."""
    B, K, N, C = a.clips, a.blocks, a.filters, a.channels
    cbr = audiocodec_amd.AudioCodec(48000, N).with_row_budget(a.row_bits)
    x = (torch.rand((B, K * N, C), device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
    rows, rb = B * (K + 1) * C, cbr.row_bytes

    def composition():
        os.environ["AC_ENCODE_PACKED_NOFUSE"] = "1"   # (read per call)
        try:
            return cbr.encode_packed_rows(x)
        finally:
            del os.environ["AC_ENCODE_PACKED_NOFUSE"]

    one, two = cbr.encode_packed_rows(x), composition()
    assert all(torch.equal(g, r) for g, r in zip(one, two)), "the two forms differ"
    dense = cbr.encode_packed(x)[0].numel()
    print("packed rows: B=%d K=%d N=%d C=%d  %d bits per row, row_bytes %d  launches=%d  rows=%d (%d do not fit)  data %.1f MB "
          "(dense %.1f MB)  the one launch and the composition agree byte for byte"
          % (B, K, N, C, a.row_bits, rb, cbr.encode_packed_rows_launches(C), rows, int((~one[2]).sum()), rows * rb / 1e6,
             dense / 1e6))
    del one, two
    forms = [("(a) encode_packed (dense, host read)", lambda: cbr.encode_packed(x)),
             ("(b) encode_packed_rows, composition", composition),
             ("(c) encode_packed_rows, %d launch" % cbr.encode_packed_rows_launches(C), lambda: cbr.encode_packed_rows(x)),
             ("(d) encode_quantized (k_fwd_fast_qb)", lambda: cbr.encode_quantized(x))]
    runs = dict((n, []) for n, _ in forms)
    for _ in range(a.rounds):
        for n, fn in forms:
            runs[n].append(timed(fn, a.round_steps, 1))
    med = []
    for n, _ in forms:
        v = sorted(runs[n])
        med.append(v[len(v) // 2])
        print("%-40s median %.3f ms  min %.3f  max %.3f  (%d alternating rounds of %d)" % (n, med[-1], v[0], v[-1], len(v), a.round_steps))
    print("(c) / (b) = %.3f   (c) / (a) = %.3f   (c) / (d) = %.3f" % (med[2] / med[1], med[2] / med[0], med[2] / med[3]))


def stream_rows(a):
    """Packed rows in a stream: per workload the chain of older public calls and, where the package has
    them, the chunk methods; forms alternating, --rounds rounds of --round-steps passes over the workload's chunks."""
    N, C, lib = a.filters, a.channels, _lib.load()
    cbr = audiocodec_amd.AudioCodec(48000, N).with_row_budget(a.row_bits)
    rb, psy = (a.row_bits + 31) // 32 * 4, cbr.psy
    kmin = psy.row_budget[1]
    new = hasattr(audiocodec_amd.codec.StreamingMDCT, "encode_packed_rows_chunk")
    for name, B, k, n in (("one clip, chunks of 256 blocks", 1, 256, 8), ("%d clips x %d blocks, one chunk" % (a.clips, a.blocks), a.clips, a.blocks, 1)):
        g = torch.Generator("cuda").manual_seed(1)
        chunks = [torch.rand((B, k * N, C), device="cuda", generator=g) * 2 - 1 for _ in range(n)]
        enc, dec = cbr.stream(B, C), cbr.stream(B, C)
        index = (torch.arange(B * k * C, dtype=torch.int64, device="cuda") * rb).view(B, k, C)
        plan = psy._plan(index.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

        def chain_enc(x):
            X, _, thr = enc.encode_chunk(x)
            codes, sf, _, bits = psy.quantize_to_budget(X, thr, a.row_bits, kmin)
            fits = bits <= 8 * rb
            sf.masked_fill_(~fits.unsqueeze(2), -128)
            data = torch.zeros((B * k * C * rb,), dtype=torch.uint8, device=x.device)
            _lib.check(lib.ac_pack(plan, p(codes), p(sf), p(index), p(data), B, k, C,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            return data, fits

        def chain_dec(data):
            return dec.inverse_chunk(psy.dequantize(*psy.unpack(data, index)))

        def chain_dec16(data):
            return torch.nan_to_num(chain_dec(data) * 32768.0, nan=0.0).round_().clamp_(-32768.0, 32767.0).to(torch.int16)

        packed = [chain_enc(x)[0] for x in chunks]
        forms = [("encode: encode_chunk + quantize_to_budget + mask + ac_pack", lambda: [chain_enc(x) for x in chunks]),
                 ("decode f32: unpack + dequantize + inverse_chunk", lambda: [chain_dec(d) for d in packed]),
                 ("decode pcm16: the same + the 16-bit store in torch", lambda: [chain_dec16(d) for d in packed])]
        launches = ""
        if new:
            enc.reset()
            for x, d in zip(chunks, packed):
                assert torch.equal(enc.encode_packed_rows_chunk(x)[0], d), "the chunk method and the chain differ"
            dec.reset()
            want = [chain_dec(d) for d in packed]
            want16 = [torch.nan_to_num(w * 32768.0, nan=0.0).round_().clamp_(-32768.0, 32767.0).to(torch.int16) for w in want]
            for pcm16, ws in ((False, want), (True, want16)):
                dec.reset()
                for d, w in zip(packed, ws):
                    got = dec.decode_packed_chunk(d, index, pcm16=pcm16)
                    assert got.dtype == w.dtype and torch.equal(got.view(torch.int16), w.view(torch.int16)), \
                        "decode_packed_chunk and the chain differ (pcm16=%s)" % pcm16
            del want, want16
            forms += [("encode: encode_packed_rows_chunk", lambda: [enc.encode_packed_rows_chunk(x) for x in chunks]),
                      ("decode f32: decode_packed_chunk", lambda: [dec.decode_packed_chunk(d, index) for d in packed]),
                      ("decode pcm16: decode_packed_chunk", lambda: [dec.decode_packed_chunk(d, index, pcm16=True) for d in packed])]
            launches = ("  launches: encode %d, decode %d; the chunk methods and the chain agree bit for bit (rows; float32 and 16-bit PCM)"
                        % (enc.packed_chunk_launches(), dec.packed_chunk_launches(decode=True)))
        print("stream rows: %s  (B=%d k=%d N=%d C=%d, %d chunks per pass, %d bits per row)%s"
              % (name, B, k, N, C, n, a.row_bits, launches))
        runs = dict((f, []) for f, _ in forms)
        for _ in range(a.rounds):
            for f, fn in forms:
                runs[f].append(timed(fn, a.round_steps, 1) / n * 1e3)
        for f, _ in forms:
            v = sorted(runs[f])
            print("  %-60s median %9.1f us per chunk  min %9.1f  max %9.1f  (%d alternating rounds of %d)"
                  % (f, v[len(v) // 2], v[0], v[-1], len(v), a.round_steps))


def pcm16_rows(a):
    B, K, N, C = a.clips, a.blocks, a.filters, a.channels
    cbr = audiocodec_amd.AudioCodec(48000, N).with_row_budget(a.row_bits)

    def alternate(forms, unit, scale):
        runs = dict((n, []) for n, _ in forms)
        for _ in range(a.rounds):
            for n, fn in forms:
                runs[n].append(timed(fn, a.round_steps, 1) * scale)
        med = []
        for n, _ in forms:
            v = sorted(runs[n])
            med.append(v[len(v) // 2])
            print("  %-50s median %9.3f %s  min %9.3f  max %9.3f  (%d alternating rounds of %d)"
                  % (n, med[-1], unit, v[0], v[-1], len(v), a.round_steps))
        print("  int16 / (convert + float32) = %.3f   int16 / float32 resident = %.3f" % (med[0] / med[1], med[0] / med[2]))

    x = (torch.rand((B, K * N, C), device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
    p = torch.round(x * 32767).to(torch.int16)
    x = p.to(torch.float32) / 32768
    one, flt = cbr.encode_packed_rows(p), cbr.encode_packed_rows(x)
    assert all(torch.equal(g, r) for g, r in zip(one, flt)), "the int16 and the float32 rows differ"
    del one, flt
    print("packed rows from int16: B=%d K=%d N=%d C=%d  %d bits per row  launches: int16 %d, float32 %d  the rows agree byte for byte  %s"
          % (B, K, N, C, a.row_bits, cbr.encode_packed_rows_launches(C, pcm16=True), cbr.encode_packed_rows_launches(C),
             torch.cuda.get_device_name()))
    alternate([("encode_packed_rows(int16)", lambda: cbr.encode_packed_rows(p)),
               ("encode_packed_rows(int16.to(float32) / 32768)", lambda: cbr.encode_packed_rows(p.to(torch.float32) / 32768)),
               ("encode_packed_rows(float32 resident)", lambda: cbr.encode_packed_rows(x))], "ms", 1.0)
    del x, p
    # one stereo clip in chunks of 256 blocks
    k, n = 256, 8
    g = torch.Generator("cuda").manual_seed(1)
    ps = [torch.round((torch.rand((1, k * N, C), device="cuda", generator=g) * 2 - 1) * 32767).to(torch.int16) for _ in range(n)]
    xs = [q.to(torch.float32) / 32768 for q in ps]
    a16, a32 = cbr.stream(1, C), cbr.stream(1, C)
    for q, xf in zip(ps, xs):
        assert torch.equal(a16.encode_packed_rows_chunk(q)[0], a32.encode_packed_rows_chunk(xf)[0]), "the int16 and the float32 chunks differ"
    print("one clip, chunks of %d blocks (%d per pass)  launches: int16 %d, float32 %d  the rows agree byte for byte"
          % (k, n, a16.packed_chunk_launches(pcm16=True), a16.packed_chunk_launches()))
    alternate([("encode_packed_rows_chunk(int16)", lambda: [a16.encode_packed_rows_chunk(q) for q in ps]),
               ("encode_packed_rows_chunk(int16.to(float32) / 32768)",
                lambda: [a16.encode_packed_rows_chunk(q.to(torch.float32) / 32768) for q in ps]),
               ("encode_packed_rows_chunk(float32 resident)", lambda: [a16.encode_packed_rows_chunk(xf) for xf in xs])],
              "us per chunk", 1e3 / n)


def transrate_rows(a):
    """Transrating: rows of encode_packed_rows at --row-bits (2730 with --transrate) to each budget of
    --targets.  (a) transrate_packed_rows in its one launch; (b) its composition (AC_TRANSRATE_NOFUSE=1, read per call);
    (c) decode_packed + encode_packed_rows at the target, what a caller did before; (d) decode_packed alone, the floor of
    reading the rows.  Compared byte for byte first, then alternating, --rounds rounds of --round-steps.  Also the share of
    rows at offset 0 and the mean offset, and on one small batch the RMS error against the spectrum X of transrated rows
    beside rows encoded at the target."""
    B, K, N, C = a.clips, a.blocks, a.filters, a.channels
    base = audiocodec_amd.AudioCodec(48000, N)
    src = base.with_row_budget(a.row_bits)
    x = (torch.rand((B, K * N, C), device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
    data, index, _ = src.encode_packed_rows(x)
    rows = index.numel()
    print("transrate: B=%d K=%d N=%d C=%d  rows=%d at %d bits (%.1f MB)  %s"
          % (B, K, N, C, rows, a.row_bits, data.numel() / 1e6, torch.cuda.get_device_name()))
    for R2 in a.targets:
        dst = base.with_row_budget(R2)

        def composition():
            os.environ["AC_TRANSRATE_NOFUSE"] = "1"   # (read per call)
            try:
                return dst.transrate_packed_rows(data, index, True)
            finally:
                del os.environ["AC_TRANSRATE_NOFUSE"]

        def recode():
            return dst.encode_packed_rows(dst.decode_packed(data, index))   # (the decoded signal as it comes: K + 2 blocks)

        one, two = dst.transrate_packed_rows(data, index, True), composition()
        assert all(torch.equal(g, r) for g, r in zip(one, two)), "the two forms differ"
        off = one[3].to(torch.float32)
        print("-> %d bits per row, row_bytes %d (%.1f MB)  launches=%d  %d rows do not fit  offset 0: %.1f %% of the rows  mean "
              "offset %.2f  max %d  the one launch and the composition agree byte for byte"
              % (R2, dst.row_bytes, rows * dst.row_bytes / 1e6, dst.transrate_packed_rows_launches(C), int((~one[2]).sum()),
                 100.0 * float((off == 0).float().mean()), float(off.mean()), int(off.max())))
        del one, two, off
        forms = [("(a) transrate_packed_rows, %d launch" % dst.transrate_packed_rows_launches(C),
                  lambda: dst.transrate_packed_rows(data, index)),
                 ("(b) transrate_packed_rows, composition", composition),
                 ("(c) decode_packed + encode_packed_rows", recode),
                 ("(d) decode_packed alone", lambda: dst.decode_packed(data, index))]
        runs = dict((n, []) for n, _ in forms)
        for _ in range(a.rounds):
            for n, fn in forms:
                runs[n].append(timed(fn, a.round_steps, 1))
        med = []
        for n, _ in forms:
            v = sorted(runs[n])
            med.append(v[len(v) // 2])
            print("  %-42s median %.3f ms  min %.3f  max %.3f  (%d alternating rounds of %d)" % (n, med[-1], v[0], v[-1], len(v), a.round_steps))
        print("  (a) / (b) = %.3f   (a) / (c) = %.3f   (a) / (d) = %.3f" % (med[0] / med[1], med[0] / med[2], med[0] / med[3]))
    # an observation, not a criterion: the error of transrated rows against the spectrum beside rows encoded at the target
    xs = x[:4, :16 * N].contiguous()
    del x, data, index
    X = base.encode(xs)[0]
    d0, i0, _ = src.encode_packed_rows(xs)
    for R2 in a.targets:
        dst = base.with_row_budget(R2)
        td, ti, tf = dst.transrate_packed_rows(d0, i0)
        ed, ei, ef = dst.encode_packed_rows(xs)
        ok = (tf & ef).unsqueeze(2)
        err = []
        for dd, ii in ((td, ti), (ed, ei)):
            Xh = base.psy.dequantize(*base.psy.unpack(dd, ii))
            e = torch.where(ok, (Xh - X).double() ** 2, torch.zeros((), dtype=torch.float64, device=X.device))
            err.append(float((e.sum() / (ok.sum() * N)).sqrt()))
        print("RMS error against X at %d bits (4 clips x 16 blocks, rows that fit in both): transrated from %d %.4f, encoded "
              "directly %.4f" % (R2, a.row_bits, err[0], err[1]))


def protect_rows(a):
    """Protected rows and the recovering decode: rows of encode_packed_rows at 2730 bits, R = 1365 and
    R2 = --red-bits (341).  Protect: (a) protect_packed_rows in its one launch (k_protect_p); (b) its composition
    (AC_PROTECT_NOFUSE=1, read per call); (c) transrate_packed_rows alone at R, the floor.  Recover, on the protected slots,
    against decode_packed(lost=) without redundant_at (k_inv_fast_pl) on the same `lost`: nothing lost, 1 % lost (most lost
    rows are recovered), and the composition (AC_DECODE_PACKED_NOFUSE=1).  Compared byte for byte first, then alternating,
    --rounds rounds of --round-steps."""
    B, K, N, C = a.clips, a.blocks, a.filters, a.channels
    base = audiocodec_amd.AudioCodec(48000, N)
    src, dst, R2 = base.with_row_budget(2730), base.with_row_budget(1365), a.red_bits
    x = (torch.rand((B, K * N, C), device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
    data, index, _ = src.encode_packed_rows(x)
    del x
    print("protect: B=%d K=%d N=%d C=%d  rows=%d at 2730 bits (%.1f MB) -> R 1365, R2 %d, slot_bytes %d (%.1f MB)  launches=%d  %s"
          % (B, K, N, C, index.numel(), data.numel() / 1e6, R2, dst.protected_slot_bytes(R2),
             index.numel() * dst.protected_slot_bytes(R2) / 1e6, dst.protect_packed_rows_launches(C, red_bits=R2),
             torch.cuda.get_device_name()))

    def nofuse(name, fn):
        os.environ[name] = "1"   # (read per call)
        try:
            return fn()
        finally:
            del os.environ[name]

    def report(forms, ratios):
        runs = dict((n, []) for n, _ in forms)
        for _ in range(a.rounds):
            for n, fn in forms:
                runs[n].append(timed(fn, a.round_steps, 1))
        med = []
        for n, _ in forms:
            v = sorted(runs[n])
            med.append(v[len(v) // 2])
            print("  %-44s median %.3f ms  min %.3f  max %.3f  (%d alternating rounds of %d)" % (n, med[-1], v[0], v[-1], len(v), a.round_steps))
        print("  " + "   ".join("%s = %.3f" % (t, med[i] / med[j]) for t, i, j in ratios))

    one = dst.protect_packed_rows(data, index, R2, True)
    two = nofuse("AC_PROTECT_NOFUSE", lambda: dst.protect_packed_rows(data, index, R2, True))
    assert all(torch.equal(g, r) for g, r in zip(one, two)), "the two forms of protect differ"
    print("the one launch and the composition agree byte for byte; %d primary and %d redundant parts do not fit; mean offset %.2f, "
          "mean redundant offset %.2f" % (int((~one[2]).sum()), int((~one[3]).sum()), float(one[4].float().mean()), float(one[5].float().mean())))
    slots, sidx = one[0], one[1]
    del one, two
    report([("(a) protect_packed_rows, %d launch" % dst.protect_packed_rows_launches(C, red_bits=R2),
             lambda: dst.protect_packed_rows(data, index, R2)),
            ("(b) protect_packed_rows, composition", lambda: nofuse("AC_PROTECT_NOFUSE", lambda: dst.protect_packed_rows(data, index, R2))),
            ("(c) transrate_packed_rows alone at R", lambda: dst.transrate_packed_rows(data, index))],
           [("(a) / (b)", 0, 1), ("(a) / (c)", 0, 2)])
    del data, index
    o = dst.row_bytes
    none = torch.zeros(sidx.shape, dtype=torch.uint8, device="cuda")
    some = (torch.rand(sidx.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) < 0.01).to(torch.uint8)
    rec = int(((some[:, :-1] != 0) & (some[:, 1:] == 0)).sum())
    print("recover: %d rows lost (%.2f %%), %d of them recovered  max_age 8  redundant_at %d" % (int(some.sum()), 100.0 * float(some.float().mean()), rec, o))
    v = torch.int16
    for pcm16 in (False, True):
        plain = dst.decode_packed(slots, sidx, pcm16)
        assert torch.equal(dst.decode_packed(slots, sidx, pcm16, lost=none, redundant_at=o).view(v), plain.view(v)), "none lost != the plain decode"
        got = dst.decode_packed(slots, sidx, pcm16, lost=some, max_age=8, redundant_at=o)
        ref = nofuse("AC_DECODE_PACKED_NOFUSE", lambda: dst.decode_packed(slots, sidx, pcm16, lost=some, max_age=8, redundant_at=o))
        assert got.dtype == ref.dtype and torch.equal(got.view(v), ref.view(v)), "the two forms of the recovering decode differ"
        del plain, got, ref
    print("none lost equals the plain decode; the one launch and the composition agree bit for bit (float32 and 16-bit PCM)")
    for pcm16 in (False, True):
        print("%s out:" % ("16-bit PCM" if pcm16 else "float32"))
        report([("(a) lost all false, k_inv_fast_pl", lambda: dst.decode_packed(slots, sidx, pcm16, lost=none)),
                ("(b) lost all false, redundant_at", lambda: dst.decode_packed(slots, sidx, pcm16, lost=none, redundant_at=o)),
                ("(c) 1 % lost, k_inv_fast_pl", lambda: dst.decode_packed(slots, sidx, pcm16, lost=some)),
                ("(d) 1 % lost, redundant_at", lambda: dst.decode_packed(slots, sidx, pcm16, lost=some, redundant_at=o)),
                ("(e) 1 % lost, redundant_at, composition",
                 lambda: nofuse("AC_DECODE_PACKED_NOFUSE", lambda: dst.decode_packed(slots, sidx, pcm16, lost=some, redundant_at=o)))],
               [("(b) / (a)", 1, 0), ("(d) / (c)", 3, 2), ("(d) / (e)", 3, 4)])


def mix_rows(a):
    """Mixing: --sources S sources (2 and 4) of encode_packed_rows at 2730 bits, mixed to 1365.  (a)
    mix_packed_rows in its one launch (k_mix_p); (b) its composition (AC_MIX_NOFUSE=1, read per call); (c) the decode route:
    S decode_packed, the adds, encode_packed_rows; (d) transrate_packed_rows of one source alone, the S = 1 floor.  The two
    forms are compared byte for byte first, then all alternate, --rounds rounds of --round-steps."""
    B, K, N, C = a.clips, a.blocks, a.filters, a.channels
    base = audiocodec_amd.AudioCodec(48000, N)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    gen = torch.Generator("cuda").manual_seed(0)
    all_sources = []
    for _ in range(max(a.sources)):
        x = torch.rand((B, K * N, C), device="cuda", generator=gen) * 2 - 1
        all_sources.append(src.encode_packed_rows(x)[:2])
        del x
    rows = all_sources[0][1].numel()
    print("mix: B=%d K=%d N=%d C=%d  rows=%d per source at 2730 bits (%.1f MB each) -> 1365 bits (%.1f MB)  %s"
          % (B, K, N, C, rows, all_sources[0][0].numel() / 1e6, rows * dst.row_bytes / 1e6, torch.cuda.get_device_name()))

    def composition(sources, offset=False):
        os.environ["AC_MIX_NOFUSE"] = "1"   # (read per call)
        try:
            return dst.mix_packed_rows(sources, None, None, offset)
        finally:
            del os.environ["AC_MIX_NOFUSE"]

    def decode_route(sources):
        pcm = dst.decode_packed(*sources[0])
        for d, i in sources[1:]:
            pcm = pcm + dst.decode_packed(d, i)
        return dst.encode_packed_rows(pcm[:, N:-N].contiguous())   # (K + 1 frames decode to K + 2 blocks: the K in the middle)

    for S in a.sources:
        sources = all_sources[:S]
        one, two = dst.mix_packed_rows(sources, None, None, True), composition(sources, True)
        assert all(torch.equal(g, r) for g, r in zip(one, two)), "the two forms differ"
        print("S = %d: launches %d (composition %d); the one launch and the composition agree byte for byte; %d rows do not fit; "
              "%.1f %% of the rows at offset 0, mean offset %.2f" % (S, dst.mix_packed_rows_launches(C, sources_n=S), 2 * S + 2,
                                                                    int((~one[2]).sum()), 100.0 * float((one[3] == 0).float().mean()), float(one[3].float().mean())))
        del one, two
        forms = [("(a) mix_packed_rows, %d launch" % dst.mix_packed_rows_launches(C, sources_n=S), lambda: dst.mix_packed_rows(sources)),
                 ("(b) mix_packed_rows, composition", lambda: composition(sources)),
                 ("(c) %d decode_packed + adds + encode_packed_rows" % S, lambda: decode_route(sources)),
                 ("(d) transrate_packed_rows of one source", lambda: dst.transrate_packed_rows(*sources[0]))]
        runs = dict((n, []) for n, _ in forms)
        for _ in range(a.rounds):
            for n, fn in forms:
                runs[n].append(timed(fn, a.round_steps, 1))
        med = []
        for n, _ in forms:
            v = sorted(runs[n])
            med.append(v[len(v) // 2])
            print("  %-52s median %.3f ms  min %.3f  max %.3f  (%d alternating rounds of %d)" % (n, med[-1], v[0], v[-1], len(v), a.round_steps))
        read = S * all_sources[0][0].numel() + rows * dst.row_bytes
        print("  (a) / (b) = %.3f   (a) / (c) = %.3f   (a) / (d) = %.3f   per added source: %.3f of one transrate   (a) moves %.1f MB: %.0f GB/s"
              % (med[0] / med[1], med[0] / med[2], med[0] / med[3], (med[0] - med[3]) / max(S - 1, 1) / med[3], read / 1e6, read / med[0] / 1e6))


def route_rows(a):
    """Routing: mix-minus of S = O parties (--sources, default 2 3 4 8), independent noise per source,
    encode_packed_rows at 2730 bits routed to 1365.  (a) route_packed_rows in its one launch (k_route_p); (b) O calls of
    mix_packed_rows, each one launch of k_mix_p; (c) what a bridge did before mixing: S decode_packed, the adds, O
    encode_packed_rows.  (a) and (b) are compared byte for byte first, then all alternate, --rounds rounds of --round-steps."""
    B, K, N, C = a.clips, a.blocks, a.filters, a.channels
    base = audiocodec_amd.AudioCodec(48000, N)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    gen = torch.Generator("cuda").manual_seed(0)
    counts = a.sources if a.sources != [2, 4] else [2, 3, 4, 8]
    all_sources = []
    for _ in range(max(counts)):
        x = torch.rand((B, K * N, C), device="cuda", generator=gen) * 2 - 1
        all_sources.append(src.encode_packed_rows(x)[:2])
        del x
    rows = all_sources[0][1].numel()
    print("route: B=%d K=%d N=%d C=%d  rows=%d per source at 2730 bits (%.1f MB each) -> 1365 bits (%.1f MB per output)  %s"
          % (B, K, N, C, rows, all_sources[0][0].numel() / 1e6, rows * dst.row_bytes / 1e6, torch.cuda.get_device_name()))

    def mixes(sources, routes, offset=False):
        return [dst.mix_packed_rows([sources[i] for i, g in enumerate(r) if g is not None], [g for g in r if g is not None], None, offset)
                for r in routes]

    def decode_route(sources):
        pcm = [dst.decode_packed(d, i) for d, i in sources]
        total = pcm[0]
        for p in pcm[1:]:
            total = total + p
        return [dst.encode_packed_rows((total - p)[:, N:-N].contiguous()) for p in pcm]

    for S in counts:
        sources, routes = all_sources[:S], dst.mix_minus_routes(S)
        launches = dst.route_packed_rows_launches(C, sources_n=S, outputs_n=S)
        one, two = dst.route_packed_rows(sources, routes, None, True), mixes(sources, routes, True)
        for o in range(S):
            assert torch.equal(one[0][o], two[o][0]) and torch.equal(one[2][o], two[o][2]) and torch.equal(one[3][o], two[o][3]), "the two forms differ"
        print("S = O = %d: launches %d (%d mix_packed_rows: %d); the one launch and the mixes agree byte for byte; %d rows do not fit; "
              "mean offset %.2f" % (S, launches, S, S * dst.mix_packed_rows_launches(C, sources_n=max(S - 1, 1)), int((~one[2]).sum()),
                                    float(one[3].float().mean())))
        del one, two
        forms = [("(a) route_packed_rows, %d launch" % launches, lambda: dst.route_packed_rows(sources, routes)),
                 ("(b) %d mix_packed_rows of %d sources" % (S, S - 1), lambda: mixes(sources, routes)),
                 ("(c) %d decode_packed + adds + %d encode_packed_rows" % (S, S), lambda: decode_route(sources))]
        runs = dict((n, []) for n, _ in forms)
        for _ in range(a.rounds):
            for n, fn in forms:
                runs[n].append(timed(fn, a.round_steps, 1))
        med, spread = [], []
        for n, _ in forms:
            v = sorted(runs[n])
            med.append(v[len(v) // 2])
            spread.append(v[-1] - v[0])
            print("  %-52s median %.3f ms  min %.3f  max %.3f  (%d alternating rounds of %d)" % (n, med[-1], v[0], v[-1], len(v), a.round_steps))
        moved_a = S * all_sources[0][0].numel() + S * rows * dst.row_bytes
        moved_b = S * (S - 1) * all_sources[0][0].numel() + S * rows * dst.row_bytes
        print("  (a) / (b) = %.3f   (a) / (c) = %.3f   (b) - (a) = %.3f ms against a spread of %.3f   per output: (a) %.3f ms, (b) %.3f ms   "
              "(a) moves %.1f MB: %.0f GB/s, (b) %.1f MB"
              % (med[0] / med[1], med[0] / med[2], med[1] - med[0], max(spread[0], spread[1]), med[0] / S, med[1] / S, moved_a / 1e6,
                 moved_a / med[0] / 1e6, moved_b / 1e6))


def level_rows(a):
    """Levels and the selector on sources of encode_packed_rows at 2730 bits.  (a) packed_rows_level in
    its one launch (k_level_p); (b) its composition (AC_LEVEL_NOFUSE=1, read per call); (c) what a caller did before:
    decode_packed and a per-block energy pass over the PCM; (d) transrate_packed_rows of the same rows to 1365 bits, the
    parse-search-pack yardstick; (e) select_loudest at S = 4 and S = 8 on those levels; (f) a bridge of four, mix-minus to 1365
    bits: everyone routed, against levels + select_loudest(n = 2) + route_packed_rows(active=).  (a) and (b) are compared bit
    for bit first, then all alternate, --rounds rounds of --round-steps."""
    B, K, N, C = a.clips, a.blocks, a.filters, a.channels
    base = audiocodec_amd.AudioCodec(48000, N)
    src, dst = base.with_row_budget(2730), base.with_row_budget(1365)
    gen = torch.Generator("cuda").manual_seed(0)
    sources = []
    for _ in range(4):
        x = torch.rand((B, K * N, C), device="cuda", generator=gen) * 2 - 1
        sources.append(src.encode_packed_rows(x)[:2])
        del x
    data, index = sources[0]
    rows = index.numel()
    print("level: B=%d K=%d N=%d C=%d  rows=%d per source at 2730 bits (%.1f MB each)  %s"
          % (B, K, N, C, rows, data.numel() / 1e6, torch.cuda.get_device_name()))

    def composition():
        os.environ["AC_LEVEL_NOFUSE"] = "1"   # (read per call)
        try:
            return base.packed_rows_level(data, index, True)
        finally:
            del os.environ["AC_LEVEL_NOFUSE"]

    def decode_route():
        pcm = base.decode_packed(data, index)
        return pcm.view(B, -1, N, C).square().sum(dim=2)   # the energy of every block

    one, two = base.packed_rows_level(data, index, True), composition()
    assert all(torch.equal(g, r) for g, r in zip(one, two)), "the two forms differ"
    print("launches %d; the one launch and the composition agree bit for bit; %d bad rows; mean energy %.4g"
          % (base.packed_rows_level_launches(C), int(one[1].sum()), float(one[0].mean())))
    del one, two
    gen = torch.Generator("cuda").manual_seed(1)
    levels = {S: torch.rand((S, B, K + 1, C), device="cuda", generator=gen) * (torch.rand((S, B, K + 1, 1), device="cuda", generator=gen) < 0.25)
              for S in (4, 8)}
    states = {S: torch.zeros((S, B), device="cuda") for S in (4, 8)}
    routes = dst.mix_minus_routes(4)

    def bridge():
        lv = [base.packed_rows_level(d, i, True) for d, i in sources]
        active = base.select_loudest([e for e, _ in lv], 2, torch.stack([bad == 0 for _, bad in lv]), 0.5, 0.0)
        return dst.route_packed_rows(sources, routes, active)

    forms = [("(a) packed_rows_level, %d launch" % base.packed_rows_level_launches(C), lambda: base.packed_rows_level(data, index, True)),
             ("(b) packed_rows_level, composition", composition),
             ("(c) decode_packed + energy of every PCM block", decode_route),
             ("(d) transrate_packed_rows to 1365 bits", lambda: dst.transrate_packed_rows(data, index)),
             ("(e) select_loudest, S = 4, n = 2", lambda: base.select_loudest(levels[4], 2, None, 0.5, 0.0, states[4])),
             ("(e) select_loudest, S = 8, n = 2", lambda: base.select_loudest(levels[8], 2, None, 0.5, 0.0, states[8])),
             ("(f) bridge of 4: everyone routed", lambda: dst.route_packed_rows(sources, routes)),
             ("(f) bridge of 4: 4 levels + select (n = 2) + route", bridge)]
    runs = dict((n, []) for n, _ in forms)
    for _ in range(a.rounds):
        for n, fn in forms:
            runs[n].append(timed(fn, a.round_steps, 1))
    med, spread = [], []
    for n, _ in forms:
        v = sorted(runs[n])
        med.append(v[len(v) // 2])
        spread.append(v[-1] - v[0])
        print("  %-52s median %.3f ms  min %.3f  max %.3f  (%d alternating rounds of %d)" % (n, med[-1], v[0], v[-1], len(v), a.round_steps))
    read = data.numel() + rows * 13
    print("  (a) / (b) = %.3f   (b) - (a) = %.3f ms against a spread of %.3f   (a) / (c) = %.3f   (a) / (d) = %.3f   (a) moves %.1f MB: %.0f GB/s"
          % (med[0] / med[1], med[1] - med[0], max(spread[0], spread[1]), med[0] / med[2], med[0] / med[3], read / 1e6, read / med[0] / 1e6))
    print("  bridge: selected / everyone = %.3f   everyone - selected = %.3f ms against a spread of %.3f"
          % (med[7] / med[6], med[6] - med[7], max(spread[6], spread[7])))


def conceal_rows(a):
    """Concealment of lost rows on the rows of encode_packed_rows at --row-bits: (a) decode_packed
    without `lost`, the yardstick; (b) with `lost` all false; (c) with 1 % of the rows lost at random, max_age 8 -- both the
    one launch of k_inv_fast_pl; (d) the composition of (c) (AC_DECODE_PACKED_NOFUSE=1, read per call: conceal_plan, unpack,
    conceal_fade, decode_quantized).  Compared bit for bit first, then alternating, --rounds rounds of --round-steps,
    float32 and 16-bit PCM out."""
    B, K, N, C = a.clips, a.blocks, a.filters, a.channels
    cbr = audiocodec_amd.AudioCodec(48000, N).with_row_budget(a.row_bits)
    x = (torch.rand((B, K * N, C), device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
    data, index, _ = cbr.encode_packed_rows(x)
    del x
    none = torch.zeros(index.shape, dtype=torch.uint8, device="cuda")
    some = (torch.rand(index.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) < 0.01).to(torch.uint8)
    print("conceal: B=%d K=%d N=%d C=%d  rows=%d at %d bits (%.1f MB)  %d rows lost (%.2f %%)  max_age 8  decode_packed "
          "launches=%d  %s" % (B, K, N, C, index.numel(), a.row_bits, data.numel() / 1e6, int(some.sum()),
                               100.0 * float(some.float().mean()), cbr.decode_packed_launches(C), torch.cuda.get_device_name()))

    def composition(lost, pcm16):
        os.environ["AC_DECODE_PACKED_NOFUSE"] = "1"   # (read per call)
        try:
            return cbr.decode_packed(data, index, pcm16, lost=lost, max_age=8)
        finally:
            del os.environ["AC_DECODE_PACKED_NOFUSE"]

    for pcm16 in (False, True):
        v = torch.int16
        plain = cbr.decode_packed(data, index, pcm16)
        assert torch.equal(cbr.decode_packed(data, index, pcm16, lost=none).view(v), plain.view(v)), "none lost != the plain decode"
        one, two = cbr.decode_packed(data, index, pcm16, lost=some, max_age=8), composition(some, pcm16)
        assert one.dtype == two.dtype and torch.equal(one.view(v), two.view(v)), "the two forms differ"
        del plain, one, two
    print("none lost equals the plain decode; the one launch and the composition agree bit for bit (float32 and 16-bit PCM)")
    for pcm16 in (False, True):
        forms = [("(a) decode_packed", lambda: cbr.decode_packed(data, index, pcm16)),
                 ("(b) lost all false, %d launch" % cbr.decode_packed_launches(C), lambda: cbr.decode_packed(data, index, pcm16, lost=none)),
                 ("(c) 1 %% lost, %d launch" % cbr.decode_packed_launches(C), lambda: cbr.decode_packed(data, index, pcm16, lost=some)),
                 ("(d) 1 % lost, composition", lambda: composition(some, pcm16))]
        runs = dict((n, []) for n, _ in forms)
        for _ in range(a.rounds):
            for n, fn in forms:
                runs[n].append(timed(fn, a.round_steps, 1))
        med = []
        print("%s out:" % ("16-bit PCM" if pcm16 else "float32"))
        for n, _ in forms:
            v = sorted(runs[n])
            med.append(v[len(v) // 2])
            print("  %-32s median %.3f ms  min %.3f  max %.3f  (%d alternating rounds of %d)" % (n, med[-1], v[0], v[-1], len(v), a.round_steps))
        print("  (b) / (a) = %.3f   (c) / (a) = %.3f   (c) / (d) = %.3f" % (med[1] / med[0], med[2] / med[0], med[2] / med[3]))


def conceal_stream_rows(a):
    """Concealment of lost rows in a stream ("Streams") on the rows of encode_packed_rows_chunk at
    --row-bits, per workload: (a) decode_packed_chunk without `lost`, the yardstick (k_inv_fast_p; the only form an older
    commit has, so the same script times it there); (b) with `lost` all false; (c) with 1 % of the rows lost at random,
    max_age 8 -- both the one launch of k_inv_fast_pls; (d) the composition of (c) (AC_DECODE_PACKED_NOFUSE=1, read per call).
    Compared bit for bit first, then alternating, --rounds rounds of --round-steps passes over the workload's chunks, float32
    and 16-bit PCM out.  Two workloads: one stereo clip in chunks of 256 blocks and --clips x --blocks as one chunk."""
    import inspect
    N, C = a.filters, a.channels
    cbr = audiocodec_amd.AudioCodec(48000, N).with_row_budget(a.row_bits)
    rb = (a.row_bits + 31) // 32 * 4
    new = "lost" in inspect.signature(audiocodec_amd.codec.StreamingMDCT.decode_packed_chunk).parameters
    for name, B, k, n in (("one clip, chunks of 256 blocks", 1, 256, 8), ("%d clips x %d blocks, one chunk" % (a.clips, a.blocks), a.clips, a.blocks, 1)):
        g = torch.Generator("cuda").manual_seed(1)
        enc, dec, comp = cbr.stream(B, C), cbr.stream(B, C), cbr.stream(B, C)
        packed = []
        for _ in range(n):
            packed.append(enc.encode_packed_rows_chunk(torch.rand((B, k * N, C), device="cuda", generator=g) * 2 - 1)[0])
        index = (torch.arange(B * k * C, dtype=torch.int64, device="cuda") * rb).view(B, k, C)
        none = torch.zeros(index.shape, dtype=torch.uint8, device="cuda")
        some = [(torch.rand(index.shape, device="cuda", generator=g) < 0.01).to(torch.uint8) for _ in range(n)]

        def composition(pcm16):
            os.environ["AC_DECODE_PACKED_NOFUSE"] = "1"   # (read per call)
            try:
                return [comp.decode_packed_chunk(d, index, pcm16=pcm16, lost=s, max_age=8) for d, s in zip(packed, some)]
            finally:
                del os.environ["AC_DECODE_PACKED_NOFUSE"]

        launches = ""
        if new:
            v = torch.int16
            for pcm16 in (False, True):
                dec.reset()
                plain = [dec.decode_packed_chunk(d, index, pcm16=pcm16) for d in packed]
                dec.reset()
                for d, w in zip(packed, plain):
                    assert torch.equal(dec.decode_packed_chunk(d, index, pcm16=pcm16, lost=none).view(v), w.view(v)), "none lost != the plain chunk"
                dec.reset()
                comp.reset()
                one = [dec.decode_packed_chunk(d, index, pcm16=pcm16, lost=s, max_age=8) for d, s in zip(packed, some)]
                for o, t in zip(one, composition(pcm16)):
                    assert o.dtype == t.dtype and torch.equal(o.view(v), t.view(v)), "the two forms differ"
                del plain, one
            launches = ("  launches: %d; none lost equals the plain chunk, the one launch and the composition agree bit for bit "
                        "(float32 and 16-bit PCM)" % dec.packed_chunk_launches(decode=True, conceal=True))
        print("conceal stream: %s  (B=%d k=%d N=%d C=%d, %d chunks per pass, %d bits per row, %.2f %% of the rows lost, max_age 8)  %s%s"
              % (name, B, k, N, C, n, a.row_bits, 100.0 * float(torch.stack(some).float().mean()), torch.cuda.get_device_name(), launches))
        for pcm16 in (False, True):
            forms = [("(a) decode_packed_chunk", lambda: [dec.decode_packed_chunk(d, index, pcm16=pcm16) for d in packed])]
            if new:
                forms += [("(b) lost all false, one launch", lambda: [dec.decode_packed_chunk(d, index, pcm16=pcm16, lost=none) for d in packed]),
                          ("(c) 1 % lost, one launch",
                           lambda: [dec.decode_packed_chunk(d, index, pcm16=pcm16, lost=s, max_age=8) for d, s in zip(packed, some)]),
                          ("(d) 1 % lost, composition", lambda: composition(pcm16))]
            runs = dict((f, []) for f, _ in forms)
            for _ in range(a.rounds):
                for f, fn in forms:
                    runs[f].append(timed(fn, a.round_steps, 1) / n * 1e3)
            med = []
            print("  %s out:" % ("16-bit PCM" if pcm16 else "float32"))
            for f, _ in forms:
                v = sorted(runs[f])
                med.append(v[len(v) // 2])
                print("    %-32s median %9.1f us per chunk  min %9.1f  max %9.1f  (%d alternating rounds of %d)"
                      % (f, med[-1], v[0], v[-1], len(v), a.round_steps))
            if new:
                print("    (b) / (a) = %.3f   (c) / (a) = %.3f   (c) / (d) = %.3f" % (med[1] / med[0], med[2] / med[0], med[2] / med[3]))


def protect_stream_rows(a):
    """The recovering decode of chunks ("Streams") on protected slots -- rows of
    encode_packed_rows_chunk at 2730 bits, protected chunk by chunk to --row-bits with a copy at --red-bits -- per workload:
    (a) decode_packed_chunk with `lost`, the concealing chunk (k_inv_fast_pls), on the same `lost` as (c): the yardstick; (b)
    with redundant_at and nothing lost; (c) with redundant_at and 1 % of the rows lost at random, max_age 8 -- both the one
    launch of k_inv_fast_plsr; (d) the composition of (c) (AC_DECODE_PACKED_NOFUSE=1, read per call).  (c) and (d) compared
    byte for byte first, flush included, then alternating, --rounds rounds of --round-steps passes over the workload's chunks,
    float32 and 16-bit PCM out.  Two workloads: one stereo clip in chunks of 256 blocks and --clips x --blocks as one chunk."""
    N, C = a.filters, a.channels
    base = audiocodec_amd.AudioCodec(48000, N)
    src, dst = base.with_row_budget(2730), base.with_row_budget(a.row_bits)
    o = dst.row_bytes
    for name, B, k, n in (("one clip, chunks of 256 blocks", 1, 256, 8), ("%d clips x %d blocks, one chunk" % (a.clips, a.blocks), a.clips, a.blocks, 1)):
        g = torch.Generator("cuda").manual_seed(1)
        enc, pls, dec, comp = src.stream(B, C), dst.stream(B, C), dst.stream(B, C), dst.stream(B, C)
        packed = []
        for _ in range(n):
            data, index, _ = enc.encode_packed_rows_chunk(torch.rand((B, k * N, C), device="cuda", generator=g) * 2 - 1)
            packed.append(dst.protect_packed_rows(data, index, a.red_bits)[:2])
        none = torch.zeros((B, k, C), dtype=torch.uint8, device="cuda")
        some = [(torch.rand((B, k, C), device="cuda", generator=g) < 0.01).to(torch.uint8) for _ in range(n)]

        def recovering(st, lost, pcm16):
            st.reset()
            return [st.decode_packed_chunk(d, i, pcm16=pcm16, lost=s, max_age=8, redundant_at=o) for (d, i), s in zip(packed, lost)]

        def composition(pcm16):
            os.environ["AC_DECODE_PACKED_NOFUSE"] = "1"   # (read per call)
            try:
                return recovering(comp, some, pcm16)
            finally:
                del os.environ["AC_DECODE_PACKED_NOFUSE"]

        def concealing(pcm16):
            pls.reset()
            return [pls.decode_packed_chunk(d, i, pcm16=pcm16, lost=s, max_age=8) for (d, i), s in zip(packed, some)]

        v = torch.int16
        for pcm16 in (False, True):
            one = recovering(dec, some, pcm16) + [dec.flush_packed(pcm16)]
            os.environ["AC_DECODE_PACKED_NOFUSE"] = "1"
            try:
                two = recovering(comp, some, pcm16) + [comp.flush_packed(pcm16)]
            finally:
                del os.environ["AC_DECODE_PACKED_NOFUSE"]
            for p, q in zip(one, two):
                assert p.dtype == q.dtype and torch.equal(p.view(v), q.view(v)), "the two forms differ"
            del one, two
        print("protect stream: %s  (B=%d k=%d N=%d C=%d, %d chunks per pass, %d + %d bits per slot, %.2f %% of the rows lost, max_age 8)  %s"
              "  launches: %d; the one launch and the composition agree byte for byte, flush included (float32 and 16-bit PCM)"
              % (name, B, k, N, C, n, a.row_bits, a.red_bits, 100.0 * float(torch.stack(some).float().mean()), torch.cuda.get_device_name(),
                 dec.packed_chunk_launches(decode=True, conceal=True, recover=True)))
        for pcm16 in (False, True):
            forms = [("(a) concealing chunk, 1 % lost", lambda: concealing(pcm16)),
                     ("(b) recovering, none lost", lambda: recovering(dec, [none] * n, pcm16)),
                     ("(c) recovering, 1 % lost", lambda: recovering(dec, some, pcm16)),
                     ("(d) recovering, composition", lambda: composition(pcm16))]
            runs = dict((f, []) for f, _ in forms)
            for _ in range(a.rounds):
                for f, fn in forms:
                    runs[f].append(timed(fn, a.round_steps, 1) / n * 1e3)
            med = []
            print("  %s out:" % ("16-bit PCM" if pcm16 else "float32"))
            for f, _ in forms:
                t = sorted(runs[f])
                med.append(t[len(t) // 2])
                print("    %-32s median %9.1f us per chunk  min %9.1f  max %9.1f  (%d alternating rounds of %d)"
                      % (f, med[-1], t[0], t[-1], len(t), a.round_steps))
            print("    (b) / (a) = %.3f   (c) / (a) = %.3f   (c) / (d) = %.3f" % (med[1] / med[0], med[2] / med[0], med[2] / med[3]))
        # ---- the sending side: protect_chunk against the one-shot protect on the same rows, and against its composition
        rows = []
        enc.reset()
        g = torch.Generator("cuda").manual_seed(1)
        for _ in range(n):
            rows.append(enc.encode_packed_rows_chunk(torch.rand((B, k * N, C), device="cuda", generator=g) * 2 - 1)[:2])
        ps, pc = dst.protect_stream(B, C, a.red_bits), dst.protect_stream(B, C, a.red_bits)

        def chunks(p, nofuse=False):
            if nofuse:
                os.environ["AC_PROTECT_NOFUSE"] = "1"   # (read per call)
            try:
                p.reset()
                return [p.protect_chunk(d, i, True) for d, i in rows]
            finally:
                if nofuse:
                    del os.environ["AC_PROTECT_NOFUSE"]

        for p, q in zip(chunks(ps), chunks(pc, True)):
            for t, u in zip(p, q):
                assert t.dtype == u.dtype and torch.equal(t, u), "protect_chunk: the two forms differ"
        forms = [("(a) protect_packed_rows, one-shot", lambda: [dst.protect_packed_rows(d, i, a.red_bits, True) for d, i in rows]),
                 ("(b) protect_chunk, one launch", lambda: chunks(ps)),
                 ("(c) protect_chunk, composition", lambda: chunks(pc, True))]
        runs = dict((f, []) for f, _ in forms)
        for _ in range(a.rounds):
            for f, fn in forms:
                runs[f].append(timed(fn, a.round_steps, 1) / n * 1e3)
        med = []
        print("  protect, launches %d; the one launch and the composition agree byte for byte:" % ps.launches())
        for f, _ in forms:
            t = sorted(runs[f])
            med.append(t[len(t) // 2])
            print("    %-36s median %9.1f us per chunk  min %9.1f  max %9.1f  (%d alternating rounds of %d)"
                  % (f, med[-1], t[0], t[-1], len(t), a.round_steps))
        print("    (b) / (a) = %.3f   (b) / (c) = %.3f" % (med[1] / med[0], med[1] / med[2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--protect-stream", action="store_true", help="only decode_packed_chunk with redundant_at, against the concealing chunk and its composition")
    ap.add_argument("--conceal-stream", action="store_true", help="only decode_packed_chunk with lost rows concealed, against without")
    ap.add_argument("--level", action="store_true", help="only packed_rows_level and select_loudest on sources at 2730 bits")
    ap.add_argument("--mix", action="store_true", help="only mix_packed_rows: --sources sources at 2730 bits mixed to 1365")
    ap.add_argument("--sources", type=int, nargs="+", default=[2, 4], help="the source counts of --mix (--route: 2 3 4 8 by default)")
    ap.add_argument("--route", action="store_true", help="only route_packed_rows: mix-minus of --sources parties at 2730 bits to 1365")
    ap.add_argument("--protect", action="store_true", help="only protect_packed_rows and the recovering decode (2730 -> 1365 with --red-bits)")
    ap.add_argument("--red-bits", type=int, default=341, help="the redundant budget of --protect (16 kbit/s)")
    ap.add_argument("--conceal", action="store_true", help="only decode_packed with lost rows concealed, against without")
    ap.add_argument("--transrate", action="store_true", help="only transrating: rows at --row-bits (default 2730 here) to --targets")
    ap.add_argument("--targets", type=int, nargs="+", default=[1365, 682], help="the target budgets of --transrate")
    ap.add_argument("--pcm16", action="store_true", help="only int16 PCM to packed rows, one-shot and chunk by chunk")
    ap.add_argument("--stream", action="store_true", help="only the packed rows of a stream, chunk by chunk")
    ap.add_argument("--row-bits", type=int, default=1365, help="the row budget of the packed-rows section (64 kbit/s)")
    ap.add_argument("--only-rows", action="store_true", help="only the packed-rows section")
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=468)
    ap.add_argument("--filters", type=int, default=1024)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-steps", type=int, default=30)
    a = ap.parse_args()
    B, K, N, C = a.clips, a.blocks, a.filters, a.channels
    if a.protect_stream:
        return protect_stream_rows(a)
    if a.level:
        return level_rows(a)
    if a.mix:
        return mix_rows(a)
    if a.route:
        return route_rows(a)
    if a.protect:
        return protect_rows(a)
    if a.conceal:
        return conceal_rows(a)
    if a.conceal_stream:
        return conceal_stream_rows(a)
    if a.transrate:
        if a.row_bits == 1365:
            a.row_bits = 2730   # the source rows: 128 kbit/s
        return transrate_rows(a)
    if a.pcm16:
        return pcm16_rows(a)
    if a.stream:
        return stream_rows(a)
    if a.only_rows:
        return packed_rows(a)
    codec = audiocodec_amd.AudioCodec(48000, N)
    psy, lib = codec.psy, _lib.load()
    M = psy.bark_bands_n
    x = (torch.rand((B, K * N, C), device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
    codes, sf = codec.encode_quantized(x)
    del x
    F = K + 1
    data, index = psy.pack(codes, sf)
    rows = B * F * C
    samples = B * F * N * C
    code_b, sf_b, pk_b, ix_b = codes.numel() * 2, sf.numel(), data.numel(), rows * 8
    pcm_f32 = B * (F + 1) * N * C * 4
    pcm_i16 = pcm_f32 // 2
    print("pack_bench: B=%d K=%d N=%d C=%d M=%d  rows=%d  decode_quantized launches=%d  decode_packed launches=%d  %s"
          % (B, K, N, C, M, rows, codec.decode_quantized_launches(C), codec.decode_packed_launches(C),
             torch.cuda.get_device_name()))
    print("size: codes+sf %.1f MB -> packed %.1f MB (%.2fx smaller)  bits/sample %.3f (%.3f with the 8-byte index per row)"
          % ((code_b + sf_b) / 1e6, pk_b / 1e6, (code_b + sf_b) / pk_b, 8.0 * pk_b / samples, 8.0 * (pk_b + ix_b) / samples))
    print("widest code: %d" % int(codes.abs().max()))

    plan, dev = psy._plan(codes.device), codes.device
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nscr = int(lib.ac_pack_scratch_bytes(B, F, C))
    scratch = torch.empty((max(nscr, 1),), dtype=torch.uint8, device=dev)
    index2, total = torch.empty_like(index), torch.empty((1,), dtype=torch.int64, device=dev)
    data2 = torch.empty_like(data)

    def pack_index():
        _lib.check(lib.ac_pack_index(plan, p(codes), p(sf), p(index2), p(total), p(scratch) if nscr else None, B, F, C, s))

    def pack_both():
        pack_index()
        _lib.check(lib.ac_pack(plan, p(codes), p(sf), p(index2), p(data2), B, F, C, s))

    pack_both()
    torch.cuda.synchronize()
    assert torch.equal(index2, index) and torch.equal(data2, data) and int(total.item()) == pk_b
    out_c, out_s = torch.empty_like(codes), torch.empty_like(sf)

    def unpack_into():
        _lib.check(lib.ac_unpack(plan, p(data), pk_b, p(index), p(out_c), p(out_s), B, F, C, s))

    def composition(pcm16):
        os.environ["AC_DECODE_PACKED_NOFUSE"] = "1"   # (read per call)
        try:
            return codec.decode_packed(data, index, pcm16=pcm16)
        finally:
            del os.environ["AC_DECODE_PACKED_NOFUSE"]

    for pcm16 in (False, True):   # the two forms give the same bits at the timed size
        one, two = codec.decode_packed(data, index, pcm16=pcm16), composition(pcm16)
        assert one.dtype == two.dtype and torch.equal(one.view(torch.int16), two.view(torch.int16)), "the two forms differ"
        del one, two
    print("decode_packed: the one launch and unpack + decode_quantized agree bit for bit (float32 and 16-bit PCM)")

    rows_t = [
        ("pack_index", pack_index, code_b + sf_b + ix_b),
        ("pack_index + pack", pack_both, code_b + sf_b + pk_b),
        ("psy.pack (syncs)", lambda: psy.pack(codes, sf), code_b + sf_b + pk_b),
        ("unpack (into)", unpack_into, pk_b + code_b + sf_b),
        ("psy.unpack", lambda: psy.unpack(data, index), pk_b + code_b + sf_b),
        ("decode_packed f32", lambda: codec.decode_packed(data, index), pk_b + ix_b + pcm_f32),
        ("decode_quantized f32", lambda: codec.decode_quantized(codes, sf), code_b + sf_b + pcm_f32),
    ]
    res = {}
    for name, fn, nbytes in rows_t:
        ms = timed(fn, a.steps, a.warmup)
        res[name] = ms
        print("%-24s %8.3f ms  %6.3f GB  %6.2f TB/s" % (name, ms, nbytes / 1e9, nbytes / ms / 1e9))
    print("decode_packed / decode_quantized = %.3f" % (res["decode_packed f32"] / res["decode_quantized f32"]))
    if a.rounds < 1:
        return
    # the two forms of decode_packed and decode_quantized, alternating in this process
    forms = [
        ("decode_packed f32 (%d launch)" % codec.decode_packed_launches(C), lambda: codec.decode_packed(data, index),
         pk_b + ix_b + pcm_f32),
        ("unpack + decode_quantized f32", lambda: composition(False), pk_b + ix_b + 2 * (code_b + sf_b) + pcm_f32),
        ("decode_quantized f32", lambda: codec.decode_quantized(codes, sf), code_b + sf_b + pcm_f32),
        ("decode_packed pcm16 (%d launch)" % codec.decode_packed_launches(C),
         lambda: codec.decode_packed(data, index, pcm16=True), pk_b + ix_b + pcm_i16),
        ("unpack + decode_quantized pcm16", lambda: composition(True), pk_b + ix_b + 2 * (code_b + sf_b) + pcm_i16),
        ("decode_quantized pcm16", lambda: codec.decode_quantized(codes, sf, pcm16=True), code_b + sf_b + pcm_i16),
    ]
    runs = dict((n, []) for n, _, _ in forms)
    for _ in range(a.rounds):
        for n, fn, _ in forms:
            runs[n].append(timed(fn, a.round_steps, 1))
    med = {}
    for n, _, nbytes in forms:
        v = sorted(runs[n])
        med[n] = v[len(v) // 2]
        print("%-34s median %.3f ms  min %.3f  max %.3f  %6.3f GB  %5.2f TB/s  (%d alternating rounds of %d)"
              % (n, med[n], v[0], v[-1], nbytes / 1e9, nbytes / med[n] / 1e9, len(v), a.round_steps))
    for k in (0, 3):
        print("%s: one launch / composition = %.3f   one launch / decode_quantized = %.3f"
              % ("pcm16" if k else "f32", med[forms[k][0]] / med[forms[k + 1][0]], med[forms[k][0]] / med[forms[k + 2][0]]))
    packed_rows(a)


if __name__ == "__main__":
    main()
