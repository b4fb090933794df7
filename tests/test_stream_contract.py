"""Every entry point that takes a stream keeps to it (include/audiocodec_amd.h: "every call only enqueues work [on
`stream`] and returns without synchronising").

Two checks per row of the table below (tests/stream_order.py has the harness): the DELAYED PRODUCER -- the inputs of the
call are produced on the call's own stream behind a delay kernel, so whatever the call puts on another stream runs on zeros
or on intermediates that are not written yet -- and the BUSY DEFAULT STREAM -- the null stream sleeps while the warmed call
runs on a side stream; a call that touches the null stream or waits for the device returns only after the delay.  One row per
C entry point that takes a stream (43 in the header), reached through the Python method that calls it, or through the
ctypes binding where none does; test_stream_contract_table.py holds ROWS + EXEMPT to the header without a GPU.  Then: the
first-ever call of a fresh plan of every kind, a stream object created while the default stream sleeps, and two streams
through one codec at once.  Results are compared bit for bit with the same call on the default stream, everything
synchronised: every call proved bit-reproducible run to run.

Measured on an MI355X (GPU_MAX_HW_QUEUES = 4):
* torch.cuda._sleep: 2.391e9, 2.393e9, 2.395e9 cycles/s in three probes (2.05e9 in a first probe of a cold process); the
  slowest rate sets the cycles for DELAY_S = 60 ms, and the 141 checks measured delays of 59.4 .. 59.9 ms.
* the slowest warmed call, host entry to side-stream completion: typed[float64-1024-2] 0.99 ms, then
  backward[float32-1024-2] 0.70 ms and backward[float32-34-2] 0.68 ms; the delay is 60 x the slowest.  Every check measures
  its own delay and its own warmed call and fails if the delay is not 20 x the call.
* streams are multiplexed onto the hardware queues: of 16 torch streams 11 run beside the null stream, the others share
  its queue and run in order with it (a stray null-stream launch would wait behind THEIR delay).  The harness proves every
  side stream independent in both directions before it uses it.
* hipMemset is NOT reliably host-blocking on this runtime.  It is ordered on the null stream, and with the default stream
  asleep a call of 8 KiB, 16 KiB, 64 KiB and 1 MiB in turn took 59.7, 0.00, 59.7 and 0.01 ms on the host: the calls that
  returned at once had not run -- a side stream that read the buffer right after them saw every byte unwritten (16384 of
  16384, 1048576 of 1048576) -- the others had written all of it.  With an idle device every call had completed.
  hipMemcpy from host memory took the delay on the host in every probe (64 KiB, 1 MiB) and had completed.
* the module: 142 cases in 14.9 s beside the suite's 194 s.

Found wrong, and fixed:
* ac_stream_create zeroed the float32 state with four hipMemset calls and returned; under a busy null stream some of them
  were still queued, and a first chunk call on a non-blocking stream overtook them.  Seen as a wrong first frame of chunk 1
  (X, tonality, threshold) at filters_n 1024 and 960 wherever hipMalloc handed back used memory -- a fresh process gets
  zero pages and hides it.  ac_stream_create and the plan builders (hipMemcpy uploads, which were never seen late) now end
  with a wait for the null stream: creation may block the host, and nothing it enqueued can be overtaken.
  test_stream_object_created_while_the_default_stream_sleeps holds it.
* the float64 streaming state: the first float64 chunk call zeroed it with hipMemset -- the null stream, inside a chunk
  call.  It is now hipMemsetAsync on the call's stream (chunks[float64-*] and the float64 case of the test above).
ac_workspace_create fails the busy-default check by design (EXEMPT: it frees its losing candidates); ac_probe_placement
waits for its own stream only and passes it.  Every other entry point passed both checks as it was.

Two things are torch's and not the library's: backward() makes the forward's stream wait for the stream that is current at
the call, so the busy-default rows of the backward kernels call it with the side stream current; and pack() reads its byte
count back, waiting for its own stream only.

Teeth.  The fixture's negative control (ac_mdct_forward on the null stream against a delayed input) must differ from the
reference.  Two scratch builds of the library, never committed, each failed named cases and nothing else of the rows run:
* k_scan_top of launch_pack_index launched on stream 0: test_delayed_producer[pack[2100 rows]] and
  test_busy_default_stream[pack[2100 rows]] (unpack[2100 rows] passed both);
* the hipMemsetAsync of launch_quantize_clip_budget on stream 0: test_delayed_producer and test_busy_default_stream of all
  four quantize_to_clip_budget rows ([1x4500x2x64-int], [1x4500x2x64-tensor], [300x1x2x1024-int], [300x1x2x1024-tensor]),
  all five outputs; test_two_streams_share_one_codec_at_once passed.
A memset that strays to the null stream runs EARLY under the delayed producer, and zeros that nobody overwrites are still
zeros when the kernels read them: those rows first let work on the call's stream fill the blocks the method is about to
allocate with 0x5A (_poison), as a previous tenant of the memory would.

Not covered by an assertion: that results a chunk call allocates under stream= come from that stream's allocator pool
(StreamingMDCT._out).  Only a reuse of freed memory by another stream's work would show it; the docstring of StreamingMDCT
states the rule.
"""

import ctypes
import functools
import time

import pytest
import torch

import audiocodec_amd
from audiocodec_amd import _host, _lib, placement
from stream_order import DELAY_S, Harness, flat, same_bits

gpu = pytest.mark.gpu
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16


# ---- the table ---------------------------------------------------------------------------------------------------------
class Row:
    def __init__(self, rid, covers, build, checks, env, pool):
        self.id, self.covers, self.build, self.checks, self.env, self.pool = rid, tuple(covers), build, checks, env or {}, pool


ROWS = {}
BOTH = ("producer", "busy")


def row(rid, covers, checks=BOTH, env=None, pool=False):
    """Registers ``build() -> (inputs, fn)`` as the row ``rid`` of the table; ``covers`` names the C entry points the row
    reaches with a stream.  checks: "producer" = the delayed producer, "busy" = the busy default stream.  env: switches the
    library reads per call.  pool: both checks use the harness's one side stream (the placed pool hands a released extent
    only to the stream of its last tenant)."""
    def deco(build):
        assert rid not in ROWS, rid
        ROWS[rid] = Row(rid, covers, build, checks, env, pool)
        return build
    return deco


# Entry points that take a stream and have no row, each with its reason (test_stream_contract_table.py holds the header to
# ROWS + EXEMPT).
EXEMPT = {
    "ac_workspace_create": "allocates and frees candidate regions and times the encode on them: it waits for its own stream "
                           "and for the device by design (hipFree), so the busy-default check cannot pass; the header says so",
}


@functools.lru_cache(maxsize=None)
def _codec(N, M=64, dtype=F32, sr=48000, window="vorbis"):
    return audiocodec_amd.AudioCodec(sr, N, bark_bands_n=M, compute_dtype=dtype, window_type=window)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _rand(*shape, dtype=F32):
    return (torch.rand(*shape, device="cuda") * 2 - 1).to(dtype)


def _spectra(B, F, N, C, dtype=F32):
    X = (torch.randn(B, F, N, C, device="cuda") * 10.0 ** (torch.rand(B, F, 1, C, device="cuda") * 4 - 4)).to(dtype)
    thr = (torch.randn(B, F, N, C, device="cuda").abs() * 10.0 ** (torch.rand(B, F, 1, C, device="cuda") * 3 - 5) + 1e-8).to(dtype)
    return X, thr


def _poison(*nbytes):
    """The blocks the next allocations of these sizes get on the current stream, filled with 0x5A by work on that stream:
    a previous tenant's writes, still queued behind whatever the stream waits for.  torch's allocator hands a freed block to
    the next request of its size on the same stream, so the scratch and the outputs a method allocates itself start from
    these bytes -- a memset the call lets stray to another stream runs before (delayed producer) or after (busy default
    stream) the kernels that count on it, and they read 0x5A5A..., not zeros left by luck."""
    blocks = [torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda") for n in nbytes]
    for b in blocks:
        b.fill_(0x5A)


def _bands(N):
    return 8 if N in (30, 34) else 64


def _sp():
    return _host.stream_ptr(_dev())


P = _host.ptr
CK = _lib.check

TYPED_FB = ("ac_mdct_forward_typed", "ac_tonality_typed", "ac_mask_threshold_typed", "ac_mdct_inverse_typed")


# ---- filter bank and masking model -----------------------------------------------------------------------------------
def _fb_case(N, C, dtype=F32, launches=None, extras=False):
    codec = _codec(N, _bands(N), dtype)
    x = _rand(2, 3 * N, C, dtype=dtype)
    if launches is not None:
        assert codec.encode_launches(C) == launches, (N, C, codec.encode_launches(C), launches)

    def fn(x):
        X, t, thr = codec.encode(x, 0.25)
        X2 = codec.mdct.transform(x)
        t2 = codec.psy.tonality(X2)
        thr2 = codec.psy.global_masking_threshold(X2, t2, 0.25)
        out = [X, t, thr, X2, t2, thr2, codec.mdct.inverse_transform(X2)]
        if extras:
            out += [codec.psy.amplitude_to_dB(X2), codec.psy.amplitude_to_dB_norm(X2), codec.psy.add_noise(X2, thr2, seed=11)]
        return out
    return (x,), fn


# 1024 / 2048 / 64: the wave-level kernels (mono, stereo) and what serves three channels; 960: the LDS-FFT tier (stereo: the
# fused encode; six channels: the team forms); 30: the tier's run-time forms; 34: the O(N^2) kernels
FB_SHAPES = [(1024, 1), (1024, 2), (1024, 3), (2048, 1), (2048, 2), (2048, 3), (64, 1), (64, 2), (64, 3), (960, 2), (960, 6),
             (30, 2), (34, 2)]
for _N, _C in FB_SHAPES:
    row("filter_bank[%d-%d]" % (_N, _C), ("ac_encode_fused",) + TYPED_FB)(
        functools.partial(_fb_case, _N, _C, launches=1 if (_N, _C) == (960, 2) else None))
row("encode_two_launches[960-2]", ("ac_encode_fused",) + TYPED_FB, env={"AC_LDS_WAVE_NOFUSE": "1"})(
    functools.partial(_fb_case, 960, 2, launches=2))
row("psy_team[960-6]", ("ac_encode_fused",) + TYPED_FB, env={"AC_PSY_TEAM_ALWAYS": "1"})(functools.partial(_fb_case, 960, 6))

TYPED_ALL = ("ac_encode_fused_typed",) + TYPED_FB + ("ac_amplitude_to_db_typed", "ac_add_noise_typed")
for _dt, _N, _C in [(F64, 1024, 2), (F64, 34, 3), (BF16, 1024, 2), (BF16, 960, 2)]:
    row("typed[%s-%d-%d]" % (str(_dt)[6:], _N, _C), TYPED_ALL)(functools.partial(_fb_case, _N, _C, dtype=_dt, extras=True))


def _f16_case(N, C):
    m = audiocodec_amd.MDCTransformer(N, compute_dtype=F16)
    x = _rand(2, 3 * N, C, dtype=F16)

    def fn(x):
        X = m.transform(x)
        return X, m.inverse_transform(X)
    return (x,), fn


for _N, _C in [(960, 2), (1024, 2), (34, 2)]:
    row("typed[float16-%d-%d]" % (_N, _C), ("ac_mdct_forward_typed", "ac_mdct_inverse_typed"))(functools.partial(_f16_case, _N, _C))


def _direct_case(N, C):
    """The float32 entry points no Python method calls (the package goes through their *_typed twins)."""
    codec = _codec(N, _bands(N))
    lib, dev = _lib.load(), _dev()
    mp, pp = codec.mdct._plan(dev), codec.psy._plan(dev)
    B, K = 2, 3
    Fr = K + 1
    x = _rand(B, K * N, C)
    gt = _rand(B, Fr, 1, C)
    gthr = _rand(B, Fr, N, C)

    def fn(x, gt, gthr):
        sp = _sp()
        e = lambda *s: torch.empty(*s, device="cuda")   # noqa: E731
        X, t, thr, xh = e(B, Fr, N, C), e(B, Fr, 1, C), e(B, Fr, N, C), e(B, (Fr + 1) * N, C)
        gX, gX2, gt2, db, ga, nz = e(B, Fr, N, C), e(B, Fr, N, C), e(B, Fr, 1, C), e(B, Fr, N, C), e(B, Fr, N, C), e(B, Fr, N, C)
        n = X.numel()
        CK(lib.ac_mdct_forward(mp, P(x), P(X), B, K, C, sp))
        CK(lib.ac_tonality(pp, P(X), P(t), B, Fr, C, sp))
        CK(lib.ac_mask_threshold(pp, P(X), P(t), 0.25, P(thr), B, Fr, C, sp))
        CK(lib.ac_mdct_inverse(mp, P(X), P(xh), B, Fr, C, sp))
        CK(lib.ac_tonality_backward(pp, P(X), P(gt), P(gX), 0, B, Fr, C, sp))
        CK(lib.ac_mask_threshold_backward(pp, P(X), P(t), 0.25, P(gthr), P(gX2), P(gt2), B, Fr, C, sp))
        CK(lib.ac_amplitude_to_db(P(X), P(db), n, 1, sp))
        CK(lib.ac_amplitude_to_db_backward(P(X), P(gthr), P(ga), n, 0, sp))
        CK(lib.ac_add_noise(P(X), P(thr), P(nz), n, 7, sp))
        return X, t, thr, xh, gX, gX2, gt2, db, ga, nz
    return (x, gt, gthr), fn


DIRECT = ("ac_mdct_forward", "ac_tonality", "ac_mask_threshold", "ac_mdct_inverse", "ac_tonality_backward",
          "ac_mask_threshold_backward", "ac_amplitude_to_db", "ac_amplitude_to_db_backward", "ac_add_noise")
for _N, _C in [(1024, 2), (960, 3), (34, 2)]:
    row("float32_direct[%d-%d]" % (_N, _C), DIRECT)(functools.partial(_direct_case, _N, _C))


def _elementwise_case():
    psy = _codec(1024).psy
    X, thr = _spectra(1, 3, 1024, 3)

    def fn(X, thr):
        return psy.amplitude_to_dB(X), psy.amplitude_to_dB_norm(X), psy.add_noise(X, thr, seed=11)
    return (X, thr), fn


row("elementwise[float32]", ("ac_amplitude_to_db_typed", "ac_add_noise_typed"))(_elementwise_case)


def _encode_ex_case(N, C):
    codec = _codec(N)
    x = _rand(2, 3 * N, C)
    return (x,), lambda x: codec.encode_ex(x, 0.1, noise_seed=5, db_norm=True)


for _N, _C in [(1024, 2), (960, 2), (1024, 3)]:   # one launch; the encode and two element-wise launches
    row("encode_ex[%d-%d]" % (_N, _C), ("ac_encode_fused_ex",))(functools.partial(_encode_ex_case, _N, _C))


def _pcm16_case(N, C):
    codec = _codec(N)
    lib, dev = _lib.load(), _dev()
    B, K = 2, 3
    xi = torch.randint(-32768, 32768, (B, K * N, C), device="cuda", dtype=torch.int16)
    X = _rand(B, K + 1, N, C) * 0.5

    def fn(xi, X):
        Xf = torch.empty(B, K + 1, N, C, device="cuda")
        CK(lib.ac_mdct_forward_pcm16(codec.mdct._plan(dev), P(xi), P(Xf), B, K, C, _sp()))
        return codec.encode(xi, 0.25), codec.decode(X, pcm16=True), Xf
    return (xi, X), fn


for _N, _C in [(1024, 2), (960, 2), (64, 1)]:
    row("pcm16[%d-%d]" % (_N, _C), ("ac_encode_fused_pcm16", "ac_mdct_inverse_pcm16", "ac_mdct_forward_pcm16"))(
        functools.partial(_pcm16_case, _N, _C))


# ---- backward: the forward on the side stream, .backward() called from the default-stream context ---------------------
# torch's engine runs each backward node on the stream of its forward, and makes that stream wait for the stream that is
# current where backward() is called (the incoming gradients are taken to be produced there).  Under a sleeping default
# stream that wait is torch's, not the library's: the busy-default check calls backward() with the side stream current.
def _backward_case(N, C, dtype, from_default=True):
    full = dtype == F32                                   # (amplitude_to_dB and add_noise are differentiable in float32)
    if dtype == F16:
        mdct, psy = audiocodec_amd.MDCTransformer(N, compute_dtype=F16), None
    else:
        codec = _codec(N, _bands(N), dtype)
        mdct, psy = codec.mdct, codec.psy
    B, K = 2, 3
    x = _rand(B, K * N, C, dtype=dtype)
    Xin = (_rand(B, K, N, C) * 0.5).to(dtype)
    g = [_rand(B, K + 1, N, C, dtype=dtype), _rand(B, K + 1, 1, C, dtype=dtype), _rand(B, K + 1, N, C, dtype=dtype),
         _rand(B, K + 1, N, C, dtype=dtype), _rand(B, K + 1, N, C, dtype=dtype), _rand(B, (K + 1) * N, C, dtype=dtype)]

    def fn(x, Xin, gX, gt, gthr, gdb, gnz, gxh):
        xl, Xl = x.detach().requires_grad_(), Xin.detach().requires_grad_()
        X = mdct.transform(xl)
        roots, grads = [X, mdct.inverse_transform(Xl)], [gX, gxh]
        if psy is not None:
            t = psy.tonality(X)
            roots += [t, psy.global_masking_threshold(X, t, 0.25)]
            grads += [gt, gthr]
        if full:
            roots += [psy.amplitude_to_dB(X), psy.add_noise(X, roots[3], seed=3)]
            grads += [gdb, gnz]
        with torch.cuda.stream(torch.cuda.default_stream() if from_default else torch.cuda.current_stream()):
            torch.autograd.backward(roots, grads)
        return [r.detach() for r in roots], xl.grad, Xl.grad
    return (x, Xin) + tuple(g), fn


BWD = ("ac_tonality_backward_typed", "ac_mask_threshold_backward_typed", "ac_mdct_forward_typed", "ac_mdct_inverse_typed")
for _dt, _N, _C in [(F32, 1024, 2), (F32, 960, 3), (F32, 34, 2), (F64, 64, 2), (BF16, 1024, 2), (F16, 960, 2)]:
    _cov = BWD + (("ac_amplitude_to_db_backward", "ac_add_noise_typed") if _dt == F32 else ())
    row("backward[%s-%d-%d]" % (str(_dt)[6:], _N, _C), _cov if _dt != F16 else BWD[2:], checks=("producer",))(
        functools.partial(_backward_case, _N, _C, _dt))
    row("backward_on_the_side_stream[%s-%d-%d]" % (str(_dt)[6:], _N, _C), _cov if _dt != F16 else BWD[2:], checks=("busy",))(
        functools.partial(_backward_case, _N, _C, _dt, from_default=False))


# ---- quantiser and rate control -------------------------------------------------------------------------------------
def _encoded(N, C, B=2, K=4):
    codec = _codec(N)
    X, _, thr = codec.encode(_rand(B, K * N, C), 0.0)
    return codec, X.clone(), thr.clone()


def _quantize_case():
    codec, X, thr = _encoded(1024, 2)

    def fn(X, thr):
        codes, sf = codec.psy.quantize(X, thr)
        return codes, sf, codec.psy.dequantize(codes, sf)
    return (X, thr), fn


row("quantize_dequantize[1024-2]", ("ac_quantize", "ac_dequantize"))(_quantize_case)


def _decode_quantized_case(N, C, launches):
    codec, X, thr = _encoded(N, C)
    codes, sf = codec.psy.quantize(X, thr)
    assert codec.decode_quantized_launches(C) == launches
    return (codes, sf), lambda codes, sf: (codec.decode_quantized(codes, sf), codec.decode_quantized(codes, sf, pcm16=True))


row("decode_quantized[one launch]", ("ac_decode_quantized",))(functools.partial(_decode_quantized_case, 1024, 2, 1))
row("decode_quantized[two launches]", ("ac_decode_quantized",))(functools.partial(_decode_quantized_case, 960, 2, 2))


def _budget_case(tensor):
    codec, X, thr = _encoded(1024, 2)
    _, _, _, bits = codec.psy.quantize_to_budget(X, thr, 16 * 1024 + 13 * 64)
    if tensor:
        budget = torch.clamp((bits.double() * 0.6).to(torch.int32), min=5 * 64)
        return (X, thr, budget), lambda X, thr, b: codec.psy.quantize_to_budget(X, thr, b, -4)
    budget = max(5 * 64, int(bits.double().mean() * 0.6))
    return (X, thr), lambda X, thr: codec.psy.quantize_to_budget(X, thr, budget, -4)


row("quantize_to_budget[int]", ("ac_quantize_budget",))(functools.partial(_budget_case, False))
row("quantize_to_budget[tensor]", ("ac_quantize_budget",))(functools.partial(_budget_case, True))


def _clip_budget_case(B, Fr, C, N, tensor):
    """(1, 4500, 2, 64): a clip's rows split over workgroups; (300, 1, 2, 1024): more clips than splits.  One call: the
    memset of the totals, the bisection steps, the scan and the codes."""
    psy = audiocodec_amd.PsychoacousticModel(48000, filter_bands_n=N, bark_bands_n=64)
    X, thr = _spectra(B, Fr, N, C)
    floor = Fr * C * 32 * ((5 * 64 + 31) // 32)
    top = psy.quantize_to_clip_budget(X, thr, 2 ** 40)[4]
    nscratch = int(_lib.load().ac_clip_budget_scratch_bytes(psy._plan(_dev()), B, Fr, C))
    assert nscratch > 0
    # what the method allocates, in its order: codes, sf, offset, row bits, clip bits, scratch (the totals the call zeroes)
    sizes = (2 * B * Fr * N * C, B * Fr * 64 * C, 2 * B * Fr * C, 4 * B * Fr * C, 8 * B, nscratch)

    def call(X, thr, T):
        _poison(*sizes)
        return psy.quantize_to_clip_budget(X, thr, T, -2)
    if tensor:
        T = torch.clamp((top.double() * 0.6).long(), min=floor + 40)
        return (X, thr, T), call
    T = max(floor + 40, int(top.double().mean() * 0.6))
    return (X, thr), lambda X, thr: call(X, thr, T)


for _shape in [(1, 4500, 2, 64), (300, 1, 2, 1024)]:
    for _tensor in (False, True):
        row("quantize_to_clip_budget[%s-%s]" % ("x".join(map(str, _shape)), "tensor" if _tensor else "int"),
            ("ac_quantize_clip_budget",))(functools.partial(_clip_budget_case, *_shape, _tensor))


# ---- pack ------------------------------------------------------------------------------------------------------------------
def _pack_inputs():
    codec = _codec(64, 16)
    B, Fr, C = 3, 350, 2                                        # 2100 rows: the three-kernel scan
    assert _lib.load().ac_pack_scratch_bytes(B, Fr, C) > 0
    X, thr = _spectra(B, Fr, 64, C)
    codes, sf = codec.psy.quantize(X, thr)
    return codec.psy, codes, sf


def _pack_case():
    psy, codes, sf = _pack_inputs()
    B, Fr, _, C = codes.shape
    sizes = (8 * B * Fr * C, 8, int(_lib.load().ac_pack_scratch_bytes(B, Fr, C)))   # index, total, the scan's partial sums

    def fn(codes, sf):                                           # (pack() reads its byte count back: it waits for ITS stream)
        _poison(*sizes)
        data, index = psy.pack(codes, sf)
        return data, index, psy.unpack(data, index)
    return (codes, sf), fn


def _unpack_case():
    psy, codes, sf = _pack_inputs()
    data, index = psy.pack(codes, sf)
    return (data, index), lambda data, index: psy.unpack(data, index)


row("pack[2100 rows]", ("ac_pack_index", "ac_pack", "ac_unpack"))(_pack_case)
row("unpack[2100 rows]", ("ac_unpack",))(_unpack_case)


# ---- streaming chunk calls ----------------------------------------------------------------------------------------------
def _chunks_case(N, C, dtype, keyword):
    """Three chunks with a reset() before the third; keyword: the default stream is current and stream= names the side
    stream (results allocated by the call included)."""
    codec = _codec(N, 64, dtype)
    B, k = 2, 2
    st = codec.stream(B, C)
    xs = [_rand(B, k * N, C, dtype=dtype) for _ in range(3)]
    Xs = [(_rand(B, k, N, C) * 0.5).to(dtype) for _ in range(3)]

    def fn(x0, x1, x2, X0, X1, X2):
        cur = torch.cuda.current_stream()
        st.reset()
        out = []
        for i, (x, X) in enumerate(zip((x0, x1, x2), (X0, X1, X2))):
            if i == 2:
                st.reset()
            if keyword:
                with torch.cuda.stream(torch.cuda.default_stream()):
                    out += [st.transform_chunk(x, stream=cur), st.encode_chunk(x, 0.25, stream=cur), st.inverse_chunk(X, stream=cur)]
            else:
                out += [st.transform_chunk(x), st.encode_chunk(x, 0.25), st.inverse_chunk(X)]
        return out
    return tuple(xs) + tuple(Xs), fn


for _dt, _N, _C in [(F32, 1024, 2), (F32, 960, 3), (F64, 64, 2), (BF16, 1024, 2)]:
    for _kw in (False, True):
        row("chunks[%s-%d-%d-%s]" % (str(_dt)[6:], _N, _C, "stream=" if _kw else "current"),
            ("ac_stream_encode_typed", "ac_stream_inverse_typed", "ac_stream_reset"))(
            functools.partial(_chunks_case, _N, _C, _dt, _kw))


def _chunks_direct_case(N, C):
    codec = _codec(N)
    lib, dev = _lib.load(), _dev()
    B, k = 2, 2
    st = codec.stream(B, C)
    pp = codec.psy._plan(dev)
    xs = [_rand(B, k * N, C) for _ in range(2)]
    Xin = _rand(B, k, N, C) * 0.5

    def fn(x0, x1, Xin):
        sp, h = _sp(), st._handle
        CK(lib.ac_stream_reset(h, sp))
        e = lambda *s: torch.empty(*s, device="cuda")   # noqa: E731
        out = []
        for x in (x0, x1):
            Xa, Xb, t, thr, xh = e(B, k, N, C), e(B, k, N, C), e(B, k, 1, C), e(B, k, N, C), e(B, k * N, C)
            CK(lib.ac_stream_forward(h, P(x), P(Xa), k, sp))
            CK(lib.ac_stream_encode(h, pp, P(x), P(Xb), P(t), P(thr), 0.25, k, sp))
            CK(lib.ac_stream_inverse(h, P(Xin), P(xh), k, sp))
            out += [Xa, Xb, t, thr, xh]
        return out
    return tuple(xs) + (Xin,), fn


for _N, _C in [(1024, 2), (960, 3)]:
    row("chunks_direct[%d-%d]" % (_N, _C), ("ac_stream_forward", "ac_stream_encode", "ac_stream_inverse", "ac_stream_reset"))(
        functools.partial(_chunks_direct_case, _N, _C))


# ---- stream run ----------------------------------------------------------------------------------------------------------
def _run_case(K):
    codec = _codec(1024)
    st = codec.stream(1, 2)
    x = _rand(1, K * 1024, 2)

    def fn(x):
        st.reset()
        return st.run(x, 16)
    return (x,), fn


row("run[duplex K=80 k=16]", ("ac_stream_run", "ac_stream_reset"))(functools.partial(_run_case, 80))
row("run[duplex K=83 k=16, short last chunk]", ("ac_stream_run", "ac_stream_reset"))(functools.partial(_run_case, 83))


def _run_graph_case():
    """run(graph=True) after chunk calls: the state sits in the other buffer of its pair, ac_stream_settle moves it home and
    the captured launches replay -- all on the delayed stream.  The graph is keyed by its input buffer, so the case copies
    into one fixed buffer; the capture happens once, in the reference run."""
    codec = _codec(1024)
    st = codec.stream(1, 2)
    x, c = _rand(1, 80 * 1024, 2), _rand(1, 1024, 2)
    buf = torch.empty_like(x)

    def fn(x, c):
        st.reset()
        first = st.transform_chunk(c)
        buf.copy_(x, non_blocking=True)
        return first, st.run(buf, 16, graph=True)
    return (x, c), fn


row("run[graph replay after chunk calls]", ("ac_stream_settle", "ac_stream_run", "ac_stream_reset", "ac_stream_encode_typed"))(
    _run_graph_case)


# ---- workspace ------------------------------------------------------------------------------------------------------------
def _workspace_case():
    codec = _codec(1024)
    B, K, C = 2, 4, 2
    ws = codec.workspace(B, K, C, tune=False)
    x = _rand(B, K * 1024, C)

    def fn(x):
        codec.encode_into(x, ws.X, ws.t, ws.thr, 0.25)
        codec.decode_into(ws.X, ws.xh)
        return ws.X, ws.t, ws.thr, ws.xh
    return (x,), fn


row("workspace[encode_into, decode_into]", ("ac_encode_fused", "ac_mdct_inverse"))(_workspace_case)

POOL_SHAPE = (80, 234, 2)   # (the shape test_pool_streams_and_graph_capture builds its pool for: X is 150 MB)


def _pool_case():
    """codec.encode / decode with results from the placed pool (ac_workspace_alloc_dlpack on the call's stream)."""
    codec = _codec(1024)
    B, K, C = POOL_SHAPE
    x = _rand(B, K * 1024, C)
    placement.release()
    codec.decode(codec.encode(x)[0])                            # warm: builds the pool (probes and synchronises, once)
    torch.cuda.synchronize()
    assert placement.report() is not None

    def fn(x):
        X, t, thr = codec.encode(x, 0.25)
        xh = codec.decode(X)
        assert placement.report()["live_tensors"] >= 3, "results did not come from the pool"
        placement.record_stream(xh, torch.cuda.current_stream())
        return X, t, thr, xh
    return (x,), fn


row("pool[encode, decode]", ("ac_workspace_alloc_dlpack", "ac_workspace_record_stream", "ac_encode_fused", "ac_mdct_inverse_typed"),
    pool=True)(_pool_case)


def _probe_case():
    codec = _codec(1024)
    lib, dev = _lib.load(), _dev()
    B, K, C = 2, 4, 2
    x = _rand(B, K * 1024, C)

    def fn(x):
        X, t = torch.empty(B, K + 1, 1024, C, device="cuda"), torch.empty(B, K + 1, 1, C, device="cuda")
        cands = [torch.empty_like(X) for _ in range(2)]
        arr = (ctypes.c_void_p * 2)(*[c.data_ptr() for c in cands])
        best, ms = ctypes.c_int(-1), (ctypes.c_float * 2)()
        CK(lib.ac_probe_placement(codec.mdct._plan(dev), codec.psy._plan(dev), P(x), P(X), P(t), arr, 2, B, K, C, _sp(),
                                  ctypes.byref(best), ms))
        assert best.value in (0, 1)
        return X, t, cands
    return (x,), fn


# (ac_probe_placement times its candidates and waits for ITS stream by design: the busy-default check holds for it)
row("probe_placement", ("ac_probe_placement",), checks=("busy",))(_probe_case)


# ---- the tests ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    """The harness with its premises proved: they fail loudly, nothing skips."""
    assert torch.cuda.is_available(), "the stream contract is checked on the GPU"
    h = Harness()
    side = h.fresh()
    # the two queues run concurrently: a plain op on a side stream completes while the default stream sleeps
    v = torch.zeros(1024, device="cuda")
    torch.cuda.synchronize()
    delay = h.sleep()
    ev = torch.cuda.Event()
    ev.record()
    with torch.cuda.stream(side):
        v.add_(1)
    side.synchronize()
    early = not ev.query()
    torch.cuda.synchronize()
    figures = "_sleep rates %s cycles/s, %d cycles, delay measured %.2f ms" % (["%.3e" % r for r in h.rates], h.cycles, 1e3 * delay())
    assert delay() >= 0.5 * DELAY_S, "the delay kernel is shorter than calibrated: " + figures
    assert early, "a side stream did not run beside the sleeping default stream: the busy-default check is blind (%s)" % figures
    assert float(v.sum()) == 1024.0
    # ... and the same op on the default stream is seen as late: it waits behind the delay (the host, waiting for the op
    # alone, waits the delay out), and by then the event the busy-default check watches has completed
    delay = h.sleep()
    ev = torch.cuda.Event()
    ev.record()
    t0 = time.perf_counter()
    v.add_(1)
    done = torch.cuda.Event()
    done.record()
    done.synchronize()
    waited = time.perf_counter() - t0
    late = ev.query()
    torch.cuda.synchronize()
    assert waited >= 0.5 * delay(), ("an op on the default stream did not wait for the delay ahead of it: %.2f ms of %.2f"
                                     % (1e3 * waited, 1e3 * delay()))
    assert late, "an op on the default stream completed before the delay ahead of it"
    # negative control of the delayed producer: ac_mdct_forward on the NULL stream while its input is produced behind the
    # delay on a side stream computes on the zeros
    codec = _codec(1024)
    lib, dev = _lib.load(), _dev()
    B, K, C = 2, 3, 2
    x = _rand(B, K * 1024, C)
    ref, got = torch.empty(B, K + 1, 1024, C, device="cuda"), torch.empty(B, K + 1, 1024, C, device="cuda")
    CK(lib.ac_mdct_forward(codec.mdct._plan(dev), P(x), P(ref), B, K, C, None))
    z = torch.zeros_like(x)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        h.sleep()
        z.copy_(x, non_blocking=True)
    CK(lib.ac_mdct_forward(codec.mdct._plan(dev), P(z), P(got), B, K, C, None))
    side.synchronize()
    torch.cuda.synchronize()
    assert float(ref.abs().max()) > 0
    assert not same_bits(got, ref), "a launch on the null stream saw the delayed input: the delayed-producer check is blind"
    assert torch.equal(z, x)
    yield h
    # what the module measured (shown with -s): the figures of the module docstring
    slow = sorted(h.call_s.items(), key=lambda kv: -kv[1])[:5]
    delays = list(h.delay_s.values()) or [0.0]
    print("\nstream contract: _sleep rates %s cycles/s, %d cycles for %.0f ms; delays measured %.1f .. %.1f ms over %d checks; "
          "slowest warmed calls: %s" % (["%.3e" % r for r in h.rates], h.cycles, 1e3 * DELAY_S, 1e3 * min(delays), 1e3 * max(delays),
                                        len(delays), ", ".join("%s %.2f ms" % (k, 1e3 * v) for k, v in slow)))


_CASES = {}


def _case(rid, monkeypatch):
    r = ROWS[rid]
    for k, v in r.env.items():
        monkeypatch.setenv(k, v)
    if rid not in _CASES:                       # the inputs and the reference: computed once, shared, never written
        case = r.build()
        _CASES[rid] = (case, None)
    return r, _CASES[rid][0]


def _ref(rid, h, case):
    if _CASES[rid][1] is None:
        _CASES[rid] = (case, h.reference(case))
    return _CASES[rid][1]


@gpu
@pytest.mark.parametrize("rid", [r for r in ROWS if "producer" in ROWS[r].checks])
def test_delayed_producer(rid, harness, monkeypatch):
    """Check 1: every launch, memset and copy of the call waits for the call's own stream."""
    r, case = _case(rid, monkeypatch)
    harness.delayed_producer(rid, case, _ref(rid, harness, case), side=harness.side if r.pool else None)
    if r.pool:                                   # (the pool serves every later encode of the process: give it back)
        _CASES.pop(rid)
        placement.release()


@gpu
@pytest.mark.parametrize("rid", [r for r in ROWS if "busy" in ROWS[r].checks])
def test_busy_default_stream(rid, harness, monkeypatch):
    """Check 2: the warmed call neither touches the null stream nor waits for the device."""
    r, case = _case(rid, monkeypatch)
    harness.busy_default(rid, case, _ref(rid, harness, case))
    if r.pool:
        _CASES.pop(rid)
        placement.release()


# ---- first use ------------------------------------------------------------------------------------------------------------------
def _first_wave():
    return [_rand(2, 3 * 1024, 2)], lambda: (lambda x, m=audiocodec_amd.MDCTransformer(1024): (m.transform(x),))


def _first_lds_fft():
    return [_rand(2, 3 * 960, 3)], lambda: (lambda x, m=audiocodec_amd.MDCTransformer(960): (m.transform(x),))


def _first_adjoint():   # (the rectangular window: the adjoint plan differs from the plan)
    return [_rand(2, 3, 1024, 2)], lambda: (lambda g, m=audiocodec_amd.MDCTransformer(1024, "rect"): (m._inverse(g, adjoint=True),))


def _first_psy(sr, N, M, C, pre=F64):
    X, _ = _spectra(2, 3, N, C)

    def make():
        p = audiocodec_amd.PsychoacousticModel(sr, N, M, precompute_dtype=pre)

        def fn(X):
            t = p.tonality(X)
            return t, p.global_masking_threshold(X, t, 0.25)
        return fn
    return [X], make


def _first_f64():
    x = _rand(2, 3 * 64, 2, dtype=F64)

    def make():
        c = audiocodec_amd.AudioCodec(48000, 64, compute_dtype=F64)
        return lambda x: c.encode(x, 0.25)
    return [x], make


def _first_fused():
    x = _rand(2, 3 * 1024, 2)
    return [x], lambda: (lambda x, c=audiocodec_amd.AudioCodec(48000, 1024): c.encode(x, 0.25))


FIRST_USE = {
    "wave-level": _first_wave, "LDS-FFT": _first_lds_fft, "adjoint": _first_adjoint, "fused encode": _first_fused,
    "psy fast": lambda: _first_psy(48000, 1024, 64, 2),
    "psy mid (band walk)": lambda: _first_psy(8000, 1024, 64, 3, F32),    # (no run structure: test_runs_image.py)
    "psy runs": lambda: _first_psy(48000, 960, 64, 2),
    "psy generic": lambda: _first_psy(48000, 1024, 128, 2),
    "float64 tables": _first_f64,
}


@gpu
@pytest.mark.parametrize("kind", list(FIRST_USE))
def test_first_use(kind, harness):
    """Plans upload their tables inside the first call on a device, with synchronous runtime calls: the first-ever call of a
    fresh object on a side stream, while the default stream sleeps, computes what a second fresh object computes with
    everything synchronised."""
    if kind == "psy mid (band walk)":
        from emulate_runs import runs_image
        assert runs_image(_lib.load(), 1024, 64, 8000, 0.6, precompute=0) is None
    inputs, make = FIRST_USE[kind]()
    ref = harness.reference((inputs, make()))
    harness.first_use(kind, inputs, make, ref)


@gpu
@pytest.mark.parametrize("dtype,N", [(F32, 1024), (F32, 960), (F64, 64)])
def test_stream_object_created_while_the_default_stream_sleeps(dtype, N, harness):
    """ac_stream_create zeroes the state with runtime calls of its own; the float64 state is allocated and zeroed by the first
    float64 chunk call.  Chunks 1 and 2 on a side stream while the default stream sleeps, chunk 3 after everything has
    synchronised: a zeroing that ran late -- behind the default stream's delay -- wipes the state under chunk 3."""
    codec = _codec(N, 64, dtype)
    B, C, k = 2, 2, 2
    x = _rand(B, 3 * k * N, C, dtype=dtype)
    X, t, thr = codec.encode(x, 0.25)
    xh = codec.decode(X[:, :3 * k].contiguous())
    parts = [x[:, i * k * N:(i + 1) * k * N].contiguous() for i in range(3)]
    Xparts = [X[:, i * k:(i + 1) * k].contiguous() for i in range(3)]
    torch.cuda.synchronize()
    side = harness.fresh()
    delay = harness.sleep()
    st = codec.stream(B, C)
    got = []
    with torch.cuda.stream(side):
        for i in range(2):
            got.append((st.encode_chunk(parts[i], 0.25), st.inverse_chunk(Xparts[i])))
    side.synchronize()
    torch.cuda.synchronize()
    got.append((st.encode_chunk(parts[2], 0.25), st.inverse_chunk(Xparts[2])))
    torch.cuda.synchronize()
    harness.delay_s[("stream create", "%s-%d" % (dtype, N))] = delay()
    bad = []
    for i, ((Xc, tc, thrc), xc) in enumerate(got):
        f = slice(i * k, (i + 1) * k)
        pairs = (("X", Xc, X[:, f]), ("tonality", tc, t[:, f]), ("threshold", thrc, thr[:, f]),
                 ("pcm", xc.reshape(B, k, N, C), xh[:, i * k * N:(i + 1) * k * N].reshape(B, k, N, C)))
        for what, a, b in pairs:
            if not same_bits(a, b):       # which (clip, frame or block) differ, and by how much
                where = [(int(bb), int(ff)) for bb, ff in (a != b).flatten(2).any(2).nonzero().tolist()]
                bad.append("chunk %d %s at (clip, frame) %s, max |diff| %.3g" % (i + 1, what, where, float((a.double() - b.double()).abs().max())))
    assert not bad, "; ".join(bad)


@gpu
def test_two_streams_share_one_codec_at_once(harness):
    """Two side streams released together by one event, each with encode + decode, quantize_to_clip_budget and a StreamingMDCT
    of its own on different inputs through the same AudioCodec: each result equals its serial result."""
    codec = _codec(1024)
    B, K, C = 2, 6, 2
    xs = [_rand(B, K * 1024, C) for _ in range(2)]
    sts = [codec.stream(B, C) for _ in range(2)]
    floor = (K + 1) * C * 32 * ((5 * 64 + 31) // 32)

    def work(x, st):
        st.reset()
        X, t, thr = codec.encode(x, 0.25)
        xh = codec.decode(X)
        q = codec.psy.quantize_to_clip_budget(X, thr, 3 * floor, -2)
        ch = [st.encode_chunk(x[:, i * 3 * 1024:(i + 1) * 3 * 1024].contiguous(), 0.25) for i in range(2)]
        return [t_.clone() for t_ in flat([X, t, thr, xh, q, ch])]

    serial = [work(x, st) for x, st in zip(xs, sts)]
    torch.cuda.synchronize()
    sides = [harness.fresh(), harness.fresh()]
    harness.sleep()
    go = torch.cuda.Event()
    go.record()
    got = []
    for x, st, s in zip(xs, sts, sides):
        with torch.cuda.stream(s):
            s.wait_event(go)
            got.append(work(x, st))
    torch.cuda.synchronize()
    for i in range(2):
        bad = [j for j, (g, r) in enumerate(zip(got[i], serial[i])) if not same_bits(g, r)]
        assert not bad, "stream %d: outputs %s differ from the serial run" % (i, bad)
