"""Harness of test_stream_contract.py: does a library call keep to the stream it was given?

The library promises (include/audiocodec_amd.h) that a call only enqueues on the given stream and never
synchronises.  On inputs that are already complete a launch on the wrong stream gives the right bits, so the two checks
here put a long delay kernel (``torch.cuda._sleep``) between the call's own stream and everything else:

* :meth:`Harness.delayed_producer` -- the inputs of the call are produced on the call's stream BEHIND the delay; whatever
  the call puts on another stream runs during the delay, on zeros or on intermediates that are not written yet;
* :meth:`Harness.busy_default` -- the default (null) stream sleeps while the call runs on a side stream whose inputs are
  there; a call that touches the null stream or waits for the device returns only after the delay.

A *case* is ``(inputs, fn)``: device tensors and a callable ``fn(*inputs)`` that returns a tensor or a (nested) tuple of
tensors / None.  ``fn`` addresses its inputs only through its arguments and takes the current stream (or passes one on).
Zeros must be a valid input of ``fn``: the delayed producer runs it on zero-filled stand-ins when a launch strays.

Every check measures its own premise: the delay it really had (events around the sleep) against the warmed call's time
from host entry to completion, and fails when the delay is not ``MARGIN`` times longer.
"""

import time

import torch

DELAY_S = 0.060          # the delay every check enqueues (see the figures in test_stream_contract.py's docstring)
MARGIN = 20              # delay >= MARGIN x (the call, host entry to side-stream completion)
_PROBE_CYCLES = 20_000_000


def flat(out):
    """The tensors of a (nested) result, in order; None entries dropped."""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out for t in flat(o)]


def same_bits(a, b):
    """Bit-for-bit equality (NaN payloads included; dtype and shape must agree)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


class Harness:
    def __init__(self):
        assert torch.cuda.is_available()
        self.default = torch.cuda.default_stream()
        assert self.default.cuda_stream == 0, "torch's default stream is expected to be the null stream"
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        rates = []
        idle = torch.cuda.Stream()
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(idle):
                e0.record()
                torch.cuda._sleep(_PROBE_CYCLES)
                e1.record()
            idle.synchronize()
            rates.append(_PROBE_CYCLES / (e0.elapsed_time(e1) * 1e-3))
        self.rates = rates
        self.rate = min(rates)                    # cycles per second, the slowest of three
        self.cycles = int(DELAY_S * self.rate)
        # Streams are multiplexed onto a few hardware queues (GPU_MAX_HW_QUEUES; 4 is HIP's default), and a stream that
        # shares the null stream's queue runs in order with it: work on it waits behind a sleeping default stream, and a
        # stray null-stream launch waits behind ITS delay -- both checks would be blind on it.  Measured on an MI355X with 4
        # queues: one torch stream in four.  So every side stream the checks use is proved first, in both directions.
        self.tried, self.ring, self._next = 0, [], 0
        for _ in range(16):
            s = torch.cuda.Stream()
            self.tried += 1
            if self._independent(s):
                self.ring.append(s)
        assert len(self.ring) >= 4, "only %d of %d streams run beside the null stream" % (len(self.ring), self.tried)
        self.side = self.fresh()                  # busy_default's side stream, warm (its allocator pool too)
        self.call_s = {}                          # case -> warmed call, host entry to side-stream completion
        self.delay_s = {}                         # (check, case) -> the delay the check really had

    # ---- building blocks ---------------------------------------------------------------------------------------
    def _independent(self, s):
        """Does `s` run beside the null stream, and the null stream beside `s`?  (a short sleep on one, an op on the other)"""
        v = torch.zeros(64, device="cuda")
        torch.cuda.synchronize()
        ok = True
        for sleeper, worker in ((self.default, s), (s, self.default)):
            with torch.cuda.stream(sleeper):
                torch.cuda._sleep(self.cycles // 12)
                ev = torch.cuda.Event()
                ev.record()
            with torch.cuda.stream(worker):
                v.add_(1)
            worker.synchronize()
            ok = ok and not ev.query()
            torch.cuda.synchronize()
        return ok

    def fresh(self):
        """The next proved side stream (torch hands its streams out of a fixed pool: "fresh" is one not used by the
        previous check)."""
        s = self.ring[self._next % len(self.ring)]
        self._next += 1
        return s

    def sleep(self):
        """The delay on the current stream, between two timing events: returns a callable that gives its length in
        seconds once both events have completed."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(self.cycles)
        e1.record()
        return lambda: e0.elapsed_time(e1) * 1e-3

    def reference(self, case):
        """The call on the default stream, everything synchronised before and after."""
        inputs, fn = case
        torch.cuda.synchronize()
        ref = [t.clone() for t in flat(fn(*inputs))]
        torch.cuda.synchronize()
        assert ref, "the case returns no tensor"
        return ref

    def timed(self, name, case, stream):
        """The warmed call once more on `stream`, from host entry to the stream's completion."""
        inputs, fn = case
        with torch.cuda.stream(stream):
            fn(*inputs)
        stream.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            out = fn(*inputs)
        stream.synchronize()
        dt = time.perf_counter() - t0
        del out
        self.call_s[name] = max(dt, self.call_s.get(name, 0.0))
        return dt

    def _margin(self, check, name, delay, call):
        self.delay_s[(check, name)] = delay
        assert delay >= MARGIN * call, ("%s, %s: the delay (%.1f ms) is not %d x the call (%.2f ms): the check has no "
                                        "margin on this machine" % (check, name, delay * 1e3, MARGIN, call * 1e3))

    @staticmethod
    def _compare(check, name, got, ref, same):
        assert len(got) == len(ref), (check, name, len(got), len(ref))
        bad = [i for i, (g, r) in enumerate(zip(got, ref)) if not same(g, r)]
        assert not bad, "%s, %s: outputs %s of %d differ from the default-stream reference" % (check, name, bad, len(ref))

    # ---- check 1 -------------------------------------------------------------------------------------------------
    def delayed_producer(self, name, case, ref=None, same=same_bits, side=None):
        """Every launch of the call waits for its own stream: delay, the copies of the real inputs into zero-filled
        buffers, the call and the clones of its outputs on one fresh side stream (or on `side`)."""
        inputs, fn = case
        ref = self.reference(case) if ref is None else ref
        call = self.timed(name, case, self.side)
        zeros = [torch.zeros_like(t) for t in inputs]
        torch.cuda.synchronize()
        side = self.fresh() if side is None else side
        with torch.cuda.stream(side):
            delay = self.sleep()
            for z, t in zip(zeros, inputs):
                z.copy_(t, non_blocking=True)
            got = [t.clone() for t in flat(fn(*zeros))]
        side.synchronize()
        torch.cuda.synchronize()
        self._margin("delayed producer", name, delay(), call)
        self._compare("delayed producer", name, got, ref, same)
        return got

    # ---- check 2 -------------------------------------------------------------------------------------------------
    def busy_default(self, name, case, ref=None, same=same_bits):
        """The call neither touches the null stream nor waits for the device: it completes on a side stream while the
        default stream still sleeps, with the reference's bits."""
        inputs, fn = case
        ref = self.reference(case) if ref is None else ref
        call = self.timed(name, case, self.side)
        torch.cuda.synchronize()
        delay = self.sleep()                      # on the default stream
        ev = torch.cuda.Event()
        ev.record()
        with torch.cuda.stream(self.side):
            got = [t.clone() for t in flat(fn(*inputs))]
        self.side.synchronize()
        early = not ev.query()
        torch.cuda.synchronize()
        self._margin("busy default stream", name, delay(), call)
        assert early, ("busy default stream, %s: the call returned its results only after the default stream's delay -- "
                       "it put work on the null stream or waited for the device" % name)
        self._compare("busy default stream", name, got, ref, same)
        return got

    # ---- first use -------------------------------------------------------------------------------------------------
    def first_use(self, name, inputs, make, ref):
        """``make()`` builds a FRESH object on the host and returns the callable; its first-ever call (which builds the
        plans) runs on a side stream while the default stream sleeps.  Creation may block the host (then the call simply
        starts after the delay); what it enqueued must be in place before the call's kernels read it.  ``inputs`` are
        complete before the delay starts."""
        torch.cuda.synchronize()
        side = self.fresh()
        delay = self.sleep()                      # on the default stream
        fn = make()
        with torch.cuda.stream(side):
            got = [t.clone() for t in flat(fn(*inputs))]
        side.synchronize()
        torch.cuda.synchronize()
        self.delay_s[("first use", name)] = delay()
        self._compare("first use", name, got, ref, same_bits)
