"""The chunked calls that keep state on the device: :class:`StreamingMDCT` (the overlap-add wrappers, and packed rows chunk
by chunk) and :class:`ProtectStream` (protected rows chunk by chunk)."""

from __future__ import annotations

import ctypes

import torch

from . import _host, _lib, _rows
from .mdctransformer import MDCTransformer
from .psychoacoustic import PsychoacousticModel


class ProtectStream:
    """:meth:`AudioCodec.protect_packed_rows` chunk by chunk (``AudioCodec.protect_stream``; DESIGN.md section 8g, "Streams").

    :meth:`protect_chunk` returns what ``protect_packed_rows`` returns for the chunk's ``k`` frames, in the same layout, but
    the redundant part, ``red_fits`` and ``red_offset`` of frame 0 are the copy at ``red_bits`` of the previous chunk's last
    *input* row -- on a fresh or reset stream the values of f = 0 -- and the copy of the chunk's last input row is kept for
    the next chunk.  So for any split the chunks' slots, flags and offsets, put together along frames, are those of the
    one-shot call on all rows, byte for byte.  The carry lives on the device, double buffered; the calls only enqueue, on
    ``stream`` or the current stream, and calls on one object are ordered by the caller."""

    def __init__(self, codec, batches_n, channels_n, red_bits, device=None):
        if codec.row_bits is None:
            raise ValueError("protect_stream needs a codec with a row budget (with_bitrate() / with_row_budget())")
        self.codec, self.red_bits = codec, red_bits
        self.B, self.C = int(batches_n), int(channels_n)
        if self.B < 1 or self.C < 1:
            raise ValueError("batches_n (%d) and channels_n (%d) must be positive" % (self.B, self.C))
        self.device = _host.default_device(device, indexed=True)
        self._red_bytes = (red_bits + 31) // 32 * 4
        # two halves of (row, fits, offset); _cur is the half the last chunk wrote, None on a fresh stream
        self._carry = [(torch.zeros((self.B, self.C, self._red_bytes), dtype=torch.uint8, device=self.device),
                        torch.ones((self.B, self.C), dtype=torch.bool, device=self.device),
                        torch.zeros((self.B, self.C), dtype=torch.int16, device=self.device)) for _ in range(2)]
        self._cur = None

    def reset(self):
        """The next chunk's frame 0 takes the values of f = 0 again.  No device work."""
        self._cur = None

    def launches(self):
        """Library launches of :meth:`protect_chunk` (``ac_protect_chunk_launches``): 1 where
        ``protect_packed_rows_launches`` is 1, else those of the composition's two transrating calls (everywhere while
        ``AC_PROTECT_NOFUSE=1`` is set: read per call)."""
        return int(self.codec._lib.ac_protect_chunk_launches(self.codec.psy._plan(self.device), self.C, self.red_bits))

    def protect_chunk(self, data, index, return_offset=False, stream=None):
        """data uint8 [nbytes], index int64 [B, k, C] -> (data', index', fits, red_fits) and, with ``return_offset``, offset
        and red_offset: ``protect_packed_rows``' outputs for the chunk (``index'`` the chunk's own arithmetic index), frame 0
        taking the carried copy.  ``k = 0`` changes nothing."""
        codec = self.codec
        with (torch.cuda.stream(stream) if stream is not None else _host._NO_SWITCH):
            data = codec.psy._check_quant_tensor(data, "data", torch.uint8, ndim=1)
            if data.device != self.device:
                raise ValueError("data lives on %s but the stream's carry lives on %s" % (data.device, self.device))
            index = codec.psy._check_quant_tensor(index, "index", torch.int64, device=data.device, ndim=3)
            if (index.shape[0], index.shape[2]) != (self.B, self.C):
                raise ValueError("index must be [%d, k, %d], got %s" % (self.B, self.C, tuple(index.shape)))
            src_half = None if self._cur is None else self._carry[self._cur]
            nxt = 0 if self._cur is None else self._cur ^ 1
            out = _rows.protect(codec, data, index, self.red_bits, return_offset, (src_half, self._carry[nxt]), stream)
            if index.shape[1]:
                self._cur = nxt   # (only once the call has gone through)
            return out


class StreamingMDCT:
    """Chunked analysis / synthesis with device-resident overlap state (BASELINE config 5).

    Feeding consecutive chunks of ``k`` blocks gives, frame for frame, the one-shot ``transform`` /
    ``inverse_transform`` result: analysis frame ``i`` of a chunk pairs block ``i`` with block ``i-1``
    (the stored last block of the previous chunk for ``i = 0``); synthesis block ``i`` overlap-adds
    frame ``i`` with the stored aliased half of the previous frame.  With a masking model (``psy``)
    :meth:`encode_chunk` also returns tonality and threshold of the chunk's frames -- bit for bit what the one-shot
    ``AudioCodec.encode`` gives for those frames.  On a stream of a codec at a bitrate (``with_bitrate()``)
    :meth:`encode_packed_rows_chunk` and :meth:`decode_packed_chunk` go from a chunk of PCM to fixed-stride packed rows and
    back on the same state, one launch each where :meth:`packed_chunk_launches` is 1.

    Streams: every chunk call only enqueues on its stream -- the current one, or ``stream=`` -- and never touches the
    default stream or waits for the device.  Creating the object may block the host and leaves the float32 state zeroed;
    the float64 state is allocated by the first float64 chunk call and zeroed on that call's stream, ahead of its
    kernels.  Results a chunk call allocates itself (``out=None``) are allocated under the stream the work runs on, so
    torch's allocator hands their memory on in that stream's order; a caller that consumes them on another stream
    orders that itself (an event, and ``record_stream``).  The overlap state is carried from call to call: calls on one
    object are ordered by the caller (one stream, or events between streams).
    """

    def __init__(self, mdct: MDCTransformer, batches_n, channels_n, device=None, psy: PsychoacousticModel = None):
        if mdct.compute_dtype not in (torch.float32, torch.float64, torch.bfloat16):
            raise NotImplementedError("streaming overlap-add serves compute_dtype float32 and float64 (every size) and bfloat16 "
                                      "(the wave-level kernels: filters_n 1024 / 2048, mono / stereo); got %s" % mdct.compute_dtype)
        if psy is not None:
            if psy.compute_dtype != mdct.compute_dtype:
                raise ValueError("psy.compute_dtype (%s) != mdct.compute_dtype (%s)" % (psy.compute_dtype, mdct.compute_dtype))
            if psy.filter_bands_n != mdct.filters_n:
                raise ValueError("psy.filter_bands_n (%d) != mdct.filters_n (%d)" % (psy.filter_bands_n, mdct.filters_n))
        self.mdct, self.psy = mdct, psy
        self.B, self.C = int(batches_n), int(channels_n)
        self.device = _host.default_device(device, indexed=True)
        self._lib = _lib.load()
        handle = ctypes.c_void_p()
        with _host.on_device(self.device):
            _lib.check(self._lib.ac_stream_create(mdct._plan(self.device), self.B, self.C, ctypes.byref(handle)))
        self._handle = handle
        self._graphs = {}       # run(..., graph=True): captured calls by input buffers and arguments
        self._conceal = None    # decode_packed_chunk(lost=...) where it is composed: (carried codes, sf, gap), None = no source
        # decode_packed_chunk(redundant_at=...) synthesises one frame behind its rows ("Streams"):
        # _delayed from the first such chunk, _advanced from the first other call that moved the synthesis, until reset()
        self._delayed = self._advanced = False

    def close(self):
        self._graphs = {}       # (the graphs hold launches that address the stream's state)
        if self._handle is not None:
            self._lib.ac_stream_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._conceal = None
        self._delayed = self._advanced = False
        with _host.on_device(self.device):
            _lib.check(self._lib.ac_stream_reset(self._handle, _host.stream_ptr(self.device)))

    def _check_chunk(self, x, name, ndim, dtype=None):
        if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
            raise ValueError("%s requires a gradient: the streaming calls keep state on the device and are not "
                             "differentiable -- use MDCTransformer.transform / inverse_transform" % name)
        x = _host.check_device_tensor(x, name, self.mdct.compute_dtype if dtype is None else dtype, ndim)
        if x.device != self.device:
            raise ValueError("%s lives on %s but the stream's state lives on %s" % (name, x.device, self.device))
        return x

    def _blocks(self, x):
        """k of a checked PCM chunk x [B, k*N, C] of this stream's B and C."""
        B, S, C = x.shape
        N = self.mdct.filters_n
        if (B, C) != (self.B, self.C) or S % N != 0:
            raise ValueError("x_chunk must be [%d, k*%d, %d], got %s" % (self.B, N, self.C, tuple(x.shape)))
        return S // N

    def _out(self, out, name, shape, like, stream=None, dtype=None):
        """``out``, checked, or a new tensor on ``like``'s device, of ``dtype`` (default: ``like``'s)."""
        dtype, device = like.dtype if dtype is None else dtype, like.device
        if out is None:
            # the allocator's pool (and reuse order) of the stream the work runs on; no test can assert this (only a reuse of
            # freed memory by another stream's work would show it): the class docstring states the rule
            if stream is not None:
                with torch.cuda.stream(stream):
                    return torch.empty(shape, dtype=dtype, device=device)
            return torch.empty(shape, dtype=dtype, device=device)
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype \
                or out.device != device or not out.is_contiguous() or out.data_ptr() % 16 != 0:
            raise ValueError("%s must be a contiguous, 16-byte aligned %s tensor of shape %s on %s"
                             % (name, dtype, tuple(shape), device))
        return out

    def _stream(self, stream):
        return _host.stream_ptr(self.device) if stream is None else ctypes.c_void_p(stream.cuda_stream)

    def transform_chunk(self, x_chunk, out=None, stream=None):
        """x_chunk [B, k*N, C] -> X [B, k, N, C].  ``stream``: a ``torch.cuda.Stream`` to enqueue on (default: the
        current stream)."""
        x = self._check_chunk(x_chunk, "x_chunk", 3)
        B, N, C, k = self.B, self.mdct.filters_n, self.C, self._blocks(x)
        X = self._out(out, "out", (B, k, N, C), x, stream)
        with _host.on_device(x.device):
            _lib.check(self._lib.ac_stream_encode_typed(self._handle, None, _host.ptr(x), _host.ptr(X), None, None, 0.0,
                                                        self.mdct._dtype_id, k, self._stream(stream)))
        return X

    def encode_chunk(self, x_chunk, drown=0.0, out=None, stream=None):
        """x_chunk [B, k*N, C] -> (X [B, k, N, C], tonality [B, k, 1, C], threshold [B, k, N, C]) of the chunk's frames
        (``ac_stream_encode``: MDCT, tonality and masking threshold in one launch where the wave-level kernels apply).
        ``out``: optional tuple of three tensors to write into."""
        if self.psy is None:
            raise ValueError("this stream was created without a masking model (psy=...)")
        x = self._check_chunk(x_chunk, "x_chunk", 3)
        B, N, C, k = self.B, self.mdct.filters_n, self.C, self._blocks(x)
        o = out if out is not None else (None, None, None)
        X = self._out(o[0], "out[0]", (B, k, N, C), x, stream)
        t = self._out(o[1], "out[1]", (B, k, 1, C), x, stream)
        thr = self._out(o[2], "out[2]", (B, k, N, C), x, stream)
        with _host.on_device(x.device):
            _lib.check(self._lib.ac_stream_encode_typed(self._handle, self.psy._plan(x.device), _host.ptr(x), _host.ptr(X),
                                                        _host.ptr(t), _host.ptr(thr), float(drown), self.mdct._dtype_id, k,
                                                        self._stream(stream)))
        return X, t, thr

    def run(self, x, blocks_per_chunk, masking=True, synthesis=True, drown=0.0, graph=False):
        """A long device-resident signal ``x [1, K*N, C]`` (or a list of chunk tensors ``[B, k*N, C]``) through the stream
        in chunks of ``blocks_per_chunk`` blocks with one library call (``ac_stream_run``: launches issued from C; with
        ``synthesis`` and chunks small enough to be latency-bound, the analysis of chunk i + 1 and the synthesis of chunk i
        share one launch).  Returns ``(X, t, thr, xhat)`` -- tensors ``[1, K, ...]`` for
        a tensor input, lists of per-chunk tensors for a list input; ``t`` / ``thr`` are None without ``masking``,
        ``xhat`` is None without ``synthesis``.  The last chunk of a tensor input may be shorter.

        ``graph=True``: the launches of the call are captured into a HIP graph the first time these input buffers (same
        addresses, shapes and arguments) are seen, and replayed from then on -- the gaps between the dependent launches
        go (one stereo clip in chunks of 256 blocks: 7.9 us per chunk against 11.9).  A replay reads the CURRENT contents
        of the same input buffers and overwrites the output tensors of the first call, which are returned again."""
        _host.require_float32(self.mdct.compute_dtype, "StreamingMDCT.run (use the chunk calls for bfloat16 / float64 streams)")
        self._not_delayed("run")
        self._conceal = None    # (the synthesis state moves on without a source for concealment)
        if graph:
            out = self._run_graph(x, blocks_per_chunk, masking, synthesis, drown)
        else:
            out = self._run(x, blocks_per_chunk, masking, synthesis, drown)
        self._advanced = self._advanced or bool(synthesis)   # (only once the library call has gone through)
        return out

    def _run(self, x, blocks_per_chunk, masking, synthesis, drown):
        k, N = int(blocks_per_chunk), self.mdct.filters_n
        if masking and self.psy is None:
            raise ValueError("this stream was created without a masking model (psy=...)")
        if k < 1:
            raise ValueError("blocks_per_chunk must be positive")
        as_list = isinstance(x, (list, tuple))
        if as_list:
            xs = [self._check_chunk(c, "x[%d]" % i, 3) for i, c in enumerate(x)]
            for c in xs:
                if tuple(c.shape) != (self.B, k * N, self.C):
                    raise ValueError("every chunk must be [%d, %d, %d], got %s" % (self.B, k * N, self.C, tuple(c.shape)))
            groups = [(xs, k)]
            like = xs[0] if xs else None
        else:
            xt = self._check_chunk(x, "x", 3)
            B, S, C = xt.shape
            if B != 1 or self.B != 1 or C != self.C or S % N != 0:
                raise ValueError("a tensor input must be [1, K*%d, %d] on a stream of one clip (pass a list of chunks "
                                 "otherwise), got %s" % (N, self.C, tuple(xt.shape)))
            K = S // N
            full, rest = K // k, K % k
            like = xt
            if (k * N * C * 4) % 16 != 0 and K > k:
                # chunk boundaries inside one tensor would not be 16-byte aligned (filters_n * channels_n odd multiples of
                # 2): per-chunk tensors through the list form, concatenated afterwards
                parts = [xt[:, i * k * N:(i + 1) * k * N].clone() for i in range(full)]
                o = self.run(parts, k, masking=masking, synthesis=synthesis, drown=drown) if full else ([], [], [], [])
                if rest:
                    r = self.run([xt[:, full * k * N:].clone()], rest, masking=masking, synthesis=synthesis, drown=drown)
                    o = tuple((a or []) + (b or []) if (a is not None or b is not None) else None for a, b in zip(o, r))
                cat = lambda ts: torch.cat(ts, dim=1) if ts else None   # noqa: E731
                return cat(o[0]), cat(o[1]) if masking else None, cat(o[2]) if masking else None, \
                    cat(o[3]) if synthesis else None
            Xall = torch.empty((1, K, N, C), dtype=xt.dtype, device=xt.device)
            tall = torch.empty((1, K, 1, C), dtype=xt.dtype, device=xt.device) if masking else None
            thrall = torch.empty_like(Xall) if masking else None
            xhall = torch.empty_like(xt) if synthesis else None
            groups = []
            if full:
                groups.append(([xt[:, i * k * N:(i + 1) * k * N] for i in range(full)], k))
            if rest:
                groups.append(([xt[:, full * k * N:]], rest))
        outs = ([], [], [], [])
        pos = 0
        for chunks, kk in groups:
            n = len(chunks)
            if n == 0:
                continue
            if as_list:
                Xc = [torch.empty((self.B, kk, N, self.C), dtype=like.dtype, device=like.device) for _ in range(n)]
                tc = [torch.empty((self.B, kk, 1, self.C), dtype=like.dtype, device=like.device) for _ in range(n)] if masking else None
                thc = [torch.empty_like(v) for v in Xc] if masking else None
                xhc = [torch.empty_like(c) for c in chunks] if synthesis else None
            else:
                Xc = [Xall[:, pos + i * kk: pos + (i + 1) * kk] for i in range(n)]
                tc = [tall[:, pos + i * kk: pos + (i + 1) * kk] for i in range(n)] if masking else None
                thc = [thrall[:, pos + i * kk: pos + (i + 1) * kk] for i in range(n)] if masking else None
                xhc = [xhall[:, (pos + i * kk) * N: (pos + (i + 1) * kk) * N] for i in range(n)] if synthesis else None
            arr = lambda ts: (ctypes.c_void_p * n)(*[v.data_ptr() for v in ts]) if ts is not None else None   # noqa: E731
            with _host.on_device(self.device):
                _lib.check(self._lib.ac_stream_run(self._handle, self.psy._plan(self.device) if masking else None, n, kk,
                                                   arr(chunks), arr(Xc), arr(tc), arr(thc), arr(xhc), float(drown),
                                                   _host.stream_ptr(self.device)))
            for o, v in zip(outs, (Xc, tc, thc, xhc)):
                if v is not None:
                    o.extend(v)
            pos += n * kk
        if as_list:
            return outs[0], (outs[1] if masking else None), (outs[2] if masking else None), (outs[3] if synthesis else None)
        return Xall, tall, thrall, xhall

    def _run_graph(self, x, blocks_per_chunk, masking, synthesis, drown):
        chunks = list(x) if isinstance(x, (list, tuple)) else [x]
        for c in chunks:
            self._check_chunk(c, "x", 3)
        key = (tuple((c.data_ptr(), tuple(c.shape)) for c in chunks), isinstance(x, (list, tuple)), int(blocks_per_chunk),
               bool(masking), bool(synthesis), float(drown))
        hit = self._graphs.get(key)
        # a captured call addresses the stream's HOME state buffers; chunk calls (and reset) since the last run() may have
        # left the current state in the other buffer of the pair: move it home first (no device work when it is there)
        with _host.on_device(self.device):
            _lib.check(self._lib.ac_stream_settle(self._handle, _host.stream_ptr(self.device)))
        if hit is None:
            with _host.on_device(self.device):
                self.mdct._plan(self.device)                       # plans are built outside the capture
                if masking:
                    if self.psy is None:
                        raise ValueError("this stream was created without a masking model (psy=...)")
                    self.psy._plan(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    outs = self.run(x, blocks_per_chunk, masking=masking, synthesis=synthesis, drown=drown)
            while len(self._graphs) >= 8:                         # a graph keeps its outputs alive: a handful at most
                self._graphs.pop(next(iter(self._graphs)))
            hit = self._graphs[key] = (g, outs, chunks)            # (the inputs stay alive with their graph)
        hit[0].replay()
        return hit[1]

    def _not_delayed(self, what):
        if self._delayed:
            raise ValueError("%s on a stream that decodes recovering chunks (decode_packed_chunk(..., redundant_at=)), which "
                             "run one frame behind their rows: flush_packed() or reset() first" % what)

    def inverse_chunk(self, X_chunk, out=None, stream=None):
        """X_chunk [B, k, N, C] -> x [B, k*N, C]."""
        self._not_delayed("inverse_chunk")
        x = self._inverse_chunk(X_chunk, out, stream)
        if x.shape[1]:
            self._advanced = True
        return x

    def _inverse_chunk(self, X_chunk, out, stream):
        """:meth:`inverse_chunk` without the check of the stream's mode: also the last step of the composed recovering chunk."""
        X = self._check_chunk(X_chunk, "X_chunk", 4)
        B, k, N, C = X.shape
        if (B, C, N) != (self.B, self.C, self.mdct.filters_n):
            raise ValueError("X_chunk must be [%d, k, %d, %d], got %s" % (self.B, self.mdct.filters_n, self.C,
                                                                         tuple(X.shape)))
        x = self._out(out, "out", (B, k * N, C), X, stream)
        self._conceal = None    # (as the library does: a chunk that does not conceal leaves no source)
        with _host.on_device(X.device):
            _lib.check(self._lib.ac_stream_inverse_typed(self._handle, _host.ptr(X), _host.ptr(x), self.mdct._dtype_id, k,
                                                         self._stream(stream)))
        return x

    # ---- packed rows at a bitrate, chunk by chunk (extension; DESIGN.md section 8b, "Packed rows in a stream") -----
    def _packed_ready(self, what, budget):
        _host.require_float32(self.mdct.compute_dtype, "StreamingMDCT.%s" % what)
        if self.psy is None:
            raise ValueError("this stream was created without a masking model (psy=...)")
        if budget and self.psy.row_budget is None:
            raise ValueError("%s needs a stream with a row budget: make it from a codec of with_bitrate() or "
                             "with_row_budget() (codec.stream(...))" % what)

    def _on(self, stream):
        return torch.cuda.stream(stream) if stream is not None else _host._NO_SWITCH

    @property
    def row_bytes(self):
        """Bytes of a row's slot in :meth:`encode_packed_rows_chunk`'s data; None without a row budget."""
        if self.psy is None or self.psy.row_budget is None:
            return None
        return (self.psy.row_budget[0] + 31) // 32 * 4

    def packed_chunk_launches(self, decode=False, *, conceal=False, recover=False, pcm16=False):
        """Library launches of :meth:`encode_packed_rows_chunk` (``decode=True``: of :meth:`decode_packed_chunk`) on this
        stream (``ac_stream_packed_launches``): 1 = one launch that carries the overlap state -- filters_n = 1024, 64 bands,
        mono / stereo, a budget of at most ``_lib.AC_PACK_ROWS_MAX_BITS``, and for the encode a kernel instance that passed
        the register gate (stereo with ``spreading="f32"`` did not) -- else the launches of the composition (everywhere
        while ``AC_ENCODE_PACKED_NOFUSE=1`` / ``AC_DECODE_PACKED_NOFUSE=1`` is set: read per call).  0 for the encode on a
        stream without a row budget.  ``pcm16=True``: of the encode on a ``torch.int16`` chunk
        (``ac_stream_packed_launches_pcm16``; its instances passed the gate with ``spreading="bf16x2_mfma"`` only).
        ``decode=True, conceal=True``: of :meth:`decode_packed_chunk` with ``lost`` given -- 1 wherever the plain decode is
        1, else the 3 library launches of its composition.  ``recover=True`` beside them: of the recovering chunk
        (``redundant_at`` given; ``ac_stream_packed_launches(s, psy, 3)``), 1 and 3 in the same places."""
        self._packed_ready("packed_chunk_launches", False)
        if recover and not conceal:
            raise ValueError("recover=True is a form of the concealing decode: pass decode=True, conceal=True")
        if conceal:
            if not decode:
                raise ValueError("conceal=True is a form of the decode: pass decode=True")
            return int(self._lib.ac_stream_packed_launches(self._handle, self.psy._plan(self.device), 3 if recover else 2))
        if pcm16 and not decode:
            return int(self._lib.ac_stream_packed_launches_pcm16(self._handle, self.psy._plan(self.device)))
        return int(self._lib.ac_stream_packed_launches(self._handle, self.psy._plan(self.device), 1 if decode else 0))

    def encode_packed_rows_chunk(self, x_chunk, drown=0.0, stream=None):
        """On a stream of a codec made by ``with_bitrate()`` / ``with_row_budget()``: x_chunk [B, k*N, C] (float32, or
        ``torch.int16`` PCM read as ``pcm / 32768``: the rows, and the state left, of that float32 chunk) -> (data uint8
        [B*k*C*row_bytes], index int64 [B, k, C], fits bool [B, k, C]) -- the rows ``AudioCodec.encode_packed_rows`` gives
        for the chunk's frames of the whole signal, byte for byte: frame ``f`` of the chunk is frame (blocks so far + f),
        ``index[b, f, c] = ((b*k + f)*C + c) * row_bytes``.  The overlap state advances as under :meth:`encode_chunk`, so
        the chunk calls of every form may follow each other.  One launch where :meth:`packed_chunk_launches` is 1
        (``pcm16=True`` for int16; elsewhere an int16 chunk is converted and takes the float32 path), else
        :meth:`encode_chunk`, ``psy.quantize_to_budget`` and the packer: the same bytes.  Only enqueues, on ``stream`` or
        the current stream; float32 only, not differentiable."""
        self._packed_ready("encode_packed_rows_chunk", True)
        rb = self.row_bytes
        with self._on(stream):
            pcm16 = isinstance(x_chunk, torch.Tensor) and x_chunk.dtype == torch.int16
            x = self._check_chunk(x_chunk, "x_chunk", 3, torch.int16 if pcm16 else None)
            k, dev = self._blocks(x), x.device
            shape = (self.B, k, self.C)
            if 0 in shape:
                return _rows.outputs(shape, rb, dev)
            psy = self.psy._plan(dev)
            if pcm16 and self._lib.ac_stream_packed_launches_pcm16(self._handle, psy) != 1:
                x, pcm16 = x.to(torch.float32) / 32768, False
            if pcm16 or self._lib.ac_stream_packed_launches(self._handle, psy, 0) == 1:
                data, index, fits = _rows.outputs(shape, rb, dev)
                out = _lib.PackedOut(data.data_ptr(), rb, fits.data_ptr())
                with _host.on_device(dev):
                    _lib.check(self._lib.ac_stream_encode_typed(self._handle, psy, _host.ptr(x), ctypes.addressof(out), None,
                                                                None, float(drown),
                                                                _lib.AC_PACKED | (_lib.AC_IN_PCM16 if pcm16 else 0), k,
                                                                self._stream(stream)))
                return data, index, fits
            X, _, thr = self.encode_chunk(x, drown, stream=stream)
            index = _rows.row_starts(shape, rb, dev)
            data, fits = _rows.pack_rows_of_spectra(self.psy, X, thr, index, rb)
            return data, index, fits

    def decode_packed_chunk(self, data, index, pcm16=False, out=None, stream=None, *, lost=None, max_age=8, redundant_at=None):
        """data uint8 [nbytes], index int64 [B, k, C] -> x [B, k*N, C] (``torch.int16`` with ``pcm16=True``): the next k
        blocks of the signal, bit-equal to ``inverse_chunk(psy.dequantize(*psy.unpack(data, index)))`` -- with ``pcm16``
        through the store of ``AudioCodec.decode``: ``0 if NaN else clamp(rint(fp32(32768 * x)), -32768, 32767)``.
        ``index`` may hold any row starts and damaged rows read as ``psy.unpack`` reads them.  One launch where
        ``packed_chunk_launches(decode=True)`` is 1, else that composition.  Only enqueues, on ``stream`` or the current
        stream; float32 only.

        ``lost`` uint8 / bool [B, k, C] marks rows that did not arrive, and they are concealed as
        ``AudioCodec.decode_packed(..., lost=, max_age=)`` conceals them, with the last row that
        arrived carried from chunk to chunk: however a signal is split into chunks, the outputs are the blocks of that
        one-shot call on the whole signal, bit for bit; each row takes the ``max_age`` of its own call.  The carried row
        is the stream's state: :meth:`reset`, and every chunk that is decoded or inverted without ``lost``, leave no
        source behind.  One launch where ``packed_chunk_launches(decode=True, conceal=True)`` is 1, else the
        composition with the same state kept in tensors.

        ``redundant_at`` (with ``lost``; an int in [1, 2^31), DESIGN.md section 8g, "Streams") recovers before it conceals,
        as ``AudioCodec.decode_packed(..., redundant_at=)`` does, and for that the stream is *delayed*: the k blocks
        returned are the frames of ``D, row 0, ..., row k-2``, where ``D`` is the deferred last row of the chunk before (on
        a new or reset stream: a lost row with no source before it), and the chunk's last row waits for the next call.
        So the successor of every frame is in the chunk in hand: a lost frame whose successor arrived is read from
        ``index[b, successor, c] + redundant_at`` with no fade, every other frame as under ``lost`` alone.  However
        ``index [B, K', C]`` is split into chunks, the outputs are blocks ``[0, K')`` of the one-shot call on
        ``cat(index[:, :1], index)`` and ``cat(ones, lost)`` -- one lost frame in front -- bit for bit, and
        :meth:`flush_packed` returns block ``K'``.  A stream is delayed from its first such chunk until :meth:`reset`: in
        between :meth:`inverse_chunk`, :meth:`run` and this call without ``redundant_at`` raise ``ValueError`` and leave
        the state alone, as does a recovering chunk on a stream whose synthesis one of those has advanced since it was
        made or reset.  One launch where ``packed_chunk_launches(decode=True, conceal=True, recover=True)`` is 1, else
        the composition."""
        self._packed_ready("decode_packed_chunk", False)
        N = self.mdct.filters_n
        if redundant_at is not None:
            if lost is None:
                raise ValueError("redundant_at without lost: a row is recovered only where lost marks it")
            redundant_at = self.psy._check_redundant_at(redundant_at)
        with self._on(stream):
            if lost is not None:
                max_age = self.psy._check_max_age(max_age)
            data = self.psy._check_quant_tensor(data, "data", torch.uint8, ndim=1)
            if data.device != self.device:
                raise ValueError("data lives on %s but the stream's state lives on %s" % (data.device, self.device))
            index = self.psy._check_quant_tensor(index, "index", torch.int64, device=data.device, ndim=3)
            if lost is not None:
                lost = self.psy._check_lost(lost, index)
            B, k, C = index.shape
            if (B, C) != (self.B, self.C):
                raise ValueError("index must be [%d, k, %d], got %s" % (self.B, self.C, tuple(index.shape)))
            x = self._out(out, "out", (B, k * N, C), data, stream, dtype=torch.int16 if pcm16 else torch.float32)
            if k == 0:
                return x
            psy = self.psy._plan(data.device)
            if redundant_at is None:
                self._not_delayed("decode_packed_chunk without redundant_at")
            elif self._advanced:
                raise ValueError("redundant_at on a stream whose synthesis has advanced without it since it was made or "
                                 "reset: a recovering chunk runs one frame behind its rows -- reset() first")
            # the form ac_stream_packed_launches asks about: the plain, the concealing or the recovering decode
            if self._lib.ac_stream_packed_launches(self._handle, psy, 1 if lost is None else 2 if redundant_at is None else 3) == 1:
                self._conceal = None   # (a plain chunk leaves no source; of the others the state lives in the library from here on)
                rows = self._packed_in(data, index, psy, pcm16, lost, max_age, redundant_at)   # (held until the call is back)
                with _host.on_device(data.device):
                    _lib.check(self._lib.ac_stream_inverse_typed(self._handle, ctypes.addressof(rows), _host.ptr(x),
                                                                 _lib.AC_PACKED | (_lib.AC_CONCEAL if lost is not None else 0), k,
                                                                 self._stream(stream)))
            elif lost is None:
                self._inverse_chunk_into(self.psy.dequantize(*self.psy.unpack(data, index)), x, pcm16, stream)
            else:
                self._decode_packed_chunk_composed(data, index, lost, max_age, redundant_at, pcm16, x, stream)
            if redundant_at is None:   # (the mode changes only once the chunk has gone through)
                self._advanced = True
            else:
                self._delayed = True
            return x

    @staticmethod
    def _packed_in(data, index, psy, pcm16, lost, max_age, redundant_at):
        """``ac_stream_packed_in`` of a checked chunk; with ``lost`` inside an ``ac_stream_packed_lost_in``, with
        ``redundant_at`` too an ``ac_stream_packed_recover_in``."""
        rows = _lib.StreamPackedIn(_rows.packed_rows(data, index), psy.value, 1 if pcm16 else 0)
        if lost is None:
            return rows
        if redundant_at is None:
            return _lib.StreamPackedLostIn(rows, lost.data_ptr(), max_age)
        return _lib.StreamPackedRecoverIn(rows, lost.data_ptr(), max_age | _lib.AC_CONCEAL_REDUNDANT, redundant_at)

    def _inverse_chunk_into(self, X, x, pcm16, stream):
        """:meth:`inverse_chunk` of X into x, through the 16-bit PCM store where x is int16."""
        if not pcm16:
            return self._inverse_chunk(X, x, stream)
        p = torch.nan_to_num(self._inverse_chunk(X, None, stream) * 32768.0, nan=0.0)   # the float32 product
        x.copy_(p.round_().clamp_(-32768.0, 32767.0).to(torch.int16))                   # round: half to even
        return x

    def _decode_packed_chunk_composed(self, data, index, lost, max_age, redundant_at, pcm16, x, stream):
        """:meth:`decode_packed_chunk` with ``lost`` given (checked; under the stream the work runs on) where the library has
        no launch for it: the composition, which keeps the state the kernel keeps -- the carried row as ``psy.unpack`` read
        it, and the gap (frames since that row at the end of the chunk before; 32: none in reach) -- in ``self._conceal``.
        With ``redundant_at`` the chunk is the delayed one: its frames are the deferred row D -- the carried row where the gap
        is 0 -- and rows 0 .. k-2, and a lost frame whose successor arrived is the copy in the successor's slot.  Nothing
        here waits for the device."""
        B, k, C = index.shape
        dev = data.device
        if redundant_at is None:
            codes, sf = self.psy.unpack(data, index)
        else:   # the chunk's rows and, behind them, the copies their slots carry: the copy in row j's slot is of frame j - 1
            codes, sf = self.psy.unpack(data, torch.cat((index, index + redundant_at), dim=1))
            codes, red_codes, sf, red_sf = codes[:, :k], codes[:, k:], sf[:, :k], sf[:, k:]
        state = self._conceal
        if state is None:   # a new stream, after reset(), or after a chunk that did not conceal: no source (D did not arrive)
            state = (torch.zeros_like(codes[:, :1]), torch.zeros_like(sf[:, :1]),
                     torch.full((B, C), 32, dtype=torch.int64, device=dev))
        row_codes, row_sf, gap = state
        # the carried row in front of the chunk's rows; sources as DESIGN.md section 8f defines them
        codes_ext, sf_ext = torch.cat((row_codes, codes), dim=1), torch.cat((row_sf, sf), dim=1)
        f = torch.arange(k, dtype=torch.int64, device=dev).view(1, k, 1)
        if redundant_at is None:   # frame f is row f, frame f + 1 of codes_ext: the carried row is frame -1
            gone, recovered, ahead = lost != 0, None, 1
        else:                      # frame f is frame f of codes_ext: the carried row is frame 0 where it is D, else gap before it
            arrived = torch.cat(((gap == 0).view(B, 1, C), lost == 0), dim=1)              # [B, k+1, C]
            gone, recovered, ahead = ~arrived[:, :k], ~arrived[:, :k] & arrived[:, 1:], 0
        last = f.expand(B, k, C).masked_fill(gone, -1).cummax(dim=1).values   # the last frame <= f of the chunk that arrived
        inside = (last >= 0) & (f - last <= max_age)
        carried_age = gap.view(B, 1, C) + f + 1 if ahead else gap.view(B, 1, C) + f
        carried = ~inside & (gap.view(B, 1, C) <= 31) & (carried_age <= max_age)
        # two masks: muted frames have no source and become silence; unfaded frames (the muted and the recovered) take age 0
        muted = ~inside & ~carried
        if recovered is None:
            unfaded = muted
        else:
            muted = muted & ~recovered
            unfaded = muted | recovered
        src = torch.where(inside, last + 1 if ahead else last, torch.zeros_like(last))   # frame of codes_ext
        age = torch.where(inside, f - last, carried_age).masked_fill(unfaded, 0).to(torch.uint8)
        N, M = codes.shape[2], sf.shape[2]
        got_codes = codes_ext.gather(1, src.unsqueeze(2).expand(B, k, N, C)).masked_fill(muted.unsqueeze(2), 0)
        got_sf = sf_ext.gather(1, src.unsqueeze(2).expand(B, k, M, C)).masked_fill(muted.unsqueeze(2), 0)
        if recovered is not None:
            got_codes = torch.where(recovered.unsqueeze(2), red_codes, got_codes)
            got_sf = torch.where(recovered.unsqueeze(2), red_sf, got_sf)
        self._inverse_chunk_into(self.psy.dequantize(got_codes, self.psy.conceal_fade(got_sf, age)), x, pcm16, stream)
        # the state after the chunk, over its rows 0 .. k-1 whatever max_age was; final [B, C]: the last row that arrived, or -1
        final = last[:, -1] if redundant_at is None else f.expand(B, k, C).masked_fill(lost != 0, -1).max(dim=1).values
        has = final >= 0
        at = final.clamp(min=0).view(B, 1, 1, C)
        new_codes = torch.where(has.view(B, 1, 1, C), codes.gather(1, at.expand(B, 1, N, C)), row_codes)
        new_sf = torch.where(has.view(B, 1, 1, C), sf.gather(1, at.expand(B, 1, M, C)), row_sf)
        new_gap = torch.where(has, k - 1 - final, gap + k).clamp(max=32)
        self._conceal = (new_codes, new_sf, new_gap)   # (after the synthesis, which leaves no source)
        return x

    def flush_packed(self, pcm16=False, out=None, stream=None, *, max_age=8):
        """The last block of a delayed stream, x [B, N, C]: the frame of the deferred row, which no successor can recover
        any more -- concealed where it was lost.  Exactly ``decode_packed_chunk`` with ``redundant_at`` on one row marked
        lost, then :meth:`reset`: block ``K'`` of the one-shot call :meth:`decode_packed_chunk` names."""
        self._packed_ready("flush_packed", False)
        with self._on(stream):
            data = torch.zeros((16,), dtype=torch.uint8, device=self.device)
            index = torch.zeros((self.B, 1, self.C), dtype=torch.int64, device=self.device)
            lost = torch.ones((self.B, 1, self.C), dtype=torch.uint8, device=self.device)
        x = self.decode_packed_chunk(data, index, pcm16, out, stream, lost=lost, max_age=max_age, redundant_at=1)
        with self._on(stream):   # (reset() enqueues on the current stream: behind the chunk)
            self.reset()
        return x
