"""``encode()`` / ``decode()`` and the streaming overlap-add wrappers.

The reference has no ``encode``/``decode``; BASELINE.json's north star names them as the API surface,
and SURVEY.md section 0 item 3 defines them as thin compositions of the reference's methods:

    encode(x)  = transform -> tonality -> global_masking_threshold   (one fused HIP pass over the PCM)
    decode(X)  = inverse_transform
"""

from __future__ import annotations

import copy
import ctypes
import math
import os

import numpy as np
import torch

from . import _host, _lib, _rows, placement
from .mdctransformer import MDCTransformer
from .psychoacoustic import PsychoacousticModel
from .stream import ProtectStream, StreamingMDCT   # (their home is stream.py; they stay importable from here)


class AudioCodec:
    """MDCT analysis + psychoacoustic masking (encode) and MDCT synthesis (decode)."""

    def __init__(self, sample_rate=48000, filters_n=1024, bark_bands_n=64, alpha=0.6, window_type="vorbis",
                 compute_dtype=torch.float32, spreading=None, precompute_dtype=torch.float64):
        self.mdct = MDCTransformer(filters_n, window_type=window_type, compute_dtype=compute_dtype,
                                   precompute_dtype=precompute_dtype)
        self.psy = PsychoacousticModel(sample_rate, filter_bands_n=filters_n, bark_bands_n=bark_bands_n,
                                       alpha=alpha, compute_dtype=compute_dtype, precompute_dtype=precompute_dtype,
                                       spreading=spreading)
        self.filters_n = int(filters_n)
        self.compute_dtype = self.mdct.compute_dtype
        self.row_bits = None      # the row budget of a codec made by with_row_budget() / with_bitrate()
        self._red_codecs = {}     # protect_packed_rows' composition: with_row_budget(red_bits), kept per red_bits
        self._lib = _lib.load()

    def with_row_budget(self, row_bits, min_offset=0):
        """A codec at a constant bitrate: it shares ``mdct`` with this one and carries
        ``psy.with_row_budget(row_bits, min_offset)``.  On it :meth:`encode_quantized` and :meth:`encode_packed` give the
        codes and scale factors of ``encode_quantized_budget(x, row_bits, min_offset)`` -- in one launch where
        :meth:`encode_quantized_launches` is 1 -- and ``row_bits`` holds the budget.  :meth:`encode`, the ``decode*``
        methods, the explicit ``*_budget`` methods and autograd behave as on this codec.  ``row_bits``: an int, at least
        5 * bark_bands_n; ``min_offset`` in [-254, 254]; float32 only."""
        new = copy.copy(self)
        new.psy = self.psy.with_row_budget(row_bits, min_offset)
        new.row_bits = int(row_bits)
        new._red_codecs = {}      # its own: a dict shared with the copy would hold the copy in a reference cycle
        return new

    def with_bitrate(self, bits_per_second, min_offset=0):
        """:meth:`with_row_budget` at :meth:`row_bits_for_bitrate` of a per-channel bitrate."""
        return self.with_row_budget(self.row_bits_for_bitrate(bits_per_second), min_offset)

    def encode_launches(self, channels_n=2, device=None):
        """How many kernel launches :meth:`encode` takes for float32 tensors of ``channels_n`` channels on ``device``
        (``ac_encode_launches``): 1 = the fused kernels (filters_n 64 ... 2048 in powers of two, mono / stereo), 2 = transform +
        one masking-model pass, 3 = the generic kernels."""
        return self._launches(self._lib.ac_encode_launches, device, channels_n)

    def _launches(self, query, device, *counts, mdct=True):
        """A ``*_launches`` method's answer: ``query`` on the plans of ``device`` (both, or the masking model's alone) and the
        counts it takes."""
        dev = _host.default_device(device)
        plans = (self.mdct._plan(dev), self.psy._plan(dev)) if mdct else (self.psy._plan(dev),)
        return int(query(*plans, *[int(n) for n in counts]))

    def encode(self, x, drown=0.0):
        """x [B, K*N, C] -> (X [B,K+1,N,C], tonality [B,K+1,1,C], threshold [B,K+1,N,C]).

        ``x`` is float PCM in [-1, 1] (the reference's convention) or ``torch.int16`` PCM (extension: x = pcm / 32768
        is applied inside the kernel's loads, half the PCM bytes).  When ``x`` requires a gradient the same three results
        come from the differentiable entry points in sequence (transform, tonality, threshold: each carries its backward
        pass), as the reference's op chain is differentiable in a training graph; otherwise one fused launch."""
        if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
            X = self.mdct.transform(x)
            t = self.psy.tonality(X)
            return X, t, self.psy.global_masking_threshold(X, t, drown)
        pcm16 = isinstance(x, torch.Tensor) and x.dtype == torch.int16
        x = _host.check_device_tensor(x, "x", torch.int16 if pcm16 else self.compute_dtype, 3)
        B, S, C = x.shape
        N, K = self.filters_n, _host.blocks_of(x, self.filters_n)
        # the library allocates what it returns, and decides where: spectra and thresholds in different classes of VRAM
        # (audiocodec_amd/placement.py; plain torch.empty for small batches, other dtypes, AC_NO_PLACEMENT=1)
        placement.ensure(self, (B, S, C), x.device)
        X = placement.empty(placement.REGION_SPECTRA, (B, K + 1, N, C), self.compute_dtype, x.device)
        t = torch.empty((B, K + 1, 1, C), dtype=self.compute_dtype, device=x.device)
        thr = placement.empty(placement.REGION_OTHER, (B, K + 1, N, C), self.compute_dtype, x.device)
        self.encode_into(x, X, t, thr, drown)
        return X, t, thr

    def placement_report(self, device=None):
        """How the tensors :meth:`encode` / :meth:`decode` return are placed on ``device`` (``placement.report``)."""
        return placement.report(device)

    def encode_ex(self, x, drown=0.0, noise_seed=None, db_norm=False):
        """:meth:`encode` with its element-wise tail computed in the same pass (``ac_encode_fused_ex``):

        :param noise_seed: an int: also return ``X + thr * Normal(0, 1/6)`` -- the values
                           ``psy.add_noise(X, thr, seed=noise_seed)`` gives (reference ``psychoacoustic.py:150-167``)
        :param db_norm:    also return ``psy.amplitude_to_dB_norm(X)`` (``psychoacoustic.py:87-100``)
        :return: ``(X, tonality, threshold, noisy or None, db_norm or None)``
        """
        _host.require_float32(self.compute_dtype, "encode_ex")
        if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():   # the differentiable composition
            X, t, thr = self.encode(x, drown)
            return (X, t, thr, self.psy.add_noise(X, thr, seed=noise_seed) if noise_seed is not None else None,
                    self.psy.amplitude_to_dB_norm(X) if db_norm else None)
        x = _host.check_device_tensor(x, "x", self.compute_dtype, 3)
        B, _, C = x.shape
        N, K = self.filters_n, _host.blocks_of(x, self.filters_n)
        X = torch.empty((B, K + 1, N, C), dtype=x.dtype, device=x.device)
        t = torch.empty((B, K + 1, 1, C), dtype=x.dtype, device=x.device)
        thr = torch.empty_like(X)
        noisy = torch.empty_like(X) if noise_seed is not None else None
        dbn = torch.empty_like(X) if db_norm else None
        flags = (1 if noisy is not None else 0) | (2 if dbn is not None else 0)
        with _host.on_device(x.device):
            _lib.check(self._lib.ac_encode_fused_ex(
                self.mdct._plan(x.device), self.psy._plan(x.device), _host.ptr(x), _host.ptr(X), _host.ptr(t), _host.ptr(thr),
                float(drown), flags, _host.ptr(noisy) if noisy is not None else None,
                _host.ptr(dbn) if dbn is not None else None, (int(noise_seed) if noise_seed is not None else 0) & (2 ** 64 - 1),
                B, K, C, _host.stream_ptr(x.device)))
        return X, t, thr, noisy, dbn

    def _check_io(self, t, name, shape, dtype, device):
        """Caller-owned tensors go to the kernels as raw pointers: shape, dtype, device and contiguity must be exact."""
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
        if not t.is_cuda:
            raise RuntimeError("%s lives on %s: this package only runs on ROCm device tensors" % (name, t.device))
        if device is not None and t.device != device:
            raise ValueError("%s lives on %s but the input lives on %s" % (name, t.device, device))
        if t.dtype != dtype:
            raise ValueError("%s has dtype %s, expected %s" % (name, t.dtype, dtype))
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous (got strides %s for shape %s)" % (name, t.stride(), tuple(t.shape)))
        if t.data_ptr() % 16 != 0:
            raise ValueError("%s starts at an address that is not 16-byte aligned (a view into the middle of an "
                             "allocation?)" % name)
        if t.requires_grad and torch.is_grad_enabled():
            raise ValueError("%s requires a gradient: results written into caller-owned tensors carry none -- use "
                             "encode() / decode(), which are differentiable" % name)
        return t

    def encode_into(self, x, X, t, thr, drown=0.0):
        """Same as :meth:`encode` into caller-owned output tensors (no allocation in the timed path).  Every tensor
        must be a contiguous device tensor of exactly the shape :meth:`encode` would return; ``ValueError`` otherwise."""
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError("x must be a [batches_n, samples_n, channels_n] tensor")
        pcm16 = x.dtype == torch.int16
        if pcm16 and self.compute_dtype != torch.float32:
            raise ValueError("16-bit PCM input needs compute_dtype float32")
        self._check_io(x, "x", None, torch.int16 if pcm16 else self.compute_dtype, None)
        B, _, C = x.shape
        N, K = self.filters_n, _host.blocks_of(x, self.filters_n)
        self._check_io(X, "X", (B, K + 1, N, C), self.compute_dtype, x.device)
        self._check_io(t, "t", (B, K + 1, 1, C), self.compute_dtype, x.device)
        self._check_io(thr, "thr", (B, K + 1, N, C), self.compute_dtype, x.device)
        if self.compute_dtype != torch.float32:
            # float64: the three typed entry points in sequence; bfloat16: the fused wave-level kernel where it applies
            with _host.on_device(x.device):
                _lib.check(self._lib.ac_encode_fused_typed(
                    self.mdct._plan(x.device), self.psy._plan(x.device), _host.ptr(x), _host.ptr(X), _host.ptr(t),
                    _host.ptr(thr), float(drown), self.mdct._dtype_id, B, K, C, _host.stream_ptr(x.device)))
            return
        fn = self._lib.ac_encode_fused_pcm16 if pcm16 else self._lib.ac_encode_fused
        with _host.on_device(x.device):
            _lib.check(fn(self.mdct._plan(x.device), self.psy._plan(x.device), _host.ptr(x), _host.ptr(X), _host.ptr(t),
                          _host.ptr(thr), float(drown), B, K, C, _host.stream_ptr(x.device)))

    def workspace(self, batches_n, blocks_n, channels_n, **kwargs):
        """Caller-owned ``x, X, t, thr, xh`` tensors for batches of this shape, placed for the MI355X's HBM (see
        :class:`audiocodec_amd.workspace.Workspace`: on plain allocations the two kernels run up to 15 % slower when the
        tensors they stream side by side happen to share a class of VRAM stretches).  Use with :meth:`encode_into` /
        :meth:`decode_into`."""
        from .workspace import Workspace
        return Workspace(self, batches_n, blocks_n, channels_n, **kwargs)

    def stream(self, batches_n, channels_n, device=None):
        """A :class:`StreamingMDCT` over this codec's filter bank and masking model (chunked ``encode`` / ``decode`` with
        device-resident overlap state)."""
        return StreamingMDCT(self.mdct, batches_n, channels_n, device=device, psy=self.psy)

    def decode(self, X, pcm16=False):
        """X [B, K', N, C] -> x [B, (K'+1)*N, C]; ``pcm16=True`` returns ``torch.int16`` PCM, converted inside the kernel's
        stores: ``pcm = 0 if x is NaN else clamp(rint(fp32(32768 * x)), -32768, 32767)`` (``rint`` rounds half to even; +-Inf
        and products that overflow float32 go to the rail of their sign; a NaN sample decodes to silence)."""
        if not pcm16:
            return self.mdct.inverse_transform(X)
        X = _host.check_device_tensor(X, "X", self.compute_dtype, 4)
        B, Kp, N, C = X.shape
        if N != self.filters_n:
            raise ValueError("axis 2 of X (%d) != filters_n (%d)" % (N, self.filters_n))
        x = torch.empty((B, (Kp + 1) * N, C), dtype=torch.int16, device=X.device)
        self.decode_into(X, x)
        return x

    # ---- quantised spectra (extension) ------------------------------------------------
    def _encode_for_quantizer(self, x, drown, what):
        """X and the threshold of :meth:`encode` for the quantising method ``what``: float32 only, and no gradient."""
        _host.require_float32(self.compute_dtype, what)
        _host.refuse_gradient(x)
        X, _, thr = self.encode(x, drown)
        return X, thr

    def encode_quantized_launches(self, channels_n=2, device=None, *, pcm16=False):
        """Launches :meth:`encode_quantized` takes for float32 PCM of ``channels_n`` channels
        (``ac_encode_quantized_launches``): 1 = the fused encode quantises the frame in its registers (filters_n = 1024, mono /
        stereo, spreading ``"f32"`` or ``"bf16x2_mfma"``), 2 = :meth:`encode`, then the quantiser.  ``pcm16=True``: for
        ``torch.int16`` PCM (``ac_encode_quantized_launches_pcm16``)."""
        query = self._lib.ac_encode_quantized_launches_pcm16 if pcm16 else self._lib.ac_encode_quantized_launches
        return self._launches(query, device, channels_n)

    def encode_quantized(self, x, drown=0.0):
        """:meth:`encode`, then :meth:`PsychoacousticModel.quantize` on its X and threshold: x [B, K*N, C] (float or
        ``torch.int16`` PCM) -> (codes int16 [B, K+1, N, C], sf int8 [B, K+1, M, C]).  One launch that writes only codes and
        scale factors where :meth:`encode_quantized_launches` is 1 for ``x``'s format -- asked with ``pcm16=True`` for
        ``torch.int16`` (``ac_encode_fused_ex`` with ``AC_EMIT_CODES``, and ``AC_IN_PCM16`` for int16: the same values, bit
        for bit); elsewhere two launches with X, tonality and threshold as temporaries.  On a codec made by
        :meth:`with_row_budget` / :meth:`with_bitrate` the quantiser is ``quantize_to_budget`` at the codec's budget, in the
        same number of launches.  float32 only, not differentiable."""
        pcm16 = isinstance(x, torch.Tensor) and x.dtype == torch.int16
        if (self.compute_dtype == torch.float32 and isinstance(x, torch.Tensor) and (pcm16 or x.dtype == torch.float32)
                and x.is_cuda and x.dim() == 3 and not (x.requires_grad and torch.is_grad_enabled())
                and x.shape[1] % self.filters_n == 0
                and self.encode_quantized_launches(x.shape[2], x.device, pcm16=pcm16) == 1):
            x = _host.check_device_tensor(x, "x", x.dtype, 3)
            B, S, C = x.shape
            K = S // self.filters_n
            codes = torch.empty((B, K + 1, self.filters_n, C), dtype=torch.int16, device=x.device)
            sf = torch.empty((B, K + 1, self.psy.bark_bands_n, C), dtype=torch.int8, device=x.device)
            with _host.on_device(x.device):
                _lib.check(self._lib.ac_encode_fused_ex(
                    self.mdct._plan(x.device), self.psy._plan(x.device), _host.ptr(x), None, None, None, float(drown),
                    _lib.AC_EMIT_CODES | (_lib.AC_IN_PCM16 if pcm16 else 0), _host.ptr(codes), _host.ptr(sf), 0, B, K, C,
                    _host.stream_ptr(x.device)))
            return codes, sf
        X, thr = self._encode_for_quantizer(x, drown, "encode_quantized")
        return self.psy.quantize(X, thr)

    def decode_quantized_launches(self, channels_n=2, device=None):
        """Launches :meth:`decode_quantized` takes for ``channels_n`` channels (``ac_decode_quantized_launches``): 1 = the
        synthesis dequantises in its loads (filters_n 1024 / 2048, mono / stereo), 2 = dequantise, then :meth:`decode`."""
        return self._launches(self._lib.ac_decode_quantized_launches, device, channels_n)

    def decode_quantized(self, codes, sf, pcm16=False):
        """codes int16 [B, K', N, C], sf int8 [B, K', M, C] -> x [B, (K'+1)*N, C] (``torch.int16`` with ``pcm16=True``):
        bit-equal to ``decode(psy.dequantize(codes, sf), pcm16)``.  The 16-bit store is :meth:`decode`'s:
        ``pcm = 0 if x is NaN else clamp(rint(fp32(32768 * x)), -32768, 32767)`` -- overshoot of a lossy decode past full
        scale stops at the rails, and a band marked non-representable (``sf = -128``, NaN when dequantised) decodes to
        silence over the two blocks its frame covers.  float32 only."""
        _host.require_float32(self.compute_dtype, "decode_quantized")
        codes, sf = self.psy._check_codes(codes, sf)
        B, Kp, N, C = codes.shape
        dev = codes.device
        x, px, px16 = _host.pcm_out((B, (Kp + 1) * N, C), pcm16, dev)
        mdct, psy = self.mdct._plan(dev), self.psy._plan(dev)
        scratch = None
        if self._lib.ac_decode_quantized_launches(mdct, psy, C) != 1:
            scratch = torch.empty((B, Kp, N, C), dtype=torch.float32, device=dev)
        with _host.on_device(dev):
            _lib.check(self._lib.ac_decode_quantized(
                mdct, psy, _host.ptr(codes), _host.ptr(sf), px, px16,
                _host.ptr(scratch) if scratch is not None else None, B, Kp, C, _host.stream_ptr(dev)))
        return x

    def encode_packed(self, x, drown=0.0):
        """:meth:`encode_quantized`, then :meth:`PsychoacousticModel.pack`: x [B, K*N, C] -> (data uint8 [nbytes],
        index int64 [B, K+1, C]).  Synchronises with the device (``pack`` reads the byte count);
        float32 only, not differentiable."""
        codes, sf = self.encode_quantized(x, drown)
        return self.psy.pack(codes, sf)

    # ---- rate control (extension) ---------------------------------------------------------
    def row_bits_for_bitrate(self, bits_per_second):
        """The per-channel row budget of a bitrate: floor(bits_per_second * filters_n / sample_rate) bits per frame and
        channel (a frame advances filters_n samples).  Pass it to :meth:`encode_quantized_budget`."""
        if isinstance(bits_per_second, bool) or not isinstance(bits_per_second, (int, float, np.integer, np.floating)):
            raise TypeError("bits_per_second must be a number, got %s" % type(bits_per_second).__name__)
        if not bits_per_second > 0:
            raise ValueError("bits_per_second must be positive, got %r" % (bits_per_second,))
        return int(math.floor(bits_per_second * self.filters_n / self.psy.sample_rate))

    def encode_quantized_budget(self, x, row_bits, min_offset=0, drown=0.0):
        """:meth:`encode`, then :meth:`PsychoacousticModel.quantize_to_budget` on its X and threshold: x [B, K*N, C] ->
        (codes int16 [B, K+1, N, C], sf int8 [B, K+1, M, C], offset int16 [B, K+1, C], row_bits_out int32 [B, K+1, C]).
        ``row_bits`` is an int (e.g. :meth:`row_bits_for_bitrate`) or an int32 tensor [B, K+1, C].  Two launches; float32
        only, not differentiable."""
        X, thr = self._encode_for_quantizer(x, drown, "encode_quantized_budget")
        return self.psy.quantize_to_budget(X, thr, row_bits, min_offset)

    def encode_packed_budget(self, x, row_bits, min_offset=0, drown=0.0):
        """:meth:`encode_quantized_budget`, then :meth:`PsychoacousticModel.pack`: x [B, K*N, C] -> (data uint8 [nbytes],
        index int64 [B, K+1, C], offset int16 [B, K+1, C]).  A row that met its budget R takes at most ceil(R / 32) * 4
        bytes of ``data``; :meth:`decode_packed` reads the stream as it is.  Synchronises with the device; float32 only."""
        codes, sf, offset, _ = self.encode_quantized_budget(x, row_bits, min_offset, drown)
        data, index = self.psy.pack(codes, sf)
        return data, index, offset

    # ---- fixed-stride packed rows at a bitrate (extension; DESIGN.md section 8b, "packed rows") ------------------
    @property
    def row_bytes(self):
        """Bytes of a row's slot in :meth:`encode_packed_rows`' data: ceil(row_bits / 32) * 4; None without a row budget."""
        return None if self.row_bits is None else (self.row_bits + 31) // 32 * 4

    def encode_packed_rows_launches(self, channels_n=2, device=None, *, pcm16=False):
        """Library launches :meth:`encode_packed_rows` takes for float32 PCM of ``channels_n`` channels
        (``ac_encode_packed_launches``): 1 = the fused encode packs the frame's rows itself (where
        :meth:`encode_quantized_launches` is 1, bark_bands_n = 64 and the budget is at most ``_lib.AC_PACK_ROWS_MAX_BITS``),
        else :meth:`encode_launches` + 2: the encode, the budgeted quantiser and the packer (everywhere while
        ``AC_ENCODE_PACKED_NOFUSE=1`` is set: read per call).  0 on a codec without a row budget.  ``pcm16=True``: for
        ``torch.int16`` PCM (``ac_encode_packed_launches_pcm16``)."""
        query = self._lib.ac_encode_packed_launches_pcm16 if pcm16 else self._lib.ac_encode_packed_launches
        return self._launches(query, device, channels_n)

    def encode_packed_rows(self, x, drown=0.0):
        """On a codec made by :meth:`with_bitrate` / :meth:`with_row_budget`: x [B, K*N, C] (float32, or ``torch.int16``
        PCM read as ``pcm / 32768``: the bytes of the call on that float32 tensor) -> (data uint8
        [B*(K+1)*C*row_bytes], index int64 [B, K+1, C], fits bool [B, K+1, C]) -- every row in a slot of :attr:`row_bytes`
        bytes, ``index[b, f, c] = ((b*(K+1) + f)*C + c) * row_bytes``.  A slot holds the bytes
        :meth:`PsychoacousticModel.pack` writes for the row's codes and scale factors of :meth:`encode_quantized`, then zero
        bytes; a row longer than its slot (offset 254 reached with the budget unmet) is stored as the marked row -- every
        width 31, ``fits`` False -- and decodes as bands the quantiser could not represent.  :meth:`decode_packed` and
        :meth:`PsychoacousticModel.unpack` read ``(data, index)`` as they are.  One launch where
        :meth:`encode_packed_rows_launches` is 1 (``pcm16=True`` for int16), else the composition of the encode,
        ``quantize_to_budget`` and the packer: the same bytes.  The size of ``data`` is known before the call: it never
        synchronises with the device, only enqueues on the current stream, and can be captured in a graph.  float32 only,
        not differentiable."""
        _host.require_float32(self.compute_dtype, "encode_packed_rows")
        _rows.need_row_budget(self, "encode_packed_rows")
        _host.refuse_gradient(x)
        pcm16 = isinstance(x, torch.Tensor) and x.dtype == torch.int16
        x = _host.check_device_tensor(x, "x", torch.int16 if pcm16 else torch.float32, 3)
        B, _, C = x.shape
        N, K = self.filters_n, _host.blocks_of(x, self.filters_n)
        F, dev, rb = K + 1, x.device, self.row_bytes
        if B * F * C == 0:
            return _rows.outputs((B, F, C), rb, dev)
        mdct, psy = self.mdct._plan(dev), self.psy._plan(dev)
        if (self._lib.ac_encode_packed_launches_pcm16 if pcm16 else self._lib.ac_encode_packed_launches)(mdct, psy, C) == 1:
            data, index, fits = _rows.outputs((B, F, C), rb, dev)
            out = _lib.PackedOut(data.data_ptr(), rb, fits.data_ptr())
            with _host.on_device(dev):
                _lib.check(self._lib.ac_encode_fused_ex(mdct, psy, _host.ptr(x), None, None, None, float(drown),
                                                        _lib.AC_EMIT_PACKED | (_lib.AC_IN_PCM16 if pcm16 else 0),
                                                        ctypes.addressof(out), None, 0, B, K, C, _host.stream_ptr(dev)))
            return data, index, fits
        # the composition: encode_quantized_budget's codes, scale factors and row lengths (on plain allocations: nothing
        # here may wait for the device), rows longer than their slot marked, then the packer at the fixed row starts
        X = torch.empty((B, F, N, C), dtype=torch.float32, device=dev)
        t = torch.empty((B, F, 1, C), dtype=torch.float32, device=dev)
        thr = torch.empty_like(X)
        self.encode_into(x, X, t, thr, drown)
        index = _rows.row_starts((B, F, C), rb, dev)
        data, fits = _rows.pack_rows_of_spectra(self.psy, X, thr, index, rb)
        return data, index, fits

    # ---- transrating packed rows (extension) ----------------------------------------------
    def transrate_packed_rows_launches(self, channels_n=2, device=None):
        """Library launches :meth:`transrate_packed_rows` takes for rows of ``channels_n`` channels
        (``ac_transrate_launches``): 1 = one kernel reads, requantises and packs each row (filters_n = 1024, bark_bands_n =
        64, a budget of at most ``_lib.AC_PACK_ROWS_MAX_BITS``; any channel count), else 3: :meth:`PsychoacousticModel.unpack`,
        :meth:`PsychoacousticModel.requantize_to_budget` and the packer (everywhere while ``AC_TRANSRATE_NOFUSE=1`` is set:
        read per call).  0 on a codec without a row budget."""
        return self._launches(self._lib.ac_transrate_launches, device, channels_n, mdct=False)

    def transrate_packed_rows(self, data, index, return_offset=False):
        """On a codec made by :meth:`with_bitrate` / :meth:`with_row_budget`: packed rows at a higher bitrate -> the same
        frames at this codec's, without decoding.  data uint8 [nbytes], index int64 [B, F, C] -> (data' uint8
        [B*F*C*row_bytes], index' int64 [B, F, C], fits' bool [B, F, C]), and offset int16 [B, F, C] with
        ``return_offset=True`` -- the fixed-stride layout of :meth:`encode_packed_rows`.

        ``index`` holds any row starts: :meth:`encode_packed` output, the rows of :meth:`encode_packed_rows`, a slice of
        frames, a chunk's rows of ``encode_packed_rows_chunk``; rows are read as :meth:`PsychoacousticModel.unpack` reads them,
        damaged ones included.  Each row's stored scale factors are raised by the smallest offset in [0, 254] at which the
        row is at most ``row_bits`` long and its codes are quantised again at those steps
        (:meth:`PsychoacousticModel.requantize_to_budget`): a row that fits already keeps its fields.  The masking model,
        the filter bank and the frame grid are untouched; the codec's own ``min_offset`` is not used (it is relative to a
        threshold the rows no longer carry).  A row longer than its slot at offset 254 is stored as the marked row, ``fits``
        False.  ``fits`` reports only whether this call's row fitted: a marked input row comes out as the same marked
        bytes with ``fits`` True.  One launch where :meth:`transrate_packed_rows_launches` is 1, else the composition: the
        same bytes.  The size of ``data'`` is known before the call: it never synchronises with the device, only enqueues on
        the current stream, and can be captured in a graph.  Raising a bitrate is not possible.  float32 only."""
        _host.require_float32(self.compute_dtype, "transrate_packed_rows")
        _rows.need_row_budget(self, "transrate_packed_rows")
        data, index = _rows.check_pair(self.psy, data, index)
        dev, rb = data.device, self.row_bytes
        if index.numel() == 0 or self._lib.ac_transrate_launches(self.psy._plan(dev), index.shape[2]) == 1:
            out = _rows.outputs(tuple(index.shape), rb, dev, return_offset)
            return _rows.repack(self, _rows.packed_rows(data, index), 0, out, rb) if index.numel() else out
        # the composition: the rows unpacked, requantised at the budget from offset 0, rows longer than their slot marked, then
        # the packer at the fixed row starts (on plain allocations: nothing here may wait for the device)
        codes, sf = self.psy.unpack(data, index)
        return _rows.pack_quantized(self.psy, self.psy.requantize_to_budget(codes, sf, self.row_bits, 0), rb, return_offset)

    # ---- mixing the packed rows of several sources (extension) ----------------------------
    def mix_packed_rows_launches(self, channels_n=2, device=None, *, sources_n):
        """Library launches :meth:`mix_packed_rows` takes for ``sources_n`` sources of ``channels_n`` channels
        (``ac_mix_launches``): 1 = one kernel reads, sums, quantises and packs each row (where
        :meth:`transrate_packed_rows_launches` is 1 and ``sources_n`` is at most ``_lib.AC_MIX_MAX_SOURCES``), else
        ``2 * sources_n + 2``: :meth:`PsychoacousticModel.unpack` and ``dequantize`` per source, ``quantize_to_budget`` and the
        packer (everywhere while ``AC_MIX_NOFUSE=1`` is set: read per call).  0 on a codec without a row budget."""
        return self._launches(self._lib.ac_mix_launches, device, channels_n, sources_n, mdct=False)

    def mix_packed_rows(self, sources, gains=None, active=None, return_offset=False):
        """On a codec made by :meth:`with_bitrate` / :meth:`with_row_budget`: the packed rows of several sources of this
        codec on one frame grid -> their sum at this codec's bitrate, without decoding (the MDCT is linear).  ``sources``: a
        list of S >= 1 pairs (data uint8 [nbytes_i], index int64 [B, F, C]), every index of the same shape on one device ->
        (data' uint8 [B*F*C*row_bytes], index' int64 [B, F, C], fits' bool [B, F, C]), and offset int16 [B, F, C] with
        ``return_offset=True`` -- the fixed-stride layout of :meth:`encode_packed_rows`.

        Every ``index`` holds any row starts, read as :meth:`PsychoacousticModel.unpack` reads them, damaged rows included:
        :meth:`encode_packed` output, fixed-stride rows of any stride, protected slots, slices and a stream's chunks may be
        mixed with each other.  ``gains``: S ints in [-254, 254] in scale-factor units (one is 2^(1/4), 1.505 dB; default 0);
        ``active``: uint8 / bool [S, B, F, C] on the device, 0 = the row is never read and adds nothing (a silent participant,
        a lost row; default all 1).  The rules are :meth:`PsychoacousticModel.mix_to_budget`'s at this codec's ``row_bits``:
        where sources overlap in a band the coarsest of their steps is where the search starts.  A sum that passes +-32767
        codes at offset 0 clamps there and its 16-bit widths raise the offset.  With one source and gain 0 the result is
        :meth:`transrate_packed_rows`'.  A row longer than its slot at offset 254 is stored as the marked row, ``fits`` False.
        One launch where :meth:`mix_packed_rows_launches` is 1, else the composition on ``unpack``, ``mix_to_budget`` and the
        packer: the same bytes.  It never synchronises with the device, only enqueues on the current stream, and can be
        captured in a graph.  float32 only."""
        _host.require_float32(self.compute_dtype, "mix_packed_rows")
        _rows.need_row_budget(self, "mix_packed_rows")
        sources = list(sources)
        if not sources:
            raise ValueError("mix_packed_rows needs at least one source")
        S = len(sources)
        gains = self.psy._check_gains(gains, S)
        pairs, shape, dev = _rows.check_sources(self.psy, sources)
        active = self.psy._check_active(active, S, shape, dev)
        rows, rb = pairs[0][1].numel(), self.row_bytes
        if rows == 0 or self._lib.ac_mix_launches(self.psy._plan(dev), shape[2], S) == 1:
            out = _rows.outputs(shape, rb, dev, return_offset)
            if rows == 0:
                return out
            src, gain = _rows.source_rows(pairs), (ctypes.c_int32 * S)(*gains)
            mix = _lib.MixRows(S, src, gain, active.data_ptr() if active is not None else None)
            return _rows.repack(self, mix, _lib.AC_IN_MIX, out, rb)
        # the composition: every source unpacked, the rows mixed at the budget, rows longer than their slot marked, then the
        # packer at the fixed row starts (on plain allocations: nothing here may wait for the device)
        unpacked = [self.psy.unpack(d, ix) for d, ix in pairs]
        return _rows.pack_quantized(self.psy, self.psy.mix_to_budget(unpacked, gains, self.row_bits, active), rb, return_offset)

    # ---- routing the packed rows of several sources to several mixes (extension) --------------
    @staticmethod
    def mix_minus_routes(sources_n, gains=None):
        """The route table of a conference bridge for :meth:`route_packed_rows`: ``sources_n`` outputs, output o hears every
        source but o, source i at ``gains[i]`` (default 0) -- ``None`` on the diagonal."""
        if isinstance(sources_n, bool) or not isinstance(sources_n, (int, np.integer)):
            raise TypeError("sources_n must be an int, got %s" % type(sources_n).__name__)
        if sources_n < 1:
            raise ValueError("mix_minus_routes needs at least one source, got %d" % sources_n)
        gains = PsychoacousticModel._check_gains(gains, int(sources_n))
        return [[None if i == o else gains[i] for i in range(sources_n)] for o in range(sources_n)]

    @staticmethod
    def _check_routes(routes, sources_n):
        """``routes`` of :meth:`route_packed_rows` as a list of O >= 1 lists of ``sources_n`` entries, each an int in
        [-254, 254] or None."""
        routes = [list(row) for row in routes]
        if not routes:
            raise ValueError("route_packed_rows needs at least one output")
        for o, row in enumerate(routes):
            if len(row) != sources_n:
                raise ValueError("route %d has %d entries for %d sources" % (o, len(row), sources_n))
            for g in row:
                if g is None:
                    continue
                if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
                    raise TypeError("a route's gain must be an int (scale-factor units of 2^(1/4)) or None, got %s" % type(g).__name__)
                if not -254 <= int(g) <= 254:
                    raise ValueError("gain (%d) of route %d outside [-254, 254]" % (g, o))
        return [[None if g is None else int(g) for g in row] for row in routes]

    def route_packed_rows_launches(self, channels_n=2, device=None, *, sources_n, outputs_n):
        """Library launches :meth:`route_packed_rows` takes for ``outputs_n`` outputs that each hear ``sources_n`` sources of
        ``channels_n`` channels (``ac_route_launches``): 1 = one kernel stages every source row once and packs every output's
        row from it (where :meth:`mix_packed_rows_launches` is 1, ``sources_n`` is at most ``_lib.AC_ROUTE_MAX_SOURCES`` and ``outputs_n`` at most
        ``_lib.AC_ROUTE_MAX_OUTPUTS``),
        else ``outputs_n`` times :meth:`mix_packed_rows_launches`, the composition (everywhere while ``AC_ROUTE_NOFUSE=1`` is
        set: read per call).  0 on a codec without a row budget."""
        return self._launches(self._lib.ac_route_launches, device, channels_n, sources_n, outputs_n, mdct=False)

    def route_packed_rows(self, sources, routes, active=None, return_offset=False):
        """On a codec made by :meth:`with_bitrate` / :meth:`with_row_budget`: the packed rows of S sources -> O mixes of
        them at this codec's bitrate, without decoding -- a bridge's mix-minus (:meth:`mix_minus_routes`), monitor mixes,
        talk-over at a level per listener.  ``sources`` and ``active`` are :meth:`mix_packed_rows`'; ``routes`` holds O >= 1
        sequences of S entries, each an int gain in [-254, 254] in scale-factor units or ``None``: the output does not hear
        that source -> (data' uint8 [O, B*F*C*row_bytes], index' int64 [B, F, C], fits' bool [O, B, F, C]), and offset int16
        [O, B, F, C] with ``return_offset=True``.  ``(data'[o], index')`` is a packed-rows pair as
        :meth:`encode_packed_rows` returns it.

        Output o is, byte for byte, flags and offsets included, ``mix_packed_rows`` of the sources it hears, in source order,
        at its gains, with their part of ``active``; an output that hears nothing holds the slots of a mix whose sources are
        all inactive.  A damaged row or a band without a finite scale factor spoils only the outputs that hear it, and a row
        that no output hears is never read.  One launch where :meth:`route_packed_rows_launches` is 1 -- every source row is
        read and parsed once, not once per output that hears it -- else one :meth:`mix_packed_rows` per output: the same
        bytes.  It never synchronises with the device, only enqueues on the current stream, and can be captured in a graph.
        float32 only."""
        _host.require_float32(self.compute_dtype, "route_packed_rows")
        _rows.need_row_budget(self, "route_packed_rows")
        sources = list(sources)
        if not sources:
            raise ValueError("route_packed_rows needs at least one source")
        S = len(sources)
        routes = self._check_routes(routes, S)
        O = len(routes)
        pairs, shape, dev = _rows.check_sources(self.psy, sources)
        active = self.psy._check_active(active, S, shape, dev)
        rb = self.row_bytes
        out = _rows.outputs(shape, rb, dev, return_offset, lead=(O,))
        if pairs[0][1].numel() == 0:
            return out
        # (a single output's composition is one launch too: the switch itself decides there)
        if self._lib.ac_route_launches(self.psy._plan(dev), shape[2], S, O) == 1 and os.environ.get("AC_ROUTE_NOFUSE") != "1":
            src = _rows.source_rows(pairs)
            gain = (ctypes.c_int32 * (O * S))(*[_lib.AC_ROUTE_MUTE if g is None else g for row in routes for g in row])
            route = _lib.RouteRows(S, O, src, gain, active.data_ptr() if active is not None else None)
            return _rows.repack(self, route, _lib.AC_IN_ROUTE, out, rb)
        # the composition: one mix per output on the sources it hears (an output that hears nothing: source 0, never read)
        silent = None
        for o, row in enumerate(routes):
            inc = [i for i, g in enumerate(row) if g is not None]
            if inc:
                act = None if active is None else torch.stack([active[i] for i in inc])   # (no index tensor: nothing to upload)
                one = self.mix_packed_rows([pairs[i] for i in inc], [row[i] for i in inc], act, return_offset)
            else:
                if silent is None:
                    silent = torch.zeros((1,) + shape, dtype=torch.uint8, device=dev)
                one = self.mix_packed_rows(pairs[:1], [0], silent, return_offset)
            for mine, its in zip(out[:1] + out[2:], one[:1] + one[2:]):   # (data, fits and, asked for, offset)
                mine[o].copy_(its)
        return out

    # ---- the level of packed rows and the loudest sources (extension) ------------------------
    def packed_rows_level_launches(self, channels_n=2, device=None):
        """Library launches :meth:`packed_rows_level` takes for rows of ``channels_n`` channels (``ac_level_launches``): 1 =
        one kernel reads each row and sums its energy (filters_n = 1024, bark_bands_n = 64; any channel count; with or
        without a row budget), 0 = the library has no launch of its own and the method runs the composition on
        :meth:`PsychoacousticModel.unpack` and :meth:`PsychoacousticModel.level` (everywhere while ``AC_LEVEL_NOFUSE=1`` is
        set: read per call)."""
        return self._launches(self._lib.ac_level_launches, device, channels_n, mdct=False)

    def packed_rows_level(self, data, index, return_bad=False):
        """The energy of packed rows, from the rows themselves, without decoding: data uint8 [nbytes], index int64 [B, F, C]
        -> energy float32 [B, F, C], and bad uint8 [B, F, C] with ``return_bad=True``.

        ``energy`` is the sum of the squared dequantised spectrum over the row's bins (DESIGN.md section 8j has the exact
        arithmetic; within 2^-20 relative of the float64 sum), finite and never negative; by Parseval it follows the PCM
        energy of the frame's window.  A band without a finite scale factor adds nothing and sets ``bad`` for its row: marked
        rows, damaged widths, NaN-carrying input.  ``index`` holds any row starts, read as
        :meth:`PsychoacousticModel.unpack` reads them: :meth:`encode_packed` output, fixed-stride rows, protected slots,
        slices, a stream's chunks.  One launch where :meth:`packed_rows_level_launches` is 1, else the composition: the same
        bits.  It never synchronises with the device, only enqueues on the current stream, and can be captured in a graph.
        Works with or without a row budget.  float32 only."""
        _host.require_float32(self.compute_dtype, "packed_rows_level")
        data, index = _rows.check_pair(self.psy, data, index)
        shape, dev = tuple(index.shape), data.device
        if index.numel() == 0 or self._lib.ac_level_launches(self.psy._plan(dev), shape[2]) == 1:
            energy = torch.empty(shape, dtype=torch.float32, device=dev)
            bad = torch.empty(shape, dtype=torch.uint8, device=dev) if return_bad else None
            if index.numel():
                _rows.fused_ex(self, dev, _rows.packed_rows(data, index), _lib.AC_IN_PACKED | _lib.AC_EMIT_LEVEL, energy, bad,
                               shape)
            return (energy, bad) if return_bad else energy
        # the composition (the kernel's reference): the rows unpacked, then the band sums and the fold tree as tensor operations
        energy, bad = self.psy.level(*self.psy.unpack(data, index))
        return (energy, bad) if return_bad else energy

    def select_loudest(self, energy, n, valid=None, release=0.5, gate=0.0, state=None):
        """The ``n`` loudest of S sources per clip and frame: the levels of :meth:`packed_rows_level` -> ``active`` uint8
        [S, B, F, C], ready for ``mix_packed_rows(active=)`` and ``route_packed_rows(active=)``.

        ``energy``: a list of S float32 tensors [B, F, C] or one stacked tensor [S, B, F, C]; ``valid``: uint8 / bool
        [S, B, F, C], 0 = the row does not count and is never active (a lost or bad row; default all 1).  A source's level
        at a frame is the sum of its valid channels' energies (NaN, negative values and -0 count as 0), held as a peak that
        falls by ``release`` in [0, 1] per frame: ``P[f] = max(level[f], P[f-1] * release)``.  A source is selected where
        its peak is above ``gate`` >= 0 and fewer than ``n`` sources are louder (of equal peaks the lower index is the
        louder); ``active`` is the selection on the valid rows.  ``state``: float32 [S, B], the peaks carried from one chunk
        of frames to the next, updated in place (default: zeros, nothing kept) -- any split of the frames gives the bits of
        the one-shot call.  One launch for S <= ``_lib.AC_SELECT_MAX_SOURCES``; more sources take a loop of tensor
        operations over the frames, a slow reference route with the same values.  It never synchronises with the device,
        only enqueues on the current stream, and can be captured in a graph."""
        # (the host arguments first: their errors need no device)
        parts = None
        if isinstance(energy, torch.Tensor):
            if energy.dim() != 4:
                raise ValueError("energy must have 4 dimensions [S, B, F, C], got shape %s" % (tuple(energy.shape),))
            S = energy.shape[0]
        else:
            parts = list(energy)
            S = len(parts)
        if S < 1:
            raise ValueError("energy: select_loudest needs at least one source")
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
            raise TypeError("n must be an int, got %s" % type(n).__name__)
        if not 0 <= int(n) <= S:
            raise ValueError("n (%d) outside [0, %d sources]" % (n, S))
        for name, v in (("release", release), ("gate", gate)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise TypeError("%s must be a number, got %s" % (name, type(v).__name__))
        release, gate = float(np.float32(release)), float(np.float32(gate))
        if not 0.0 <= release <= 1.0:
            raise ValueError("release (%r) outside [0, 1]" % release)
        if not gate >= 0.0:
            raise ValueError("gate (%r) is negative or NaN" % gate)
        if parts is None:
            energy = self.psy._check_quant_tensor(energy, "energy", torch.float32, ndim=4)
        else:
            parts = [self.psy._check_quant_tensor(e, "energy of source %d" % i, torch.float32, ndim=3) for i, e in enumerate(parts)]
            for i, e in enumerate(parts):
                if e.shape != parts[0].shape or e.device != parts[0].device:
                    raise ValueError("energy of source %d has shape %s on %s, that of source 0 shape %s on %s"
                                     % (i, tuple(e.shape), e.device, tuple(parts[0].shape), parts[0].device))
            energy = torch.stack(parts)
        S, B, F, C = energy.shape
        dev = energy.device
        if valid is not None:
            if not isinstance(valid, torch.Tensor):
                raise TypeError("valid must be a torch.Tensor or None, got %s" % type(valid).__name__)
            if valid.dtype not in (torch.uint8, torch.bool):
                raise ValueError("valid has dtype %s, expected torch.uint8 or torch.bool" % valid.dtype)
            if tuple(valid.shape) != (S, B, F, C):
                raise ValueError("valid must have shape %s, got %s" % ((S, B, F, C), tuple(valid.shape)))
            if valid.device != dev:
                raise ValueError("valid lives on %s but energy on %s" % (valid.device, dev))
            valid = valid.contiguous()
            valid = valid.view(torch.uint8) if valid.dtype == torch.bool else valid
        if state is not None:
            if not isinstance(state, torch.Tensor):
                raise TypeError("state must be a torch.Tensor or None, got %s" % type(state).__name__)
            if state.dtype != torch.float32 or tuple(state.shape) != (S, B) or state.device != dev or not state.is_contiguous():
                raise ValueError("state must be a contiguous float32 tensor of shape %s on %s, got %s %s on %s"
                                 % ((S, B), dev, state.dtype, tuple(state.shape), state.device))
        active = torch.empty((S, B, F, C), dtype=torch.uint8, device=dev)
        if B * F * C == 0:
            return active
        if S <= _lib.AC_SELECT_MAX_SOURCES:
            sel = _lib.SelectRows(S, energy.data_ptr(), valid.data_ptr() if valid is not None else None, int(n), release, gate,
                                  state.data_ptr() if state is not None else None)
            _rows.fused_ex(self, dev, sel, _lib.AC_SELECT_ACTIVE, active, None, (B, F, C))
            return active
        # more sources than a wave has lanes: the rules frame by frame as tensor operations (slow; the same values)
        ok = energy > 0
        if valid is not None:
            ok &= valid != 0
        level = torch.where(ok, energy, 0.0)
        total = level[..., 0]
        for c in range(1, C):
            total = total + level[..., c]
        P = state.clone() if state is not None else torch.zeros((S, B), dtype=torch.float32, device=dev)
        src = torch.arange(S, device=dev)
        first = (src.view(1, S) < src.view(S, 1)).unsqueeze(2)      # [s, t, 1]: t comes before s
        for f in range(F):
            d = P * release
            P = torch.where(d > total[:, :, f], d, total[:, :, f])
            above = ((P.unsqueeze(0) > P.unsqueeze(1)) | ((P.unsqueeze(0) == P.unsqueeze(1)) & first)).sum(dim=1)
            chosen = ((P > gate) & (above < int(n))).unsqueeze(2)
            active[:, :, f, :] = chosen if valid is None else chosen & (valid[:, :, f, :] != 0)
        if state is not None:
            state.copy_(P)
        return active

    # ---- protected rows: a redundant copy of the frame before in every slot (extension) ---
    def _check_red_bits(self, red_bits, what):
        _rows.need_row_budget(self, what)
        if isinstance(red_bits, bool) or not isinstance(red_bits, (int, np.integer)):
            raise TypeError("red_bits must be an int, got %s" % type(red_bits).__name__)
        if red_bits < 5 * self.psy.bark_bands_n:
            raise ValueError("red_bits (%d) below 5 * bark_bands_n = %d, the length of a row that stores no band"
                             % (red_bits, 5 * self.psy.bark_bands_n))
        return int(red_bits)

    def _redundant_codec(self, red_bits):
        """``with_row_budget(red_bits)``, kept: its plan is created once (creating one waits for the device).  The kept codec
        holds no reference back to this one, so both are freed -- and their plans destroyed -- when the last reference goes,
        never later by the garbage collector (a plan destroyed in the middle of another call's graph capture ends it)."""
        if red_bits not in self._red_codecs:
            self._red_codecs[red_bits] = self.with_row_budget(red_bits)
        return self._red_codecs[red_bits]

    def protected_slot_bytes(self, red_bits):
        """Bytes of a slot of :meth:`protect_packed_rows`: :attr:`row_bytes` + ceil(red_bits / 32) * 4."""
        red_bits = self._check_red_bits(red_bits, "protected_slot_bytes")
        return self.row_bytes + (red_bits + 31) // 32 * 4

    def protect_packed_rows_launches(self, channels_n=2, device=None, *, red_bits):
        """Library launches :meth:`protect_packed_rows` takes for rows of ``channels_n`` channels (``ac_protect_launches``):
        1 = one kernel reads each row once and packs it at both budgets (where :meth:`transrate_packed_rows_launches` is 1
        and ``red_bits`` is at most ``_lib.AC_PACK_ROWS_MAX_BITS``), else those of the two :meth:`transrate_packed_rows`
        calls of the composition (everywhere while ``AC_PROTECT_NOFUSE=1`` is set: read per call).  0 on a codec without
        a row budget."""
        dev = _host.default_device(device)
        if self.row_bits is None:   # (ahead of the look at red_bits)
            return 0
        # (not through _launches: channels_n is looked at ahead of red_bits)
        return int(self._lib.ac_protect_launches(self.psy._plan(dev), int(channels_n), self._check_red_bits(red_bits, "")))

    def protect_packed_rows(self, data, index, red_bits, return_offset=False):
        """On a codec made by :meth:`with_bitrate` / :meth:`with_row_budget`: :meth:`transrate_packed_rows` into slots that
        also carry a copy of the frame before at the budget ``red_bits`` (in-band redundancy).  data
        uint8 [nbytes], index int64 [B, F, C] (any row starts) -> (data' uint8 [B*F*C*slot_bytes], index' int64 [B, F, C],
        fits bool [B, F, C], red_fits bool [B, F, C]), then offset and red_offset int16 [B, F, C] with
        ``return_offset=True``; ``slot_bytes`` = :meth:`protected_slot_bytes` and ``index'[b, f, c]`` = the slot's start.

        The first :attr:`row_bytes` bytes of slot (b, f, c) are the slot :meth:`transrate_packed_rows` writes for the row,
        with its ``fits`` and ``offset``.  The rest is, for f >= 1, the slot ``with_row_budget(red_bits)`` writes for the
        *input* row (b, f-1, c) -- the marked row where even offset 254 does not fit, ``red_fits`` False -- and zero bytes
        for f = 0, ``red_fits`` True, ``red_offset`` 0.  ``index'`` points at the primary rows, so every reader of packed
        rows reads ``(data', index')`` as it is; ``decode_packed(..., lost=, redundant_at=row_bytes)`` recovers a lost row
        from the next slot.  One launch where :meth:`protect_packed_rows_launches` is 1, else the composition: the same
        bytes.  Never synchronises with the device, only enqueues on the current stream, and can be captured in a graph."""
        _host.require_float32(self.compute_dtype, "protect_packed_rows")
        red_bits = self._check_red_bits(red_bits, "protect_packed_rows")
        data, index = _rows.check_pair(self.psy, data, index)
        return _rows.protect(self, data, index, red_bits, return_offset)

    def protect_stream(self, batches_n, channels_n, red_bits, device=None):
        """On a codec with a row budget: a :class:`ProtectStream` for ``batches_n`` clips of ``channels_n`` channels --
        :meth:`protect_packed_rows` chunk by chunk, the copy of a chunk's last row carried into the next chunk's first
        slots ("Streams")."""
        _host.require_float32(self.compute_dtype, "protect_stream")
        return ProtectStream(self, batches_n, channels_n, self._check_red_bits(red_bits, "protect_stream"), device)

    # ---- rate control per clip (extension) ------------------------------------------------
    def clip_bits_for_bitrate(self, bits_per_second, frames_n, channels_n):
        """The clip budget of a per-channel bitrate: frames_n * channels_n rows of :meth:`row_bits_for_bitrate` bits each,
        rounded down to the 32 bits rows are padded to, so that a clip that met it takes at most that many bits of
        ``pack()``'s data.  Pass it to :meth:`encode_quantized_clip_budget`."""
        for name, v in (("frames_n", frames_n), ("channels_n", channels_n)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError("%s must be an int, got %s" % (name, type(v).__name__))
            if v < 0:
                raise ValueError("%s must not be negative, got %d" % (name, v))
        return int(frames_n) * int(channels_n) * 32 * (self.row_bits_for_bitrate(bits_per_second) // 32)

    def encode_quantized_clip_budget(self, x, clip_bits, min_offset=0, drown=0.0):
        """:meth:`encode`, then :meth:`PsychoacousticModel.quantize_to_clip_budget` on its X and threshold: x [B, K*N, C]
        -> (codes int16 [B, K+1, N, C], sf int8 [B, K+1, M, C], offset int16 [B, K+1, C], row_bits_out int32 [B, K+1, C],
        clip_bits_out int64 [B]).  ``clip_bits`` is an int (e.g. :meth:`clip_bits_for_bitrate` with frames_n = K + 1) or
        an int64 tensor [B].  float32 only, not differentiable."""
        X, thr = self._encode_for_quantizer(x, drown, "encode_quantized_clip_budget")
        return self.psy.quantize_to_clip_budget(X, thr, clip_bits, min_offset)

    def encode_packed_clip_budget(self, x, clip_bits, min_offset=0, drown=0.0):
        """:meth:`encode_quantized_clip_budget`, then :meth:`PsychoacousticModel.pack`: x [B, K*N, C] -> (data uint8
        [nbytes], index int64 [B, K+1, C], offset int16 [B, K+1, C]).  A clip that met its budget T takes at most T / 8
        bytes of ``data``; :meth:`decode_packed` reads the stream as it is.  Synchronises with the device; float32 only."""
        codes, sf, offset, _, _ = self.encode_quantized_clip_budget(x, clip_bits, min_offset, drown)
        data, index = self.psy.pack(codes, sf)
        return data, index, offset

    def decode_packed_launches(self, channels_n=2, device=None):
        """Launches :meth:`decode_packed` takes for ``channels_n`` channels (``ac_decode_packed_launches``): 1 = the
        synthesis reads the bitstream itself (filters_n = 1024, bark_bands_n = 64, mono / stereo), else 1 +
        :meth:`decode_quantized_launches`: :meth:`PsychoacousticModel.unpack`, then :meth:`decode_quantized`
        (everywhere while ``AC_DECODE_PACKED_NOFUSE=1`` is set: read per call)."""
        return self._launches(self._lib.ac_decode_packed_launches, device, channels_n)

    def decode_packed(self, data, index, pcm16=False, *, lost=None, max_age=8, redundant_at=None):
        """data uint8 [nbytes], index int64 [B, K', C] -> x [B, (K'+1)*N, C] (``torch.int16`` with ``pcm16=True``);
        bit-equal to ``decode_quantized(*psy.unpack(data, index), pcm16)``, that is to ``decode_quantized`` on the codes
        that were packed.  One launch that reads the bitstream in the synthesis -- no codes or scale factors are
        allocated -- where :meth:`decode_packed_launches` is 1; :meth:`PsychoacousticModel.unpack`, then
        :meth:`decode_quantized` elsewhere.  ``index`` may hold any row starts (a slice of frames, channels in another
        order, a strided view), and damaged rows read as :meth:`PsychoacousticModel.unpack` reads them.  float32 only.

        ``lost`` uint8 / bool [B, K', C] marks rows that did not arrive (nonzero), and they are concealed (DESIGN.md section
        8f): a lost row is read from the last row of its clip and channel that arrived, at most ``max_age`` (0 .. 31)
        frames back, with its scale factors lowered by 4 -- the spectrum halved, exactly -- per frame of age; a row
        without such a source is silence, so ``max_age=0`` is zero-filling.  Sources are looked for in this call's
        ``index`` only.  Bit-equal to :meth:`PsychoacousticModel.conceal_plan`, ``unpack`` at its row starts,
        :meth:`PsychoacousticModel.conceal_fade` and :meth:`decode_quantized`, which is what runs where
        :meth:`decode_packed_launches` is not 1; one launch where it is.  Only enqueues on the current stream.

        ``redundant_at`` (with ``lost``; an int in [1, 2^31)) recovers before it conceals: a lost row
        whose successor arrived is read from ``index[b, f+1, c] + redundant_at`` with no fade -- on the slots of
        :meth:`protect_packed_rows` with ``redundant_at=row_bytes``, the low-bitrate copy the next slot carries.  The decoder
        reads whatever lies there; a recovered row is no source of concealment.  The same composition with
        ``conceal_plan(..., redundant_at=)``, and still one launch where :meth:`decode_packed_launches` is 1."""
        _host.require_float32(self.compute_dtype, "decode_packed")
        if redundant_at is not None:
            if lost is None:
                raise ValueError("redundant_at without lost: a row is recovered only where lost marks it")
            redundant_at = self.psy._check_redundant_at(redundant_at)
        if lost is not None:   # the concealing kernel where packed rows are decoded in one launch, the composition elsewhere
            max_age = self.psy._check_max_age(max_age)
            data, index = _rows.check_pair(self.psy, data, index)
            lost = self.psy._check_lost(lost, index)
            if index.numel() and self.decode_packed_launches(index.shape[2], data.device) == 1:
                if redundant_at is None:
                    conceal = _lib.Conceal(lost.data_ptr(), max_age)
                else:
                    conceal = _lib.ConcealRedundant(lost.data_ptr(), max_age | _lib.AC_CONCEAL_REDUNDANT, redundant_at)
                return self._decode_packed_launch(data, index, pcm16, conceal)
            src_index, age = self.psy.conceal_plan(index, lost, data.numel(), max_age, redundant_at)
            codes, sf = self.psy.unpack(data, src_index)
            return self.decode_quantized(codes, self.psy.conceal_fade(sf, age), pcm16)
        if (isinstance(data, torch.Tensor) and isinstance(index, torch.Tensor) and data.is_cuda and index.dim() == 3
                and index.shape[1] >= 1 and self.decode_packed_launches(index.shape[2], data.device) == 1):
            return self._decode_packed_launch(*_rows.check_pair(self.psy, data, index), pcm16)
        codes, sf = self.psy.unpack(data, index)
        return self.decode_quantized(codes, sf, pcm16)

    def _decode_packed_launch(self, data, index, pcm16, conceal=None):
        """:meth:`decode_packed`'s one launch on a checked pair; ``conceal``: the ``ac_conceal`` struct of lost rows."""
        B, Kp, C = index.shape
        dev = data.device
        x, px, px16 = _host.pcm_out((B, (Kp + 1) * self.filters_n, C), pcm16, dev)
        rows = _rows.packed_rows(data, index)   # (this frame holds rows and conceal until the call is back)
        with _host.on_device(dev):
            _lib.check(self._lib.ac_decode_quantized(
                self.mdct._plan(dev), self.psy._plan(dev), ctypes.addressof(rows), None, px, px16,
                ctypes.addressof(conceal) if conceal is not None else None, B, Kp, C, _host.stream_ptr(dev)))
        return x

    def decode_into(self, X, x):
        """:meth:`decode` into a caller-owned PCM tensor ``x [B, (K'+1)*N, C]`` (``torch.int16`` selects 16-bit PCM);
        same exactness rules as :meth:`encode_into`."""
        if not isinstance(X, torch.Tensor) or X.dim() != 4:
            raise ValueError("X must be a [batches_n, blocks_n, filters_n, channels_n] tensor")
        self._check_io(X, "X", None, self.compute_dtype, None)
        B, Kp, N, C = X.shape
        if N != self.filters_n:
            raise ValueError("axis 2 of X (%d) != filters_n (%d)" % (N, self.filters_n))
        pcm16 = isinstance(x, torch.Tensor) and x.dtype == torch.int16
        if pcm16 and self.compute_dtype != torch.float32:
            raise ValueError("16-bit PCM output needs compute_dtype float32")
        self._check_io(x, "x", (B, (Kp + 1) * N, C), torch.int16 if pcm16 else self.compute_dtype, X.device)
        if self.compute_dtype != torch.float32:
            with _host.on_device(X.device):
                _lib.check(self._lib.ac_mdct_inverse_typed(self.mdct._plan(X.device), _host.ptr(X), _host.ptr(x),
                                                           self.mdct._dtype_id, B, Kp, C, _host.stream_ptr(X.device)))
            return
        fn = self._lib.ac_mdct_inverse_pcm16 if pcm16 else self._lib.ac_mdct_inverse
        with _host.on_device(X.device):
            _lib.check(fn(self.mdct._plan(X.device), _host.ptr(X), _host.ptr(x), B, Kp, C, _host.stream_ptr(X.device)))

