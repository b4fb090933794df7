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

from . import _host, _lib, placement
from .mdctransformer import MDCTransformer
from .psychoacoustic import PsychoacousticModel


def _pack_rows_of_spectra(psy, X, thr, index, row_bytes):
    """The tail of the composition of packed rows, shared by :meth:`AudioCodec.encode_packed_rows` and
    :meth:`StreamingMDCT.encode_packed_rows_chunk`: ``psy.quantize_to_budget`` at the model's budget on X, thr [B, F, N, C] (on
    plain allocations: nothing here may wait for the device), rows longer than their slot marked, then the packer at the fixed
    row starts ``index`` into zero-filled data.  Returns (data uint8 [B*F*C*row_bytes], fits bool [B, F, C]); everything is
    enqueued on the current stream."""
    B, F, _, C = X.shape
    dev = X.device
    row_bits, min_offset = psy.row_budget
    codes, sf, _, bits = psy.quantize_to_budget(X, thr, row_bits, min_offset)
    return _pack_rows_of_codes(psy, codes, sf, bits, index, row_bytes)


def _pack_rows_of_codes(psy, codes, sf, bits, index, row_bytes):
    """The tail of :func:`_pack_rows_of_spectra`, which :meth:`AudioCodec.mix_packed_rows`' composition shares: codes
    [B, F, N, C], sf (changed in place) and their packed lengths ``bits`` [B, F, C] -> (data, fits)."""
    B, F, _, C = codes.shape
    dev = codes.device
    fits = bits <= 8 * row_bytes
    sf.masked_fill_(~fits.unsqueeze(2), -128)   # width 31 follows whatever the codes are
    data = torch.zeros((B * F * C * row_bytes,), dtype=torch.uint8, device=dev)
    with _host.on_device(dev):
        _lib.check(_lib.load().ac_pack(psy._plan(dev), _host.ptr(codes), _host.ptr(sf), _host.ptr(index), _host.ptr(data), B, F, C,
                                       _host.stream_ptr(dev)))
    return data, fits


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
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return int(self._lib.ac_encode_launches(self.mdct._plan(dev), self.psy._plan(dev), int(channels_n)))

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
        N = self.filters_n
        if S % N != 0:
            raise ValueError("samples_n (%d) is not a multiple of filters_n (%d)" % (S, N))
        K = S // N
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
        B, S, C = x.shape
        N = self.filters_n
        if S % N != 0:
            raise ValueError("samples_n (%d) is not a multiple of filters_n (%d)" % (S, N))
        K = S // N
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
        B, S, C = x.shape
        N = self.filters_n
        if S % N != 0:
            raise ValueError("samples_n (%d) is not a multiple of filters_n (%d)" % (S, N))
        K = S // N
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
        if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
            raise ValueError("x requires a gradient: quantisation is not differentiable -- use encode() and "
                             "psy.add_noise(), its differentiable stand-in")
        X, _, thr = self.encode(x, drown)
        return X, thr

    def encode_quantized_launches(self, channels_n=2, device=None, *, pcm16=False):
        """Launches :meth:`encode_quantized` takes for float32 PCM of ``channels_n`` channels
        (``ac_encode_quantized_launches``): 1 = the fused encode quantises the frame in its registers (filters_n = 1024, mono /
        stereo, spreading ``"f32"`` or ``"bf16x2_mfma"``), 2 = :meth:`encode`, then the quantiser.  ``pcm16=True``: for
        ``torch.int16`` PCM (``ac_encode_quantized_launches_pcm16``)."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        query = self._lib.ac_encode_quantized_launches_pcm16 if pcm16 else self._lib.ac_encode_quantized_launches
        return int(query(self.mdct._plan(dev), self.psy._plan(dev), int(channels_n)))

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
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return int(self._lib.ac_decode_quantized_launches(self.mdct._plan(dev), self.psy._plan(dev), int(channels_n)))

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
        x = torch.empty((B, (Kp + 1) * N, C), dtype=torch.int16 if pcm16 else torch.float32, device=dev)
        mdct, psy = self.mdct._plan(dev), self.psy._plan(dev)
        scratch = None
        if self._lib.ac_decode_quantized_launches(mdct, psy, C) != 1:
            scratch = torch.empty((B, Kp, N, C), dtype=torch.float32, device=dev)
        with _host.on_device(dev):
            _lib.check(self._lib.ac_decode_quantized(
                mdct, psy, _host.ptr(codes), _host.ptr(sf), None if pcm16 else _host.ptr(x), _host.ptr(x) if pcm16 else None,
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
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        query = self._lib.ac_encode_packed_launches_pcm16 if pcm16 else self._lib.ac_encode_packed_launches
        return int(query(self.mdct._plan(dev), self.psy._plan(dev), int(channels_n)))

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
        if self.row_bits is None:
            raise ValueError("encode_packed_rows needs a codec with a row budget: make one with with_bitrate() or "
                             "with_row_budget()")
        if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
            raise ValueError("x requires a gradient: quantisation is not differentiable -- use encode() and "
                             "psy.add_noise(), its differentiable stand-in")
        pcm16 = isinstance(x, torch.Tensor) and x.dtype == torch.int16
        x = _host.check_device_tensor(x, "x", torch.int16 if pcm16 else torch.float32, 3)
        B, S, C = x.shape
        N = self.filters_n
        if S % N != 0:
            raise ValueError("samples_n (%d) is not a multiple of filters_n (%d)" % (S, N))
        K = S // N
        F, dev, rb = K + 1, x.device, self.row_bytes
        rows = B * F * C
        index = (torch.arange(rows, dtype=torch.int64, device=dev) * rb).view(B, F, C)
        if rows == 0:
            return (torch.empty((0,), dtype=torch.uint8, device=dev), index, torch.empty((B, F, C), dtype=torch.bool, device=dev))
        mdct, psy = self.mdct._plan(dev), self.psy._plan(dev)
        if (self._lib.ac_encode_packed_launches_pcm16 if pcm16 else self._lib.ac_encode_packed_launches)(mdct, psy, C) == 1:
            data = torch.empty((rows * rb,), dtype=torch.uint8, device=dev)
            fits = torch.empty((B, F, C), dtype=torch.bool, device=dev)
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
        data, fits = _pack_rows_of_spectra(self.psy, X, thr, index, rb)
        return data, index, fits

    # ---- transrating packed rows (extension) ----------------------------------------------
    def transrate_packed_rows_launches(self, channels_n=2, device=None):
        """Library launches :meth:`transrate_packed_rows` takes for rows of ``channels_n`` channels
        (``ac_transrate_launches``): 1 = one kernel reads, requantises and packs each row (filters_n = 1024, bark_bands_n =
        64, a budget of at most ``_lib.AC_PACK_ROWS_MAX_BITS``; any channel count), else 3: :meth:`PsychoacousticModel.unpack`,
        :meth:`PsychoacousticModel.requantize_to_budget` and the packer (everywhere while ``AC_TRANSRATE_NOFUSE=1`` is set:
        read per call).  0 on a codec without a row budget."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return int(self._lib.ac_transrate_launches(self.psy._plan(dev), int(channels_n)))

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
        if self.row_bits is None:
            raise ValueError("transrate_packed_rows needs a codec with a row budget: make one with with_bitrate() or "
                             "with_row_budget()")
        data = self.psy._check_quant_tensor(data, "data", torch.uint8, ndim=1)
        index = self.psy._check_quant_tensor(index, "index", torch.int64, device=data.device, ndim=3)
        B, F, C = index.shape
        dev, rb = data.device, self.row_bytes
        rows = B * F * C
        index_out = (torch.arange(rows, dtype=torch.int64, device=dev) * rb).view(B, F, C)
        if rows == 0:
            out = (torch.empty((0,), dtype=torch.uint8, device=dev), index_out, torch.empty((B, F, C), dtype=torch.bool, device=dev))
            return out + (torch.empty((B, F, C), dtype=torch.int16, device=dev),) if return_offset else out
        psy = self.psy._plan(dev)
        if self._lib.ac_transrate_launches(psy, C) == 1:
            out_data = torch.empty((rows * rb,), dtype=torch.uint8, device=dev)
            fits = torch.empty((B, F, C), dtype=torch.bool, device=dev)
            offset = torch.empty((B, F, C), dtype=torch.int16, device=dev) if return_offset else None
            src = _lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr())
            dst = _lib.PackedOut(out_data.data_ptr(), rb, fits.data_ptr())
            with _host.on_device(dev):
                _lib.check(self._lib.ac_encode_fused_ex(self.mdct._plan(dev), psy, ctypes.addressof(src), None, None, None, 0.0,
                                                        _lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED, ctypes.addressof(dst),
                                                        _host.ptr(offset) if return_offset else None, 0, B, F - 1, C,
                                                        _host.stream_ptr(dev)))
            return (out_data, index_out, fits, offset) if return_offset else (out_data, index_out, fits)
        # the composition: the rows unpacked, requantised at the budget from offset 0, rows longer than their slot marked, then
        # the packer at the fixed row starts (on plain allocations: nothing here may wait for the device)
        codes, sf = self.psy.unpack(data, index)
        codes, sf, offset, bits = self.psy.requantize_to_budget(codes, sf, self.row_bits, 0)
        fits = bits <= 8 * rb
        sf.masked_fill_(~fits.unsqueeze(2), -128)   # width 31 follows whatever the codes are
        out_data = torch.zeros((rows * rb,), dtype=torch.uint8, device=dev)
        with _host.on_device(dev):
            _lib.check(self._lib.ac_pack(psy, _host.ptr(codes), _host.ptr(sf), _host.ptr(index_out), _host.ptr(out_data), B, F, C,
                                         _host.stream_ptr(dev)))
        return (out_data, index_out, fits, offset) if return_offset else (out_data, index_out, fits)

    # ---- mixing the packed rows of several sources (extension) ----------------------------
    def mix_packed_rows_launches(self, channels_n=2, device=None, *, sources_n):
        """Library launches :meth:`mix_packed_rows` takes for ``sources_n`` sources of ``channels_n`` channels
        (``ac_mix_launches``): 1 = one kernel reads, sums, quantises and packs each row (where
        :meth:`transrate_packed_rows_launches` is 1 and ``sources_n`` is at most ``_lib.AC_MIX_MAX_SOURCES``), else
        ``2 * sources_n + 2``: :meth:`PsychoacousticModel.unpack` and ``dequantize`` per source, ``quantize_to_budget`` and the
        packer (everywhere while ``AC_MIX_NOFUSE=1`` is set: read per call).  0 on a codec without a row budget."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return int(self._lib.ac_mix_launches(self.psy._plan(dev), int(channels_n), int(sources_n)))

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
        if self.row_bits is None:
            raise ValueError("mix_packed_rows needs a codec with a row budget: make one with with_bitrate() or with_row_budget()")
        sources = list(sources)
        if not sources:
            raise ValueError("mix_packed_rows needs at least one source")
        S = len(sources)
        gains = self.psy._check_gains(gains, S)
        pairs = []
        for i, (data, index) in enumerate(sources):
            data = self.psy._check_quant_tensor(data, "data of source %d" % i, torch.uint8, ndim=1)
            index = self.psy._check_quant_tensor(index, "index of source %d" % i, torch.int64, device=data.device, ndim=3)
            if pairs and (index.shape != pairs[0][1].shape or index.device != pairs[0][1].device):
                raise ValueError("index of source %d has shape %s on %s, that of source 0 shape %s on %s"
                                 % (i, tuple(index.shape), index.device, tuple(pairs[0][1].shape), pairs[0][1].device))
            pairs.append((data, index))
        B, F, C = pairs[0][1].shape
        dev, rb = pairs[0][1].device, self.row_bytes
        active = self.psy._check_active(active, S, (B, F, C), dev)
        rows = B * F * C
        index_out = (torch.arange(rows, dtype=torch.int64, device=dev) * rb).view(B, F, C)
        if rows == 0:
            out = (torch.empty((0,), dtype=torch.uint8, device=dev), index_out, torch.empty((B, F, C), dtype=torch.bool, device=dev))
            return out + (torch.empty((B, F, C), dtype=torch.int16, device=dev),) if return_offset else out
        psy = self.psy._plan(dev)
        if self._lib.ac_mix_launches(psy, C, S) == 1:
            out_data = torch.empty((rows * rb,), dtype=torch.uint8, device=dev)
            fits = torch.empty((B, F, C), dtype=torch.bool, device=dev)
            offset = torch.empty((B, F, C), dtype=torch.int16, device=dev) if return_offset else None
            src = (_lib.PackedRows * S)(*[_lib.PackedRows(d.data_ptr(), d.numel(), ix.data_ptr()) for d, ix in pairs])
            gain = (ctypes.c_int32 * S)(*gains)
            mix = _lib.MixRows(S, src, gain, active.data_ptr() if active is not None else None)
            dst = _lib.PackedOut(out_data.data_ptr(), rb, fits.data_ptr())
            with _host.on_device(dev):
                _lib.check(self._lib.ac_encode_fused_ex(self.mdct._plan(dev), psy, ctypes.addressof(mix), None, None, None, 0.0,
                                                        _lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED | _lib.AC_IN_MIX,
                                                        ctypes.addressof(dst), _host.ptr(offset) if return_offset else None, 0,
                                                        B, F - 1, C, _host.stream_ptr(dev)))
            return (out_data, index_out, fits, offset) if return_offset else (out_data, index_out, fits)
        # the composition: every source unpacked, the rows mixed at the budget, rows longer than their slot marked, then the
        # packer at the fixed row starts (on plain allocations: nothing here may wait for the device)
        unpacked = [self.psy.unpack(d, ix) for d, ix in pairs]
        codes, sf, offset, bits = self.psy.mix_to_budget(unpacked, gains, self.row_bits, active)
        out_data, fits = _pack_rows_of_codes(self.psy, codes, sf, bits, index_out, rb)
        return (out_data, index_out, fits, offset) if return_offset else (out_data, index_out, fits)

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
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return int(self._lib.ac_route_launches(self.psy._plan(dev), int(channels_n), int(sources_n), int(outputs_n)))

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
        if self.row_bits is None:
            raise ValueError("route_packed_rows needs a codec with a row budget: make one with with_bitrate() or with_row_budget()")
        sources = list(sources)
        if not sources:
            raise ValueError("route_packed_rows needs at least one source")
        S = len(sources)
        routes = self._check_routes(routes, S)
        O = len(routes)
        pairs = []
        for i, (data, index) in enumerate(sources):
            data = self.psy._check_quant_tensor(data, "data of source %d" % i, torch.uint8, ndim=1)
            index = self.psy._check_quant_tensor(index, "index of source %d" % i, torch.int64, device=data.device, ndim=3)
            if pairs and (index.shape != pairs[0][1].shape or index.device != pairs[0][1].device):
                raise ValueError("index of source %d has shape %s on %s, that of source 0 shape %s on %s"
                                 % (i, tuple(index.shape), index.device, tuple(pairs[0][1].shape), pairs[0][1].device))
            pairs.append((data, index))
        B, F, C = pairs[0][1].shape
        dev, rb = pairs[0][1].device, self.row_bytes
        active = self.psy._check_active(active, S, (B, F, C), dev)
        rows = B * F * C
        index_out = (torch.arange(rows, dtype=torch.int64, device=dev) * rb).view(B, F, C)
        out_data = torch.empty((O, rows * rb), dtype=torch.uint8, device=dev)
        fits = torch.empty((O, B, F, C), dtype=torch.bool, device=dev)
        offset = torch.empty((O, B, F, C), dtype=torch.int16, device=dev) if return_offset else None
        if rows == 0:
            return (out_data, index_out, fits, offset) if return_offset else (out_data, index_out, fits)
        psy = self.psy._plan(dev)
        # (a single output's composition is one launch too: the switch itself decides there)
        if self._lib.ac_route_launches(psy, C, S, O) == 1 and os.environ.get("AC_ROUTE_NOFUSE") != "1":
            src = (_lib.PackedRows * S)(*[_lib.PackedRows(d.data_ptr(), d.numel(), ix.data_ptr()) for d, ix in pairs])
            gain = (ctypes.c_int32 * (O * S))(*[_lib.AC_ROUTE_MUTE if g is None else g for row in routes for g in row])
            route = _lib.RouteRows(S, O, src, gain, active.data_ptr() if active is not None else None)
            dst = _lib.PackedOut(out_data.data_ptr(), rb, fits.data_ptr())
            with _host.on_device(dev):
                _lib.check(self._lib.ac_encode_fused_ex(self.mdct._plan(dev), psy, ctypes.addressof(route), None, None, None, 0.0,
                                                        _lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED | _lib.AC_IN_ROUTE,
                                                        ctypes.addressof(dst), _host.ptr(offset) if return_offset else None, 0,
                                                        B, F - 1, C, _host.stream_ptr(dev)))
            return (out_data, index_out, fits, offset) if return_offset else (out_data, index_out, fits)
        # the composition: one mix per output on the sources it hears (an output that hears nothing: source 0, never read)
        silent = None
        for o, row in enumerate(routes):
            inc = [i for i, g in enumerate(row) if g is not None]
            if inc:
                act = None if active is None else torch.stack([active[i] for i in inc])   # (no index tensor: nothing to upload)
                one = self.mix_packed_rows([pairs[i] for i in inc], [row[i] for i in inc], act, return_offset)
            else:
                if silent is None:
                    silent = torch.zeros((1, B, F, C), dtype=torch.uint8, device=dev)
                one = self.mix_packed_rows(pairs[:1], [0], silent, return_offset)
            out_data[o].copy_(one[0])
            fits[o].copy_(one[2])
            if return_offset:
                offset[o].copy_(one[3])
        return (out_data, index_out, fits, offset) if return_offset else (out_data, index_out, fits)

    # ---- the level of packed rows and the loudest sources (extension) ------------------------
    def packed_rows_level_launches(self, channels_n=2, device=None):
        """Library launches :meth:`packed_rows_level` takes for rows of ``channels_n`` channels (``ac_level_launches``): 1 =
        one kernel reads each row and sums its energy (filters_n = 1024, bark_bands_n = 64; any channel count; with or
        without a row budget), 0 = the library has no launch of its own and the method runs the composition on
        :meth:`PsychoacousticModel.unpack` and :meth:`PsychoacousticModel.level` (everywhere while ``AC_LEVEL_NOFUSE=1`` is
        set: read per call)."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return int(self._lib.ac_level_launches(self.psy._plan(dev), int(channels_n)))

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
        data = self.psy._check_quant_tensor(data, "data", torch.uint8, ndim=1)
        index = self.psy._check_quant_tensor(index, "index", torch.int64, device=data.device, ndim=3)
        B, F, C = index.shape
        dev = data.device
        if B * F * C == 0:
            energy = torch.empty((B, F, C), dtype=torch.float32, device=dev)
            return (energy, torch.empty((B, F, C), dtype=torch.uint8, device=dev)) if return_bad else energy
        psy = self.psy._plan(dev)
        if self._lib.ac_level_launches(psy, C) == 1:
            energy = torch.empty((B, F, C), dtype=torch.float32, device=dev)
            bad = torch.empty((B, F, C), dtype=torch.uint8, device=dev) if return_bad else None
            src = _lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr())
            with _host.on_device(dev):
                _lib.check(self._lib.ac_encode_fused_ex(self.mdct._plan(dev), psy, ctypes.addressof(src), None, None, None, 0.0,
                                                        _lib.AC_IN_PACKED | _lib.AC_EMIT_LEVEL, _host.ptr(energy),
                                                        _host.ptr(bad) if return_bad else None, 0, B, F - 1, C,
                                                        _host.stream_ptr(dev)))
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
            with _host.on_device(dev):
                _lib.check(self._lib.ac_encode_fused_ex(self.mdct._plan(dev), self.psy._plan(dev), ctypes.addressof(sel), None, None,
                                                        None, 0.0, _lib.AC_SELECT_ACTIVE, _host.ptr(active), None, 0, B, F - 1, C,
                                                        _host.stream_ptr(dev)))
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
        if self.row_bits is None:
            raise ValueError("%s needs a codec with a row budget: make one with with_bitrate() or with_row_budget()" % what)
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
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.row_bits is None:
            return 0
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
        data = self.psy._check_quant_tensor(data, "data", torch.uint8, ndim=1)
        index = self.psy._check_quant_tensor(index, "index", torch.int64, device=data.device, ndim=3)
        B, F, C = index.shape
        dev, rb = data.device, self.row_bytes
        sb = self.protected_slot_bytes(red_bits)
        rows = B * F * C
        index_out = (torch.arange(rows, dtype=torch.int64, device=dev) * sb).view(B, F, C)
        if rows == 0:
            flags = tuple(torch.empty((B, F, C), dtype=torch.bool, device=dev) for _ in range(2))
            offs = tuple(torch.empty((B, F, C), dtype=torch.int16, device=dev) for _ in range(2)) if return_offset else ()
            return (torch.empty((0,), dtype=torch.uint8, device=dev), index_out) + flags + offs
        psy = self.psy._plan(dev)
        if self._lib.ac_protect_launches(psy, C, red_bits) == 1:
            out_data = torch.empty((rows * sb,), dtype=torch.uint8, device=dev)
            fits = torch.empty((B, F, C), dtype=torch.bool, device=dev)
            red_fits = torch.empty((B, F, C), dtype=torch.bool, device=dev)
            offset = torch.empty((B, F, C), dtype=torch.int16, device=dev) if return_offset else None
            red_offset = torch.empty((B, F, C), dtype=torch.int16, device=dev) if return_offset else None
            src = _lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr())
            dst = _lib.ProtectedOut(out_data.data_ptr(), rb, fits.data_ptr(), red_bits, red_fits.data_ptr(),
                                    offset.data_ptr() if return_offset else None,
                                    red_offset.data_ptr() if return_offset else None)
            with _host.on_device(dev):
                _lib.check(self._lib.ac_encode_fused_ex(
                    self.mdct._plan(dev), psy, ctypes.addressof(src), None, None, None, 0.0,
                    _lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED | _lib.AC_EMIT_REDUNDANT, ctypes.addressof(dst), None, 0, B, F - 1,
                    C, _host.stream_ptr(dev)))
            out = (out_data, index_out, fits, red_fits)
            return out + (offset, red_offset) if return_offset else out
        # the composition: the rows transrated at both budgets, then copied into the two parts of every slot
        prim = self.transrate_packed_rows(data, index, True)
        red = self._redundant_codec(red_bits).transrate_packed_rows(data, index, True)
        slots = torch.zeros((B, F, C, sb), dtype=torch.uint8, device=dev)
        slots[..., :rb] = prim[0].view(B, F, C, rb)
        slots[:, 1:, :, rb:] = red[0].view(B, F, C, sb - rb)[:, :-1]
        red_fits = torch.ones((B, F, C), dtype=torch.bool, device=dev)
        red_fits[:, 1:] = red[2][:, :-1]
        out = (slots.view(-1), index_out, prim[2], red_fits)
        if return_offset:
            red_offset = torch.zeros((B, F, C), dtype=torch.int16, device=dev)
            red_offset[:, 1:] = red[3][:, :-1]
            out += (prim[3], red_offset)
        return out

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
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return int(self._lib.ac_decode_packed_launches(self.mdct._plan(dev), self.psy._plan(dev), int(channels_n)))

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
        if lost is not None:
            return self._decode_packed_concealed(data, index, pcm16, lost, max_age, redundant_at)
        if (isinstance(data, torch.Tensor) and isinstance(index, torch.Tensor) and data.is_cuda and index.dim() == 3
                and index.shape[1] >= 1 and self.decode_packed_launches(index.shape[2], data.device) == 1):
            data = self.psy._check_quant_tensor(data, "data", torch.uint8, ndim=1)
            index = self.psy._check_quant_tensor(index, "index", torch.int64, device=data.device, ndim=3)
            B, Kp, C = index.shape
            dev = data.device
            x = torch.empty((B, (Kp + 1) * self.filters_n, C), dtype=torch.int16 if pcm16 else torch.float32, device=dev)
            rows = _lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr())
            with _host.on_device(dev):
                _lib.check(self._lib.ac_decode_quantized(
                    self.mdct._plan(dev), self.psy._plan(dev), ctypes.addressof(rows), None,
                    None if pcm16 else _host.ptr(x), _host.ptr(x) if pcm16 else None, None, B, Kp, C,
                    _host.stream_ptr(dev)))
            return x
        codes, sf = self.psy.unpack(data, index)
        return self.decode_quantized(codes, sf, pcm16)

    def _decode_packed_concealed(self, data, index, pcm16, lost, max_age, redundant_at=None):
        """:meth:`decode_packed` with ``lost`` given: the concealing kernel where packed rows are decoded in one launch, the
        composition elsewhere."""
        max_age = self.psy._check_max_age(max_age)
        data = self.psy._check_quant_tensor(data, "data", torch.uint8, ndim=1)
        index = self.psy._check_quant_tensor(index, "index", torch.int64, device=data.device, ndim=3)
        lost = self.psy._check_lost(lost, index)
        B, Kp, C = index.shape
        dev = data.device
        if B >= 1 and Kp >= 1 and C >= 1 and self.decode_packed_launches(C, dev) == 1:
            x = torch.empty((B, (Kp + 1) * self.filters_n, C), dtype=torch.int16 if pcm16 else torch.float32, device=dev)
            rows = _lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr())
            if redundant_at is None:
                conceal = _lib.Conceal(lost.data_ptr(), max_age)
            else:
                conceal = _lib.ConcealRedundant(lost.data_ptr(), max_age | _lib.AC_CONCEAL_REDUNDANT, redundant_at)
            with _host.on_device(dev):
                _lib.check(self._lib.ac_decode_quantized(
                    self.mdct._plan(dev), self.psy._plan(dev), ctypes.addressof(rows), None,
                    None if pcm16 else _host.ptr(x), _host.ptr(x) if pcm16 else None, ctypes.addressof(conceal), B, Kp, C,
                    _host.stream_ptr(dev)))
            return x
        src_index, age = self.psy.conceal_plan(index, lost, data.numel(), max_age, redundant_at)
        codes, sf = self.psy.unpack(data, src_index)
        return self.decode_quantized(codes, self.psy.conceal_fade(sf, age), pcm16)

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
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
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
            B, k, C = index.shape
            if (B, C) != (self.B, self.C):
                raise ValueError("index must be [%d, k, %d], got %s" % (self.B, self.C, tuple(index.shape)))
            dev, rb, red_bits = self.device, codec.row_bytes, self.red_bits
            sb = codec.protected_slot_bytes(red_bits)
            rows = B * k * C
            index_out = (torch.arange(rows, dtype=torch.int64, device=dev) * sb).view(B, k, C)
            if k == 0:
                flags = tuple(torch.empty((B, k, C), dtype=torch.bool, device=dev) for _ in range(2))
                offs = tuple(torch.empty((B, k, C), dtype=torch.int16, device=dev) for _ in range(2)) if return_offset else ()
                return (torch.empty((0,), dtype=torch.uint8, device=dev), index_out) + flags + offs
            src_half = None if self._cur is None else self._carry[self._cur]
            nxt = 0 if self._cur is None else self._cur ^ 1
            dst_half = self._carry[nxt]
            psy = codec.psy._plan(dev)
            if codec._lib.ac_protect_chunk_launches(psy, C, red_bits) == 1:
                out_data = torch.empty((rows * sb,), dtype=torch.uint8, device=dev)
                fits = torch.empty((B, k, C), dtype=torch.bool, device=dev)
                red_fits = torch.empty((B, k, C), dtype=torch.bool, device=dev)
                offset = torch.empty((B, k, C), dtype=torch.int16, device=dev) if return_offset else None
                red_offset = torch.empty((B, k, C), dtype=torch.int16, device=dev) if return_offset else None
                src = _lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr())
                dst = _lib.ProtectedOut(out_data.data_ptr(), rb, fits.data_ptr(), red_bits, red_fits.data_ptr(),
                                        offset.data_ptr() if return_offset else None,
                                        red_offset.data_ptr() if return_offset else None)
                carry = _lib.ProtectCarry(*((None, None, None) if src_half is None else [t.data_ptr() for t in src_half]),
                                          *[t.data_ptr() for t in dst_half])
                with _host.on_device(dev):
                    _lib.check(codec._lib.ac_encode_fused_ex(
                        codec.mdct._plan(dev), psy, ctypes.addressof(src), None, None, None, 0.0,
                        _lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED | _lib.AC_EMIT_REDUNDANT | _lib.AC_EMIT_CARRY,
                        ctypes.addressof(dst), ctypes.addressof(carry), 0, B, k - 1, C,
                        _host.stream_ptr(dev) if stream is None else ctypes.c_void_p(stream.cuda_stream)))
                self._cur = nxt
                out = (out_data, index_out, fits, red_fits)
                return out + (offset, red_offset) if return_offset else out
            # the composition: the rows transrated at both budgets, copied into the slots; frame 0 from the carry, the copy of
            # the last row into the carry's other half
            prim = codec.transrate_packed_rows(data, index, True)
            red = codec._redundant_codec(red_bits).transrate_packed_rows(data, index, True)
            red_rows = red[0].view(B, k, C, sb - rb)
            slots = torch.zeros((B, k, C, sb), dtype=torch.uint8, device=dev)
            slots[..., :rb] = prim[0].view(B, k, C, rb)
            slots[:, 1:, :, rb:] = red_rows[:, :-1]
            red_fits = torch.ones((B, k, C), dtype=torch.bool, device=dev)
            red_fits[:, 1:] = red[2][:, :-1]
            red_offset = torch.zeros((B, k, C), dtype=torch.int16, device=dev)
            red_offset[:, 1:] = red[3][:, :-1]
            if src_half is not None:
                slots[:, 0, :, rb:] = src_half[0]
                red_fits[:, 0] = src_half[1]
                red_offset[:, 0] = src_half[2]
            dst_half[0].copy_(red_rows[:, -1])
            dst_half[1].copy_(red[2][:, -1])
            dst_half[2].copy_(red[3][:, -1])
            self._cur = nxt
            out = (slots.view(-1), index_out, prim[2], red_fits)
            return out + (prim[3], red_offset) if return_offset else out


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
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
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
        B, S, C = x.shape
        N = self.mdct.filters_n
        if (B, C) != (self.B, self.C) or S % N != 0:
            raise ValueError("x_chunk must be [%d, k*%d, %d], got %s" % (self.B, N, self.C, tuple(x.shape)))
        k = S // N
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
        B, S, C = x.shape
        N = self.mdct.filters_n
        if (B, C) != (self.B, self.C) or S % N != 0:
            raise ValueError("x_chunk must be [%d, k*%d, %d], got %s" % (self.B, N, self.C, tuple(x.shape)))
        k = S // N
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
        N, rb = self.mdct.filters_n, self.row_bytes
        with self._on(stream):
            pcm16 = isinstance(x_chunk, torch.Tensor) and x_chunk.dtype == torch.int16
            x = self._check_chunk(x_chunk, "x_chunk", 3, torch.int16 if pcm16 else None)
            B, S, C = x.shape
            if (B, C) != (self.B, self.C) or S % N != 0:
                raise ValueError("x_chunk must be [%d, k*%d, %d], got %s" % (self.B, N, self.C, tuple(x.shape)))
            k = S // N
            dev, rows = x.device, B * k * C
            index = (torch.arange(rows, dtype=torch.int64, device=dev) * rb).view(B, k, C)
            if rows == 0:
                return (torch.empty((0,), dtype=torch.uint8, device=dev), index,
                        torch.empty((B, k, C), dtype=torch.bool, device=dev))
            psy = self.psy._plan(dev)
            if pcm16 and self._lib.ac_stream_packed_launches_pcm16(self._handle, psy) != 1:
                x, pcm16 = x.to(torch.float32) / 32768, False
            if pcm16 or self._lib.ac_stream_packed_launches(self._handle, psy, 0) == 1:
                data = torch.empty((rows * rb,), dtype=torch.uint8, device=dev)
                fits = torch.empty((B, k, C), dtype=torch.bool, device=dev)
                out = _lib.PackedOut(data.data_ptr(), rb, fits.data_ptr())
                with _host.on_device(dev):
                    _lib.check(self._lib.ac_stream_encode_typed(self._handle, psy, _host.ptr(x), ctypes.addressof(out), None,
                                                                None, float(drown),
                                                                _lib.AC_PACKED | (_lib.AC_IN_PCM16 if pcm16 else 0), k,
                                                                self._stream(stream)))
                return data, index, fits
            X, _, thr = self.encode_chunk(x, drown, stream=stream)
            data, fits = _pack_rows_of_spectra(self.psy, X, thr, index, rb)
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
            dev = data.device
            psy = self.psy._plan(dev)
            if redundant_at is not None:
                if self._advanced:
                    raise ValueError("redundant_at on a stream whose synthesis has advanced without it since it was made or "
                                     "reset: a recovering chunk runs one frame behind its rows -- reset() first")
                self._decode_packed_chunk_recovered(data, index, lost, max_age, redundant_at, pcm16, x, psy, stream)
                self._delayed = True   # (the mode changes only once the chunk has gone through)
                return x
            self._not_delayed("decode_packed_chunk without redundant_at")
            if lost is not None:
                self._decode_packed_chunk_concealed(data, index, lost, max_age, pcm16, x, psy, stream)
            else:
                self._conceal = None   # (a chunk that does not conceal leaves no source; the library marks its own state)
                if self._lib.ac_stream_packed_launches(self._handle, psy, 1) == 1:
                    rows = _lib.StreamPackedIn(_lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr()), psy.value,
                                               1 if pcm16 else 0)
                    with _host.on_device(dev):
                        _lib.check(self._lib.ac_stream_inverse_typed(self._handle, ctypes.addressof(rows), _host.ptr(x),
                                                                     _lib.AC_PACKED, k, self._stream(stream)))
                else:
                    self._inverse_chunk_into(self.psy.dequantize(*self.psy.unpack(data, index)), x, pcm16, stream)
            self._advanced = True
            return x

    def _inverse_chunk_into(self, X, x, pcm16, stream):
        """:meth:`inverse_chunk` of X into x, through the 16-bit PCM store where x is int16."""
        if not pcm16:
            return self._inverse_chunk(X, x, stream)
        p = torch.nan_to_num(self._inverse_chunk(X, None, stream) * 32768.0, nan=0.0)   # the float32 product
        x.copy_(p.round_().clamp_(-32768.0, 32767.0).to(torch.int16))                   # round: half to even
        return x

    def _decode_packed_chunk_concealed(self, data, index, lost, max_age, pcm16, x, psy, stream):
        """:meth:`decode_packed_chunk` with ``lost`` given (checked; under the stream the work runs on): the one launch where
        the library has it, else the composition, which keeps the state the kernel keeps -- the carried row as
        ``psy.unpack`` read it, and the gap (frames since that row at the end of the chunk before; 32: none in reach) -- in
        ``self._conceal``.  Nothing here waits for the device."""
        B, k, C = index.shape
        dev = data.device
        if self._lib.ac_stream_packed_launches(self._handle, psy, 2) == 1:
            self._conceal = None   # (the state lives in the library from here on)
            rows = _lib.StreamPackedLostIn(
                _lib.StreamPackedIn(_lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr()), psy.value,
                                    1 if pcm16 else 0), lost.data_ptr(), max_age)
            with _host.on_device(dev):
                _lib.check(self._lib.ac_stream_inverse_typed(self._handle, ctypes.addressof(rows), _host.ptr(x),
                                                             _lib.AC_PACKED | _lib.AC_CONCEAL, k, self._stream(stream)))
            return x
        codes, sf = self.psy.unpack(data, index)
        state = self._conceal
        if state is None:   # a new stream, after reset(), or after a chunk that did not conceal: no source
            state = (torch.zeros_like(codes[:, :1]), torch.zeros_like(sf[:, :1]),
                     torch.full((B, C), 32, dtype=torch.int64, device=dev))
        row_codes, row_sf, gap = state
        # the carried row in front as frame -1; sources as DESIGN.md section 8f defines them
        codes_ext, sf_ext = torch.cat((row_codes, codes), dim=1), torch.cat((row_sf, sf), dim=1)
        f = torch.arange(k, dtype=torch.int64, device=dev).view(1, k, 1)
        last = f.expand(B, k, C).masked_fill(lost != 0, -1).cummax(dim=1).values   # the last frame <= f of the chunk that arrived
        inside = (last >= 0) & (f - last <= max_age)
        carried_age = gap.view(B, 1, C) + f + 1
        carried = ~inside & (gap.view(B, 1, C) <= 31) & (carried_age <= max_age)
        muted = ~inside & ~carried
        src = torch.where(inside, last + 1, torch.zeros_like(last))               # frame of codes_ext
        age = torch.where(inside, f - last, carried_age).masked_fill(muted, 0).to(torch.uint8)
        N, M = codes.shape[2], sf.shape[2]
        got_codes = codes_ext.gather(1, src.unsqueeze(2).expand(B, k, N, C)).masked_fill(muted.unsqueeze(2), 0)
        got_sf = sf_ext.gather(1, src.unsqueeze(2).expand(B, k, M, C)).masked_fill(muted.unsqueeze(2), 0)
        self._inverse_chunk_into(self.psy.dequantize(got_codes, self.psy.conceal_fade(got_sf, age)), x, pcm16, stream)
        # the state after the chunk, whatever max_age was
        final = last[:, -1]                                                         # [B, C]: f*, or -1
        has = final >= 0
        at = final.clamp(min=0).view(B, 1, 1, C)
        new_codes = torch.where(has.view(B, 1, 1, C), codes.gather(1, at.expand(B, 1, N, C)), row_codes)
        new_sf = torch.where(has.view(B, 1, 1, C), sf.gather(1, at.expand(B, 1, M, C)), row_sf)
        new_gap = torch.where(has, k - 1 - final, gap + k).clamp(max=32)
        self._conceal = (new_codes, new_sf, new_gap)   # (after inverse_chunk, which leaves no source)
        return x

    def _decode_packed_chunk_recovered(self, data, index, lost, max_age, redundant_at, pcm16, x, psy, stream):
        """:meth:`decode_packed_chunk` with ``redundant_at`` given (checked; under the stream the work runs on): the one
        launch where the library has it, else the composition on the same state as the concealing one keeps
        (``self._conceal``) -- the deferred row is the carried row where the gap is 0.  Nothing here waits for the device."""
        B, k, C = index.shape
        dev = data.device
        if self._lib.ac_stream_packed_launches(self._handle, psy, 3) == 1:
            self._conceal = None   # (the state lives in the library from here on)
            rows = _lib.StreamPackedRecoverIn(
                _lib.StreamPackedIn(_lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr()), psy.value,
                                    1 if pcm16 else 0), lost.data_ptr(), max_age | _lib.AC_CONCEAL_REDUNDANT, redundant_at)
            with _host.on_device(dev):
                _lib.check(self._lib.ac_stream_inverse_typed(self._handle, ctypes.addressof(rows), _host.ptr(x),
                                                             _lib.AC_PACKED | _lib.AC_CONCEAL, k, self._stream(stream)))
            return x
        # the chunk's rows and, behind them, the copies their slots carry: the copy in row j's slot is of frame j - 1
        codes, sf = self.psy.unpack(data, torch.cat((index, index + redundant_at), dim=1))
        codes, red_codes, sf, red_sf = codes[:, :k], codes[:, k:], sf[:, :k], sf[:, k:]
        state = self._conceal
        if state is None:   # a new stream or after reset(): the deferred row did not arrive and has no source
            state = (torch.zeros_like(codes[:, :1]), torch.zeros_like(sf[:, :1]),
                     torch.full((B, C), 32, dtype=torch.int64, device=dev))
        row_codes, row_sf, gap = state
        # frames j = 0 .. k of the delayed chunk: j = 0 is D, which arrived where the gap is 0, j = f + 1 is row f; the carried
        # row in front of the chunk's rows is frame 0 where it is D and the row gap frames before it otherwise
        codes_ext, sf_ext = torch.cat((row_codes, codes), dim=1), torch.cat((row_sf, sf), dim=1)
        arrived = torch.cat(((gap == 0).view(B, 1, C), lost == 0), dim=1)              # [B, k+1, C]
        j = torch.arange(k, dtype=torch.int64, device=dev).view(1, k, 1)
        last = j.expand(B, k, C).masked_fill(~arrived[:, :k], -1).cummax(dim=1).values   # the last frame <= j that arrived
        recovered = ~arrived[:, :k] & arrived[:, 1:]
        inside = (last >= 0) & (j - last <= max_age)
        carried_age = gap.view(B, 1, C) + j
        carried = ~inside & (gap.view(B, 1, C) <= 31) & (carried_age <= max_age)
        muted = ~inside & ~carried & ~recovered
        src = torch.where(inside, last, torch.zeros_like(last))                        # frame of codes_ext
        age = torch.where(inside, j - last, carried_age).masked_fill(muted | recovered, 0).to(torch.uint8)
        N, M = codes.shape[2], sf.shape[2]
        got_codes = codes_ext.gather(1, src.unsqueeze(2).expand(B, k, N, C)).masked_fill(muted.unsqueeze(2), 0)
        got_sf = sf_ext.gather(1, src.unsqueeze(2).expand(B, k, M, C)).masked_fill(muted.unsqueeze(2), 0)
        got_codes = torch.where(recovered.unsqueeze(2), red_codes, got_codes)
        got_sf = torch.where(recovered.unsqueeze(2), red_sf, got_sf)
        self._inverse_chunk_into(self.psy.dequantize(got_codes, self.psy.conceal_fade(got_sf, age)), x, pcm16, stream)
        # the state after the chunk, over its rows 0 .. k-1 whatever max_age was: as the concealing chunk leaves it
        f = torch.arange(k, dtype=torch.int64, device=dev).view(1, k, 1)
        final = f.expand(B, k, C).masked_fill(lost != 0, -1).max(dim=1).values          # [B, C]: the last row that arrived, or -1
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
